"""ILUCPPreconditioner / ILUTPPreconditioner: one construction next to batches of 16 and 64 (wall time and the chain kernel's time, warm, median
[min, max] of `reps` runs) on matgen.random_dd(n, 8, 25.0, seed): python profiles/tools/pivot_batch_times.py [n [reps]]"""
import os, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import matgen
import ilupp_amd as ilupp

n = int(sys.argv[1]) if len(sys.argv) > 1 else 12000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
mats = [sp.csr_matrix(matgen.random_dd(n, 8, 25.0, 500 + k), shape=(n, n)) for k in range(64)]


def stats(v):
    return "%.4f [%.4f, %.4f]" % (float(np.median(v)), min(v), max(v))


for cls in (ilupp.ILUCPPreconditioner, ilupp.ILUTPPreconditioner):
    cls(mats[0]); cls.batch(mats[:16])                                              # warm: pool, code objects
    wall, kern = [], []
    for r in range(reps):
        t0 = time.perf_counter(); P = cls(mats[0]); wall.append(time.perf_counter() - t0); kern.append(P.pr.kernel_ms)
    one = float(np.median(wall))
    print("%s n %d one: wall %s s, kernel %s ms, kernel / wall %.3f" % (cls.__name__, n, stats(wall), stats(kern), np.median(kern) / (1e3 * one)), flush=True)
    for cnt in (16, 64):
        wall, kern = [], []
        for r in range(reps):
            t0 = time.perf_counter(); B = cls.batch(mats[:cnt]); wall.append(time.perf_counter() - t0); kern.append(B[0].pr.kernel_ms)
            del B
        print("%s n %d batch of %d: wall %s s = %.2f x one, kernel %s ms" % (cls.__name__, n, cnt, stats(wall), np.median(wall) / one, stats(kern)), flush=True)
