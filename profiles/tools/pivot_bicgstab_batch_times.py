"""ilupp_amd.device.bicgstab_batch (the whole left-preconditioned BiCGstab loop of every member in ONE launch, k_bicgstab_batch) next to
the loop of single solves ilupp_amd.device.bicgstab(A_k, b_k[:, None], PivotedOperator(P_k)) on the same objects, for 1, 16 and 64 members
of matgen.random_dd(n, 8, 25.0, seed), `iters` iterations each (rtol = 0: the work is fixed); a host clock around the call and a device
synchronisation; 2 warm-up and `reps` timed repetitions of each, alternating; median [min, max] in ms.
python profiles/tools/pivot_bicgstab_batch_times.py [reps [n,n,... [members,members,... [iters]]]]"""
import os, sys, time
import numpy as np
import scipy.sparse as sp
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import matgen
import ilupp_amd as ilupp
import ilupp_amd.device as ild

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4000, 1000]
counts = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 16, 64]
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 20
WARM = 2


def stats(v):
    return "%9.3f [%9.3f, %9.3f]" % (float(np.median(v)), min(v), max(v))


print("times in ms, median [min, max] of %d after %d warm-up calls; %d iterations per member" % (reps, WARM, iters))
for n in sizes:
    mats = [sp.csr_matrix(matgen.random_dd(n, 8, 25.0, 500 + k), shape=(n, n)) for k in range(max(counts))]
    As = [ild.DeviceCSR.from_scipy(A) for A in mats]
    for cls in (ilupp.ILUCPPreconditioner, ilupp.ILUTPPreconditioner):
        members = [ild.PivotedOperator(P) for P in cls.batch(mats)]
        for cnt in counts:
            A, M = As[:cnt], members[:cnt]
            offsets = [k * n for k in range(cnt)]
            b = torch.ones(cnt * n, dtype=torch.float64, device="cuda")
            kw = dict(maxiter=iters, rtol=0.0, check_every=0)

            def batched():
                return ild.bicgstab_batch(A, b, offsets, M, **kw)

            def looped():
                return [ild.bicgstab(a, b[o:o + n][:, None], m, **kw) for a, m, o in zip(A, M, offsets)]

            out = {batched: [], looped: []}
            for r in range(WARM + reps):
                for f in (batched, looped):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); f(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
                    if r >= WARM:
                        out[f].append(1e3 * dt)
            print("%s n %5d members %2d: batched %s  looped %s  batched / looped %.3f"
                  % (cls.__name__[:5], n, cnt, stats(out[batched]), stats(out[looped]), np.median(out[batched]) / np.median(out[looped])), flush=True)
        del members
