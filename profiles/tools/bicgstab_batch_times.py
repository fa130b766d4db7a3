"""ilupp_amd.device.bicgstab_batch with non-pivoting members (the whole left-preconditioned BiCGstab loop of every member in ONE launch,
k_bicgstab_batch) next to the loop of single solves ilupp_amd.device.bicgstab(A_k, b_k[:, None], M_k) on the same objects, for ILU0
members of matgen.random_dd(n, 8, 25.0, seed) as it comes (nonsymmetric), `iters` iterations each (rtol = 0: the work is fixed).  Two
parts: the solve alone, and the full step refactor_batch_(check=False) + bicgstab_batch against the loop of refactor_ + bicgstab.
(Pivoting members: profiles/tools/pivot_bicgstab_batch_times.py.)  A host clock around the call and a device synchronisation; 2 warm-up and `reps` timed repetitions of each, alternating; median [min, max] in ms.
python profiles/tools/bicgstab_batch_times.py [reps [iters]]"""
import os, sys, time
import numpy as np
import scipy.sparse as sp
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import matgen
import ilupp_amd.device as ild

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARM = 2
CASES = [(4000, 1), (4000, 16), (4000, 64), (1000, 1), (1000, 64)]          # (n, members)
STEP_CASES = [(4000, 16), (4000, 64)]
kw = dict(maxiter=iters, rtol=0.0, check_every=0)


def stats(v):
    return "%9.3f [%9.3f, %9.3f]" % (float(np.median(v)), min(v), max(v))


def side_by_side(first, second):
    out = {first: [], second: []}
    for r in range(WARM + reps):
        for f in (first, second):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); f(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if r >= WARM:
                out[f].append(1e3 * dt)
    return out[first], out[second]


print("times in ms, median [min, max] of %d after %d warm-up calls; %d iterations per member" % (reps, WARM, iters))
built = {}
for n in sorted(set(n for n, _ in CASES), reverse=True):
    mats = [sp.csr_matrix(matgen.random_dd(n, 8, 25.0, 500 + k), shape=(n, n)) for k in range(max(c for m, c in CASES if m == n))]
    As = [ild.DeviceCSR.from_scipy(A) for A in mats]
    built[n] = (mats, As, [ild.DevicePreconditioner("ILU0", A) for A in As])

print("# the solve: bicgstab_batch against the loop of bicgstab")
for n, cnt in CASES:
    A, M = built[n][1][:cnt], built[n][2][:cnt]
    offsets = [k * n for k in range(cnt)]
    b = torch.ones(cnt * n, dtype=torch.float64, device="cuda")

    def batched():
        return ild.bicgstab_batch(A, b, offsets, M, **kw)

    def looped():
        return [ild.bicgstab(a, b[o:o + n][:, None], m, **kw) for a, m, o in zip(A, M, offsets)]

    tb, tl = side_by_side(batched, looped)
    print("ILU0  n %5d members %2d: batched %s  looped %s  batched / looped %.3f" % (n, cnt, stats(tb), stats(tl), np.median(tb) / np.median(tl)),
          flush=True)

print("# the full step: refactor_batch_(check=False) + bicgstab_batch against the loop of refactor_ + bicgstab")
for n, cnt in STEP_CASES:
    A, M = built[n][1][:cnt], built[n][2][:cnt]
    offsets = [k * n for k in range(cnt)]
    b = torch.ones(cnt * n, dtype=torch.float64, device="cuda")

    def batched():
        ild.refactor_batch_(M, A, check=False)
        return ild.bicgstab_batch(A, b, offsets, M, **kw)

    def looped():
        return [ild.bicgstab(a, b[o:o + n][:, None], m.refactor_(a), **kw) for a, m, o in zip(A, M, offsets)]

    tb, tl = side_by_side(batched, looped)
    print("ILU0  n %5d members %2d: batched %s  looped %s  batched / looped %.3f" % (n, cnt, stats(tb), stats(tl), np.median(tb) / np.median(tl)),
          flush=True)
