"""ilupp_amd.device.bicgstab_batch with non-pivoting members (the whole left-preconditioned BiCGstab loop of every member in ONE launch,
k_bicgstab_batch) next to the loop of single solves ilupp_amd.device.bicgstab(A_k, b_k[:, None], M_k) on the same objects, for ILU0
members of matgen.random_dd(n, 8, 25.0, seed) as it comes (nonsymmetric), `iters` iterations each (rtol = 0: the work is fixed).  Three
parts: the solve alone; the full step refactor_batch_(check=False) + bicgstab_batch against the loop of refactor_ + bicgstab; and 16
ILUCP members through k_bicgstab_batch against the same 16 through k_pivot_bicgstab_batch.  A host clock around the call and a device
synchronisation; 2 warm-up and `reps` timed repetitions of each, alternating; median [min, max] in ms.
python profiles/tools/bicgstab_batch_times.py [reps [iters]]"""
import os, sys, time
import numpy as np
import scipy.sparse as sp
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import matgen
import ilupp_amd as ilupp
import ilupp_amd.device as ild
from ilupp_amd import _native

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

print("# 16 ILUCP members: k_bicgstab_batch (ilupp_hip_bicgstab_batch_device) against k_pivot_bicgstab_batch (bicgstab_batch on them alone)")
n, cnt = 4000, 16
mats, As = built[n][0][:cnt], built[n][1][:cnt]
natives = [ild.PivotedOperator(P).pr for P in ilupp.ILUCPPreconditioner.batch(mats)]
offsets = [k * n for k in range(cnt)]
b = torch.ones(cnt * n, dtype=torch.float64, device="cuda")
work = torch.empty(7 * cnt * n, dtype=torch.float64, device="cuda")
its = torch.zeros(cnt, dtype=torch.int64, device="cuda")
flags = torch.zeros(cnt, dtype=torch.int32, device="cuda")
rr, init = torch.zeros(cnt, dtype=torch.float64, device="cuda"), torch.zeros(cnt, dtype=torch.float64, device="cuda")
matrices = [(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr(), A.nnz) for A in As]
xs = {}


def new_kernel():
    x = torch.zeros_like(b)
    ild._on_current_stream()
    route = _native.bicgstab_batch_device(natives, [n] * cnt, matrices, b.data_ptr(), 0, x.data_ptr(), offsets, work.data_ptr(), work.numel(),
                                          iters, 0.0, 0, its.data_ptr(), flags.data_ptr(), rr.data_ptr(), init.data_ptr(), sync=False)
    assert route == [0] * cnt
    xs["new"] = x


def old_kernel():
    xs["old"] = ild.bicgstab_batch(As, b, offsets, natives, **kw)


tn, to = side_by_side(new_kernel, old_kernel)
assert torch.equal(xs["new"].view(torch.int64), xs["old"].view(torch.int64))
print("ILUCP n %5d members %2d: new kernel %s  old kernel %s  new / old %.3f (same bits)" % (n, cnt, stats(tn), stats(to), np.median(tn) / np.median(to)),
      flush=True)
