"""The batched apply of multilevel ILU++ preconditioners (ilupp_amd.device.ml_apply_batch_ / ilupp_amd.ml_apply_batch: ONE launch of
k_ml_apply_batch, one workgroup per member walking its levels) next to the loop of single applies on the same objects in the same
process, and ilupp_amd.device.bicgstab_batch with MultilevelOperator members (k_bicgstab_batch<true>) next to the loop of
ilupp_amd.device.bicgstab(A_k, b_k[:, None], MultilevelOperator(P_k)).  Members: ILUppPreconditioner.batch of
ml_cases.weak_random(n, 6 / n, 1.0, seed), the family without pivoting (default_configuration(1), threshold 0.1, NORMALIZE_COLUMNS /
NORMALIZE_ROWS / PQ_ORDERING); the level counts and stored entries of the members are printed beside the figures.

    apply   16 and 64 members (and one alone) of n = 4 000 and n = 1 000, on device vectors and on host vectors
    solve   16 and 64 members of n = 1 000, `iters` iterations each (rtol = 0: the work is fixed; a member of n = 4 000 takes 0.115 s per
            single apply, so the loop of 16 such solves would take 75 s per repetition)
    lone    the lone-member rule: one member of n = 4 000 (launch) and n = 8 000 (route 1) against its single apply, and two members of
            n = 8 000 in one launch -- two workgroups side by side, i.e. what one workgroup needs for such a member
    guard   bicgstab_batch WITHOUT a multilevel member: 16 ILUCP and 16 ILU0 members of matgen.random_dd(4 000, 8, 25.0, seed), every
            repetition printed; runs unchanged on the parent commit's package (--package-root DIR) for the regression guard

A host clock around the call and a device synchronisation; 2 warm-up and `reps` timed repetitions of each, the two sides alternating;
median [min, max] in ms.
python profiles/tools/ml_apply_batch_times.py apply|solve|lone|guard [reps [iters]] [--package-root DIR]"""
import os, sys, time
import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
args = list(sys.argv[1:])
root = os.path.join(HERE, "..", "..")
if "--package-root" in args:
    k = args.index("--package-root")
    root = args[k + 1]
    del args[k:k + 2]
sys.path.insert(0, os.path.abspath(root))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))
import torch
import matgen
import ml_cases as C
import ilupp_amd as ilupp
import ilupp_amd.device as ild

mode = args[0] if args else "apply"
reps = int(args[1]) if len(args) > 1 else 7
iters = int(args[2]) if len(args) > 2 else 20
WARM = 2


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


def members(n, cnt):
    p = ilupp.iluplusplus_precond_parameter()
    p.default_configuration(1)
    p.threshold = 0.1
    p.PREPROCESSING = ilupp.preprocessing_sequence(("NORMALIZE_COLUMNS", "NORMALIZE_ROWS", "PQ_ORDERING"))
    mats = []
    for k in range(cnt):
        A = C.weak_random(n, 6.0 / n, 1.0, 900 + k)
        A.sort_indices()
        mats.append(A)
    t0 = time.perf_counter()
    B = ilupp.ILUppPreconditioner.batch(mats, params=p)
    lv = [P.pr.levels() for P in B]
    nz = [P.total_nnz for P in B]
    print("# n %d: %d members built in %.1f s; levels %d .. %d (median %d), stored entries %d .. %d" % (
        n, cnt, time.perf_counter() - t0, min(lv), max(lv), int(np.median(lv)), min(nz), max(nz)), flush=True)
    return mats, B, lv


def line(what, n, cnt, lv, tb, tl):
    print("%-6s n %5d members %2d (levels %d .. %d): batched %s  looped %s  batched / looped %.3f" % (
        what, n, cnt, min(lv), max(lv), stats(tb), stats(tl), np.median(tb) / np.median(tl)), flush=True)


print("times in ms, median [min, max] of %d after %d warm-up calls" % (reps, WARM))
if mode == "apply":
    for n in (4000, 1000):
        mats, B, lv = members(n, 64)
        ops = [ild.MultilevelOperator(P) for P in B]
        for cnt in (64, 16, 1):
            offsets = [k * n for k in range(cnt)]
            x = torch.ones(cnt * n, dtype=torch.float64, device="cuda")
            routes = ild.ml_apply_batch_(B[:cnt], x.clone(), offsets)
            x0 = x.clone()                  # (both sides start from the same values every time: one small copy in front of each)

            def looped_device():
                x.copy_(x0)
                for M, o in zip(ops[:cnt], offsets):
                    M.apply_(x[o:o + n])
            tb, tl = side_by_side(lambda: ild.ml_apply_batch_(B[:cnt], x.copy_(x0), offsets), looped_device)
            line("device", n, cnt, lv[:cnt], tb, tl)
            hx = [np.ones(n) for _ in range(cnt)]

            def looped_host():
                out = []
                for P, b in zip(B[:cnt], hx):
                    y = b.copy()
                    P.apply(y)
                    out.append(y)
                return out
            tb, tl = side_by_side(lambda: ilupp.ml_apply_batch(B[:cnt], hx), looped_host)
            line("host", n, cnt, lv[:cnt], tb, tl)
            print("#   routes of the %d: %s" % (cnt, sorted(set(routes))), flush=True)
        del B, ops
elif mode == "solve":
    kw = dict(maxiter=iters, rtol=0.0, check_every=0)
    print("# %d iterations per member" % iters)
    for n, counts in ((1000, (16, 64)),):
        mats, B, lv = members(n, max(counts))
        As = [ild.DeviceCSR.from_scipy(A) for A in mats]
        Ms = [ild.MultilevelOperator(P) for P in B]
        for cnt in counts:
            offsets = [k * n for k in range(cnt)]
            b = torch.ones(cnt * n, dtype=torch.float64, device="cuda")
            st = {}
            ild.bicgstab_batch(As[:cnt], b, offsets, Ms[:cnt], stats=st, **kw)
            tb, tl = side_by_side(lambda: ild.bicgstab_batch(As[:cnt], b, offsets, Ms[:cnt], **kw),
                                  lambda: [ild.bicgstab(a, b[o:o + n][:, None], m, **kw) for a, m, o in zip(As[:cnt], Ms[:cnt], offsets)])
            line("solve", n, cnt, lv[:cnt], tb, tl)
            print("#   routes of the %d: %s" % (cnt, sorted(set(st["route"]))), flush=True)
        del B, Ms
elif mode == "lone":
    for n in (4000, 8000):
        mats, B, lv = members(n, 2)
        ops = [ild.MultilevelOperator(P) for P in B]
        x = torch.ones(2 * n, dtype=torch.float64, device="cuda")
        r1 = ild.ml_apply_batch_(B[:1], x.clone(), [0])
        x0 = x.clone()
        tb, tl = side_by_side(lambda: ild.ml_apply_batch_(B[:1], x.copy_(x0), [0]), lambda: ops[0].apply_(x.copy_(x0)[:n]))
        line("lone", n, 1, lv[:1], tb, tl)
        print("#   route of the lone member: %s" % r1, flush=True)
        r2 = ild.ml_apply_batch_(B, x.clone(), [0, n])
        tb, tl = side_by_side(lambda: ild.ml_apply_batch_(B, x.copy_(x0), [0, n]),
                              lambda: (x.copy_(x0), [M.apply_(x[o:o + n]) for M, o in zip(ops, (0, n))]))
        line("pair", n, 2, lv, tb, tl)
        print("#   routes of the pair: %s (the pair's batched time is one workgroup's time for such a member)" % r2, flush=True)
        del B, ops
elif mode == "guard":
    kw = dict(maxiter=iters, rtol=0.0, check_every=0)
    n, cnt = 4000, 16
    mats = [sp.csr_matrix(matgen.random_dd(n, 8, 25.0, 500 + k), shape=(n, n)) for k in range(cnt)]
    As = [ild.DeviceCSR.from_scipy(A) for A in mats]
    offsets = [k * n for k in range(cnt)]
    b = torch.ones(cnt * n, dtype=torch.float64, device="cuda")
    for name, Ms in (("ILU0", [ild.DevicePreconditioner("ILU0", A) for A in As]), ("ILUCP", ilupp.ILUCPPreconditioner.batch(mats))):
        t = []
        for r in range(WARM + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); ild.bicgstab_batch(As, b, offsets, Ms, **kw); torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if r >= WARM:
                t.append(1e3 * dt)
        print("guard %-5s n %d members %d, %d iterations: %s  spread %.3f  runs %s" % (
            name, n, cnt, iters, stats(t), max(t) - min(t), " ".join("%.3f" % v for v in t)), flush=True)
else:
    raise SystemExit("unknown mode %s" % mode)
