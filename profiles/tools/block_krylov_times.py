"""k right-hand sides in the device Krylov layer: the CSR SpMM against k SpMVs, and one k-column CG / BiCGstab iteration against one
single-column iteration:
    python profiles/tools/block_krylov_times.py [--ks 1,2,4,8,16,32] [--reps 20] [--warmup 3] [--parts spmm,cg,bicgstab]

Every form is timed with device events on torch's current stream (warmed up, then --reps repetitions); median [min, max] in ms.
  spmm     DeviceCSR.matmat of an (n, k) block (ilupp_hip_spmm_device) against k matvec calls on k contiguous vectors, on 7-point 256^3,
           27-point 128^3 and C3's random_dd n = 10^6; modelled bytes (A once, X and Y once: nnz * 12 + (n + 1) * 4 + 2 n k * 8; k SpMVs
           read A k times) and the GB/s they give at the measured time.  The SpMM result is compared bitwise with the SpMVs.
  cg       one iteration of device.cg with k = 8 against k = 1 (a (n, 1) block) and the 1-D path: (t(m + 10) - t(m)) / 10 of whole
           calls with maxiter m = 2 and rtol = 0, on 7-point 128^3 with ICholT(5, 1e-3) and with IChol0; the block apply's route.
  bicgstab the same for device.bicgstab on C3 with ILUT(10, 1e-4)."""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matgen  # noqa: E402
import ilupp_amd.device as ild  # noqa: E402

MATS = {
    "P7_256": ("7-point 256^3", lambda: matgen.poisson3d(256)),
    "B27_128": ("27-point 128^3", lambda: matgen.box_stencil((128, 128, 128))),
    "C3": ("random_dd n = 10^6", lambda: matgen.random_dd(1000000, 19, 25.0, 12345)),
}


def timed(fn, reps, warmup):
    out = []
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        if r >= warmup:
            out.append((a, b))
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in out])
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def fmt(t):
    return "%8.3f ms [%.3f, %.3f]" % t


def device_csr(make):
    t = make()
    if isinstance(t, tuple):
        d, i, p = t
        n = p.shape[0] - 1
        t = sp.csr_matrix((d, i, p), shape=(n, n))
    return ild.DeviceCSR.from_scipy(t)


def spmm_part(ks, reps, warmup):
    print("== SpMM (DeviceCSR.matmat) against k SpMVs ==")
    for name, (what, make) in MATS.items():
        dA = device_csr(make)
        n, nnz = dA.n, dA.nnz
        a_bytes = nnz * 12 + (n + 1) * 4
        print("%-8s %s, n = %d, nnz = %d, A = %.3f GB" % (name, what, n, nnz, a_bytes / 1e9))
        g = torch.Generator(device="cuda").manual_seed(3)
        for k in ks:
            X = torch.randn((n, k), dtype=torch.float64, device="cuda", generator=g)
            Y = torch.empty_like(X)
            cols = [X[:, j].contiguous() for j in range(k)]
            outs = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(k)]
            t_mm = timed(lambda: dA.matmat(X, out=Y), reps, warmup)

            def spmvs():
                for j in range(k):
                    dA.matvec(cols[j], out=outs[j])
            t_mv = timed(spmvs, reps, warmup)
            same = torch.equal(Y.view(torch.int64), torch.stack(outs, dim=1).view(torch.int64))
            b_mm = a_bytes + 2 * n * k * 8
            b_mv = k * (a_bytes + 2 * n * 8)
            print("%-8s k=%-3d spmm %s  %6.2f GB model %7.0f GB/s | %d spmv %s  %6.2f GB model %7.0f GB/s | ratio %.3f  model %.3f  bitwise %s"
                  % (name, k, fmt(t_mm), b_mm / 1e9, b_mm / t_mm[0] / 1e6, k, fmt(t_mv), b_mv / 1e9, b_mv / t_mv[0] / 1e6,
                     t_mm[0] / t_mv[0], b_mm / b_mv, "yes" if same else "NO"))
            del X, Y, cols, outs
        del dA
        torch.cuda.empty_cache()


def iteration_time(solve, dA, M, B, reps, warmup, m=2):
    """per repetition: (t(maxiter = m + 10) - t(maxiter = m)) / 10, the two calls timed back to back; median [min, max] of those"""
    ev = []
    for r in range(warmup + reps):
        t = []
        for it in (m, m + 10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            solve(dA, B, M, maxiter=it)
            b.record()
            t.append((a, b))
        if r >= warmup:
            ev.append(t)
    torch.cuda.synchronize()
    d = np.array([(t[1][0].elapsed_time(t[1][1]) - t[0][0].elapsed_time(t[0][1])) / 10 for t in ev])
    return float(np.median(d)), float(d.min()), float(d.max())


def solver_part(label, solve, make, kind, params, reps, warmup):
    dA = device_csr(make)
    M = ild.DevicePreconditioner(kind, dA, **params)
    n = dA.n
    g = torch.Generator(device="cuda").manual_seed(5)
    B8 = torch.randn((n, 8), dtype=torch.float64, device="cuda", generator=g)
    B1 = B8[:, :1].contiguous()
    b = B8[:, 0].contiguous()
    t1d = iteration_time(solve, dA, M, b, reps, warmup)
    t1 = iteration_time(solve, dA, M, B1, reps, warmup)
    M.apply_(B8.clone())
    M.sync()
    route = M.pr.block_path()
    t8 = iteration_time(solve, dA, M, B8, reps, warmup)
    print("%-34s n = %d  route %-13s 1-D %s | k=1 %s | k=8 %s | k=8 / k=1 %.2f  per column %.3f"
          % (label, n, route, fmt(t1d), fmt(t1), fmt(t8), t8[0] / t1[0], t8[0] / t1[0] / 8))
    M.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="spmm,cg,bicgstab")
    a = ap.parse_args()
    parts = a.parts.split(",")
    print("device: %s" % torch.cuda.get_device_name(0))
    if "spmm" in parts:
        spmm_part([int(k) for k in a.ks.split(",")], a.reps, a.warmup)
    if "cg" in parts:
        print("== one CG iteration (median [min, max] over the repetitions of (t(12 iterations) - t(2)) / 10) ==")
        solver_part("CG ICholT(5, 1e-3) 7-point 128^3", ild.cg, lambda: matgen.poisson3d(128), "ICholT",
                    {"add_fill_in": 5, "threshold": 1e-3}, a.reps, a.warmup)
        solver_part("CG IChol0 7-point 128^3", ild.cg, lambda: matgen.poisson3d(128), "IChol0", {}, a.reps, a.warmup)
    if "bicgstab" in parts:
        print("== one BiCGstab iteration ==")
        solver_part("BiCGstab ILUT(10, 1e-4) C3", ild.bicgstab, MATS["C3"][1], "ILUT", {"fill_in": 10, "threshold": 1e-4}, a.reps, a.warmup)


if __name__ == "__main__":
    main()
