"""Block apply (k right-hand sides in one call) against k single applies, on device tensors, on the bench's matrices:
    python profiles/tools/block_apply_times.py [--configs C3,S9,ILUC,C4,C2] [--ks 1,4,8,16,32] [--reps 20] [--warmup 3]

Per configuration and k, every form timed with device events on torch's current stream (warmed up, then --reps repetitions; the inputs are
restored outside the timed region before each one):
  single   one apply_ of one contiguous vector
  bare     k apply_ calls on k contiguous vectors (no copies: the lower bound of any column loop)
  loop     the column loop a caller of a 2-D tensor writes: c = X[:, j].contiguous(); apply_(c); X[:, j] = c
  block    one apply_ of the (n, k) tensor (ilupp_hip_apply_block_device), with its route
Median, minimum and maximum over the repetitions.  In the same run the block result is compared bitwise with the k single applies."""
import argparse
import json
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

CONFIGS = {
    "C3": ("ILUT(10, 1e-4), random_dd n = 10^6", lambda: matgen.random_dd(1000000, 19, 25.0, 12345), "ILUT", {"fill_in": 10, "threshold": 1e-4}),
    "S9": ("ILU(0), 9-point 2048^2", lambda: matgen.box_stencil((2048, 2048)), "ILU0", {}),
    "ILUC": ("ILUC(8, 1e-2), 7-point 128^3", lambda: matgen.poisson3d(128), "ILUC", {"fill_in": 8, "threshold": 1e-2}),
    "C4": ("ICholT(0, 0), 7-point 256^3", lambda: matgen.poisson3d(256), "ICholT", {"add_fill_in": 0, "threshold": 0.0}),
    "C2": ("ILU(0), 7-point 256^3", lambda: matgen.poisson3d(256), "ILU0", {}),
}


def timed(fn, prep, reps, warmup):
    """device-event times (ms) of fn() over reps repetitions after warmup ones; prep() runs untimed before each"""
    out = []
    for r in range(warmup + reps):
        prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        if r >= warmup:
            out.append((a, b))
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in out])
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max())}


def run(name, ks, reps, warmup):
    what, make, kind, params = CONFIGS[name]
    d, i, p = make()
    n = p.shape[0] - 1
    dA = ild.DeviceCSR.from_scipy(sp.csr_matrix((d, i, p), shape=(n, n)))
    M = ild.DevicePreconditioner(kind, dA, **params)
    kmax = max(ks)
    g = torch.Generator(device="cuda").manual_seed(7)
    X0 = torch.randn((n, kmax), dtype=torch.float64, device="cuda", generator=g)
    res = {"config": name, "what": what, "n": n, "reps": reps, "k": {}}
    v0 = X0[:, 0].contiguous()
    v = torch.empty_like(v0)
    res["single_ms"] = timed(lambda: M.apply_(v), lambda: v.copy_(v0), reps, warmup)
    print("%-5s %s, n = %d: one single apply %.3f ms (min %.3f, max %.3f)" % (name, what, n, res["single_ms"]["median"],
          res["single_ms"]["min"], res["single_ms"]["max"]), flush=True)
    for k in ks:
        Xk0 = X0[:, :k].contiguous()
        Xb = torch.empty_like(Xk0)
        cols0 = [Xk0[:, j].contiguous() for j in range(k)]
        cols = [torch.empty_like(c) for c in cols0]
        Xl = torch.empty_like(Xk0)

        def bare():
            for c in cols:
                M.apply_(c)

        def bare_prep():
            for c, c0 in zip(cols, cols0):
                c.copy_(c0)

        def loop():
            for j in range(k):
                c = Xl[:, j].contiguous()
                M.apply_(c)
                Xl[:, j] = c

        t_block = timed(lambda: M.apply_(Xb), lambda: Xb.copy_(Xk0), reps, warmup)
        route = M.pr.block_path()
        t_bare = timed(bare, bare_prep, reps, warmup)
        t_loop = timed(loop, lambda: Xl.copy_(Xk0), reps, warmup)
        # bitwise: the block against the k single applies, once more from the pristine inputs
        Xb.copy_(Xk0); bare_prep()
        M.apply_(Xb); bare()
        M.sync()
        same = bool(torch.equal(Xb.view(torch.int64), torch.stack(cols, dim=1).view(torch.int64)))
        r = {"route": route, "block_ms": t_block, "bare_ms": t_bare, "loop_ms": t_loop, "bitwise_equal": same,
             "block_over_single": t_block["median"] / res["single_ms"]["median"],
             "block_over_bare": t_block["median"] / t_bare["median"], "block_over_loop": t_block["median"] / t_loop["median"]}
        res["k"][k] = r
        print("%-5s k=%-3d %-13s block %8.3f ms [%.3f, %.3f]  bare %8.3f [%.3f, %.3f]  loop %8.3f [%.3f, %.3f]  "
              "block/single %.2f  block/bare %.3f  block/loop %.3f  bitwise %s" % (
                  name, k, route, t_block["median"], t_block["min"], t_block["max"], t_bare["median"], t_bare["min"], t_bare["max"],
                  t_loop["median"], t_loop["min"], t_loop["max"], r["block_over_single"], r["block_over_bare"], r["block_over_loop"],
                  "yes" if same else "NO"), flush=True)
        del Xb, cols, cols0, Xl, Xk0
    del M, dA, X0
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,S9,ILUC,C4,C2")
    ap.add_argument("--ks", default="1,4,8,16,32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    ok = True
    for name in a.configs.split(","):
        r = run(name, ks, a.reps, a.warmup)
        ok = ok and all(v["bitwise_equal"] for v in r["k"].values())
        print(json.dumps(r), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
