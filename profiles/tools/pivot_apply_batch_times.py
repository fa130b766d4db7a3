"""ILUCPPreconditioner / ILUTPPreconditioner: the batched apply next to the loop of single applies, for 1, 16 and 64 members of n = 12000
and n = 1000 on matgen.random_dd(n, 8, 25.0, seed), both directions; 3 warm-up and `reps` timed repetitions of each, median [min, max]:

  device  device events around ilupp_amd.device.pivot_apply_batch_ on one packed tensor, against the loop of
          PivotedPreconditioner.apply_device(sync=False) over the same vectors on the same stream
  host    a host clock around ilupp_amd.apply_batch (one packed upload, the launch, one download, waited for), against the loop of
          P.apply(x) on copies of the same vectors

the two alternate repetition by repetition.  python profiles/tools/pivot_apply_batch_times.py [reps [n,n,... [members,members,...]]]"""
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [12000, 1000]
counts = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 16, 64]
WARM = 3


def stats(v):
    return "%8.3f [%8.3f, %8.3f]" % (float(np.median(v)), min(v), max(v))


def device_times(B, n, transpose):
    """ms per call: (batched, looped), device events on torch's current stream"""
    cnt = len(B)
    x = torch.ones(cnt * n, dtype=torch.float64, device="cuda")
    offsets = [k * n for k in range(cnt)]
    st = torch.cuda.current_stream()
    _native.set_caller_stream(st.cuda_stream, True)

    def batched():
        ild.pivot_apply_batch_(B, x, offsets, transpose=transpose)

    def looped():
        for k, P in enumerate(B):
            P.pr.apply_device(x.data_ptr() + 8 * offsets[k], n, transpose=transpose, sync=False)

    out = {batched: [], looped: []}
    for r in range(WARM + reps):
        for f in (batched, looped):
            x.fill_(1.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st); f(); b.record(st)
            b.synchronize()
            if r >= WARM:
                out[f].append(a.elapsed_time(b))
    return out[batched], out[looped]


def host_times(B, n, transpose):
    """ms per call: (batched, looped), host clock around calls that wait for their result"""
    rhs = [np.ones(n) for _ in B]

    def batched():
        ilupp.apply_batch(B, rhs, transpose=transpose)

    def looped():
        for P, b in zip(B, rhs):
            x = b.copy()
            (P.apply_trans if transpose else P.apply)(x)

    out = {batched: [], looped: []}
    for r in range(WARM + reps):
        for f in (batched, looped):
            t0 = time.perf_counter(); f(); dt = time.perf_counter() - t0
            if r >= WARM:
                out[f].append(1e3 * dt)
    return out[batched], out[looped]


print("cap: n <= %d takes the launch; times in ms, median [min, max] of %d after %d warm-up calls" % (_native.pivot_apply_batch_max_n(), reps, WARM))
for n in sizes:
    mats = [sp.csr_matrix(matgen.random_dd(n, 8, 25.0, 500 + k), shape=(n, n)) for k in range(max(counts))]
    for cls in (ilupp.ILUCPPreconditioner, ilupp.ILUTPPreconditioner):
        members = cls.batch(mats)
        for cnt in counts:
            B = members[:cnt]
            for transpose in (False, True):
                for what, f in (("device", device_times), ("host  ", host_times)):
                    tb, tl = f(B, n, transpose)
                    print("%s n %5d members %2d %s %s: batched %s  looped %s  batched / looped %.3f"
                          % (cls.__name__[:5], n, cnt, "apply_trans" if transpose else "apply      ", what, stats(tb), stats(tl),
                             np.median(tb) / np.median(tl)), flush=True)
        del members, B
