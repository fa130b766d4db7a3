"""ilupp_amd.device.ilut_batch(As, fill_in, threshold) (the first construction of every ILUT member by one rows launch over all members,
one count launch, one read-back, one fill launch: k_ilut_rows_batch) next to the loop of DevicePreconditioner("ILUT", A, ...) over the same
matrices, for 1, 16 and 64 members of matgen.random_dd(n, 8, 25.0, seed) (nonsymmetric, about 8 entries per row) and the parameter sets
ILUT(10, 1e-4) and ILUT(100, 0.1).  A host clock around the call and a device synchronisation; the two ways INTERLEAVED repetition by
repetition (batched, looped, batched, ...), 2 warm-up rounds and `reps` timed ones, median [min, max] in ms; the objects of a repetition
are destroyed outside the timed region, the pool stays warm.  Per line also: the rows launches' event time (timings()["numeric_ms"] of a
launched member), the loop's own spread (max - min of its repetitions), and the full step -- ilut_batch + bicgstab_batch (20 iterations)
against the loop of constructor + bicgstab over the same systems.  For `order_at` (default 64 members of n = 4000): the round-robin
ticket order against the member-major one (ILUPP_ILUT_BATCH_ORDER=member, read per call), interleaved the same way.
python profiles/tools/ilut_batch_times.py [reps [n,n,... [members,members,... [order_members,order_n]]]]"""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import matgen
import ilupp_amd.device as ild

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1000, 4000]
counts = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 16, 64]
order_at = tuple(int(v) for v in sys.argv[4].split(",")) if len(sys.argv) > 4 else (64, 4000)
PARAMS = [(10, 1e-4), (100, 0.1)]
WARM = 2
ITERS = 20


def stats(v):
    return "%9.3f [%9.3f, %9.3f]" % (float(np.median(v)), min(v), max(v))


def interleaved(fs):
    """the functions of `fs` one after the other, round by round; each builds objects and returns them (dropped behind the clock)"""
    out = [[] for _ in fs]
    last = [None] * len(fs)
    for r in range(WARM + reps):
        for k, f in enumerate(fs):
            last[k] = None
            torch.cuda.synchronize()
            t0 = time.perf_counter(); last[k] = f(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if r >= WARM:
                out[k].append(1e3 * dt)
    return out, last


print("times in ms, median [min, max] of %d interleaved repetitions after %d warm-up rounds" % (reps, WARM))
for n in sizes:
    As = []
    for k in range(max(counts + [order_at[0] if order_at[1] == n else 0])):
        d, i, p = matgen.random_dd(n, 8, 25.0, 500 + k)
        As.append(ild.DeviceCSR(torch.from_numpy(np.asarray(d, dtype=np.float64)).cuda(), torch.from_numpy(np.asarray(i, dtype=np.int32)).cuda(),
                                torch.from_numpy(np.asarray(p, dtype=np.int32)).cuda()))
    for fill, tau in PARAMS:
        for cnt in counts:
            mats = As[:cnt]
            offsets = [k * n for k in range(cnt)]
            b = torch.from_numpy(np.random.default_rng(1).standard_normal(n * cnt) + 2.0).cuda()
            ild._on_current_stream()
            rows_ms = []

            def looped():
                return [ild.DevicePreconditioner("ILUT", A, fill_in=fill, threshold=tau) for A in mats]

            def batched():
                Ms = ild.ilut_batch(mats, fill_in=fill, threshold=tau)
                rows_ms.append(Ms[0].pr.timings()["numeric_ms"])
                return Ms

            def step_looped():
                Ms = looped()
                xs = [ild.bicgstab(A, b[o:o + n, None], M, maxiter=ITERS) for A, M, o in zip(mats, Ms, offsets)]
                return Ms, xs

            def step_batched():
                Ms = ild.ilut_batch(mats, fill_in=fill, threshold=tau)
                return Ms, ild.bicgstab_batch(mats, b, offsets, Ms, maxiter=ITERS)

            (t_batch, t_loop), built = interleaved([batched, looped])
            paths = sorted(set(M.pr.path() for M in built[0]))
            del built
            (s_batch, s_loop), built = interleaved([step_batched, step_looped])
            del built
            tag = "ILUT(%d, %g) n %5d members %2d" % (fill, tau, n, cnt)
            print("%s: batched %s  looped %s  batched / looped %.3f  loop's spread %.3f  paths %s"
                  % (tag, stats(t_batch), stats(t_loop), np.median(t_batch) / np.median(t_loop), max(t_loop) - min(t_loop), paths), flush=True)
            print("%s  rows launches %.3f  looped per member %.3f  step (construct + %d BiCGstab iterations): batched %s  looped %s  ratio %.3f"
                  % (" " * len(tag), float(np.median(rows_ms[WARM:])) if paths == ["ilut:batch"] else float("nan"), np.median(t_loop) / cnt, ITERS,
                     stats(s_batch), stats(s_loop), np.median(s_batch) / np.median(s_loop)), flush=True)
            if (cnt, n) == order_at or (cnt == max(counts) and n == order_at[1] and order_at[0] > cnt):
                mm = As[:order_at[0]]
                rows = {"round-robin": [], "member-major": []}

                def ordered(name):
                    def f():
                        if name == "member-major":
                            os.environ["ILUPP_ILUT_BATCH_ORDER"] = "member"
                        try:
                            Ms = ild.ilut_batch(mm, fill_in=fill, threshold=tau)
                        finally:
                            os.environ.pop("ILUPP_ILUT_BATCH_ORDER", None)
                        rows[name].append(Ms[0].pr.timings()["numeric_ms"])
                        return Ms
                    return f

                (t_rr, t_mm), built = interleaved([ordered("round-robin"), ordered("member-major")])
                del built
                print("%s  ticket order, %d members: round-robin call %s rows launch %s | member-major call %s rows launch %s"
                      % (" " * len(tag), len(mm), stats(t_rr), stats(rows["round-robin"][WARM:]), stats(t_mm), stats(rows["member-major"][WARM:])), flush=True)
