"""ilupp_amd.device.DevicePreconditioner.batch("ILU0", As) (the first construction of every member by two launches of one workgroup per
member around one read-back: k_ilu0_symbolic_batch, k_ilu0_create_batch) next to the loop of DevicePreconditioner("ILU0", A) over the same
matrices, for 1, 16 and 64 members of matgen.random_dd(n, 8, 25.0, seed); a host clock around the call and a device synchronisation; 2
warm-up and `reps` timed repetitions, median [min, max] in ms.  The objects of a repetition are destroyed outside the timed region.
Per line also: the two launches' event times (timings() of a launched member: analysis_ms = symbolic, numeric_ms = create), the host
share per member -- (the call's wall time - the two launches) / members: objects, streams and events, pool blocks, descriptor uploads,
the read-back and the final wait --, and the first apply_batch_ behind a batched and behind a looped construction (one call each, on fresh
objects: the looped ones bring the transposed-free CSR triangles of their construction, a static-form one unpacks its records first).
On a checkout without the batched construction only the loop is timed (the loop of the commit before, for comparison).
python profiles/tools/ilu0_create_batch_times.py [reps [n,n,... [members,members,...]]]"""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import matgen
import ilupp_amd.device as ild

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1000, 4000]
counts = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 16, 64]
WARM = 2
HAVE_BATCH = hasattr(ild.DevicePreconditioner, "batch")


def stats(v):
    return "%9.3f [%9.3f, %9.3f]" % (float(np.median(v)), min(v), max(v))


def timed(f):
    """f builds objects and returns them: they are dropped behind the clock"""
    out, last = [], None
    for r in range(WARM + reps):
        last = None
        torch.cuda.synchronize()
        t0 = time.perf_counter(); last = f(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if r >= WARM:
            out.append(1e3 * dt)
    return out, last


def first_apply(members, n):
    offsets = [k * n for k in range(len(members))]
    x = torch.ones(n * len(members), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter(); ild.apply_batch_(members, x, offsets); torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


print("times in ms, median [min, max] of %d after %d warm-up calls%s" % (reps, WARM, "" if HAVE_BATCH else "  (no batched construction here: the loop only)"))
for n in sizes:
    As = []
    for k in range(max(counts)):
        d, i, p = matgen.random_dd(n, 8, 25.0, 500 + k)
        As.append(ild.DeviceCSR(torch.from_numpy(np.asarray(d, dtype=np.float64)).cuda(), torch.from_numpy(np.asarray(i, dtype=np.int32)).cuda(),
                                torch.from_numpy(np.asarray(p, dtype=np.int32)).cuda()))
    for cnt in counts:
        mats = As[:cnt]
        ild._on_current_stream()

        def looped():
            return [ild.DevicePreconditioner("ILU0", A) for A in mats]

        def batched():
            return ild.DevicePreconditioner.batch("ILU0", mats)

        t_loop, built = timed(looped)
        a_loop = first_apply(built, n)
        paths = sorted(set(M.pr.path() for M in built))
        del built
        if not HAVE_BATCH:
            print("ILU0   n %5d members %2d: looped %s  per member %.3f  first apply_batch_ %.3f  paths %s"
                  % (n, cnt, stats(t_loop), np.median(t_loop) / cnt, a_loop, paths), flush=True)
            continue
        t_batch, built = timed(batched)
        tm = built[0].pr.timings()
        bpaths = sorted(set(M.pr.path() for M in built))
        a_batch = first_apply(built, n)
        del built
        launches = tm["analysis_ms"] + tm["numeric_ms"] if bpaths == ["ilu0:batch"] else float("nan")
        print("ILU0   n %5d members %2d: batched %s  looped %s  batched / looped %.3f  paths %s (looped: %s)"
              % (n, cnt, stats(t_batch), stats(t_loop), np.median(t_batch) / np.median(t_loop), bpaths, paths), flush=True)
        print("       symbolic launch %.3f  create launch %.3f  host share per member %.4f  looped per member %.3f  first apply_batch_: batched %.3f looped %.3f"
              % (tm["analysis_ms"] if launches == launches else float("nan"), tm["numeric_ms"] if launches == launches else float("nan"),
                 (np.median(t_batch) - launches) / cnt, np.median(t_loop) / cnt, a_batch, a_loop), flush=True)
