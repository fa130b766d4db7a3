"""ilupp_amd.device.refactor_batch_ (the numeric ILU(0) re-factorisation of every member in ONE launch, k_ilu0_refactor_batch) with
check=False next to the loop of single re-factorisations P.pr.refactor_device over the same objects, for 1, 16 and 64 members of
matgen.random_dd(n, 8, 25.0, seed), new values in the analysed pattern; a host clock around the call and a device synchronisation; 2
warm-up and `reps` timed repetitions, median [min, max] in ms.  The loop is timed first, on the objects as their construction left them
(their packed sweeps are re-packed by every single re-factorisation, as in a program that only has the loop); the batched calls follow
(the first warm-up call drops those packed copies, the timed calls wait for nothing).  A member alone takes the single path inside
the batched call (route 1); the extra line is the launch of that one member with the rule switched off (ILUPP_REFACTOR_ALONE_MIN).
python profiles/tools/refactor_batch_times.py [reps [n,n,... [members,members,...]]]"""
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


def stats(v):
    return "%9.3f [%9.3f, %9.3f]" % (float(np.median(v)), min(v), max(v))


def timed(f):
    out = []
    for r in range(WARM + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); f(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if r >= WARM:
            out.append(1e3 * dt)
    return out


print("times in ms, median [min, max] of %d after %d warm-up calls" % (reps, WARM))
for n in sizes:
    As, A2 = [], []
    for k in range(max(counts)):
        d, i, p = matgen.random_dd(n, 8, 25.0, 500 + k)
        d = np.asarray(d, dtype=np.float64)
        ti, tp = torch.from_numpy(np.asarray(i, dtype=np.int32)).cuda(), torch.from_numpy(np.asarray(p, dtype=np.int32)).cuda()
        As.append(ild.DeviceCSR(torch.from_numpy(d).cuda(), ti, tp))
        A2.append(ild.DeviceCSR(torch.from_numpy(d * (1.0 + 0.1 * np.random.default_rng(k).random(d.shape[0]))).cuda(), ti, tp))
    for cnt in counts:
        members = [ild.DevicePreconditioner("ILU0", A) for A in As[:cnt]]
        new = A2[:cnt]
        ild._on_current_stream()

        def looped():
            for M, A in zip(members, new):
                M.pr.refactor_device(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr())

        def batched():
            return ild.refactor_batch_(members, new, check=False)

        t_loop = timed(looped)
        t_batch = timed(batched)
        routes = batched()[0]
        print("ILU0   n %5d members %2d: batched %s  looped %s  batched / looped %.3f  routes %s"
              % (n, cnt, stats(t_batch), stats(t_loop), np.median(t_batch) / np.median(t_loop), sorted(set(routes))), flush=True)
        if cnt == 1 and routes == [1]:
            # the member alone takes the single path (the rule in api.hip); what the launch of that one member costs, the rule switched off
            os.environ["ILUPP_REFACTOR_ALONE_MIN"] = str(n + 1)
            t_alone = timed(batched)
            routes = batched()[0]
            del os.environ["ILUPP_REFACTOR_ALONE_MIN"]
            print("       n %5d alone in the launch:  %s  / looped %.3f  routes %s"
                  % (n, stats(t_alone), np.median(t_alone) / np.median(t_loop), routes), flush=True)
        del members
