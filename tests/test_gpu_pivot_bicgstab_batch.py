"""GPU tests of the batched BiCGstab solve of the two pivoting classes (ilupp_amd.device.bicgstab_batch over
ilupp_hip_bicgstab_batch_device: one launch of k_bicgstab_batch, one workgroup per system with the whole preconditioned loop inside it;
the C entry of these classes alone, ilupp_hip_pivot_bicgstab_batch_device, runs the same kernel and is called directly in the last
test).  Every member has the bits of ilupp_amd.device.bicgstab(A_k, b_k[:, None], PivotedOperator(P_k), ...) -- the loop of SpMM,
single device apply, block dots and block updates -- run one member at a time: the solution on its int64 view, the iteration count, the
converged flag and the relative residual.  Across the dot's and the sweeps' shapes, with convergence per member, with x0, next to a zero
and a NaN member, with more members than CUs, across the LDS cap, between a producer and a consumer on a side stream; and sixteen
systems side by side take less time than the loop over them."""
import os
import time

import numpy as np
import pytest
import scipy.sparse as sp

import matgen
import ml_cases as C

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["laplace2d", "random", "rdd_300", "weak_200", "offdiag_150"]          # the matrices of tests/golden/ilucp.npz / ilutp.npz


def _random(n, seed, fmt, diag=3.0):
    rng = np.random.default_rng(seed)
    A = (sp.random(n, n, min(1.0, 6.0 / n), random_state=rng, data_rvs=lambda k: rng.standard_normal(k)) + sp.eye(n) * diag).asformat(fmt)
    A.sort_indices()
    return A


def _dd(n, seed, fmt="csr"):
    return sp.csr_matrix(matgen.random_dd(n, 8, 25.0, seed), shape=(n, n)).asformat(fmt)


def _band(n, seed):
    """rows of 2 - 3 entries: a random tridiagonal matrix with a heavy diagonal (its construction is a short chain per row)"""
    rng = np.random.default_rng(seed)
    A = sp.diags([rng.standard_normal(n - 1), 4.0 + rng.random(n), rng.standard_normal(n - 1)], [-1, 0, 1], format="csr")
    A.sort_indices()
    return A


def _golden_matrices():
    gold = np.load(os.path.join(HERE, "golden", "ilucp.npz"))
    mats = []
    for name in NAMES:
        key = "%s_csr" % name
        n = gold[key + "/indptr"].shape[0] - 1
        mats.append(sp.csr_matrix((gold[key + "/data"].copy(), gold[key + "/indices"].copy(), gold[key + "/indptr"].copy()), shape=(n, n)))
    return mats


def _mixed(mats, **params):
    """ILUCP and ILUTP objects in turn"""
    import ilupp_amd as ilupp
    return [(ilupp.ILUCPPreconditioner if k % 2 == 0 else ilupp.ILUTPPreconditioner)(A, **params) for k, A in enumerate(mats)]


def _pack(vectors, gap=3, fill=0.0):
    """the vectors in one array with `gap` elements in front of, between and behind them: (array, offsets)"""
    offsets, total = [], gap
    for v in vectors:
        offsets.append(total)
        total += v.shape[0] + gap
    host = np.full(total, fill, dtype=np.float64)
    for o, v in zip(offsets, vectors):
        host[o:o + v.shape[0]] = v
    return host, offsets


def _device(mats):
    import ilupp_amd.device as ild
    return [ild.DeviceCSR.from_scipy(A) for A in mats]


def _loop(As, Ps, b, offsets, x0=None, **kw):
    """the reference: one member at a time through device.bicgstab with the thin adapter; per member (x, iterations, converged, relres)"""
    import ilupp_amd.device as ild
    out = []
    for A, P, o in zip(As, Ps, offsets):
        st = {}
        x = ild.bicgstab(A, b[o:o + A.n][:, None], ild.PivotedOperator(P), x0=None if x0 is None else x0[o:o + A.n][:, None], stats=st, **kw)
        out.append((x[:, 0].cpu().numpy(), int(st["iterations"][0]), bool(st["converged"][0]), st["relres"].numpy().copy()))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _batch_equals(As, Ps, b, offsets, ref, x0=None, nan_members=(), tag="", **kw):
    """bicgstab_batch against `ref` (what _loop gave): the solutions on their int64 views (equal_nan for the members of nan_members, whose
    NaNs need not share a payload), iterations, converged and the bits of relres.  Returns (x on the host, stats)."""
    import ilupp_amd.device as ild
    st = {}
    x = ild.bicgstab_batch(As, b, offsets, Ps, x0=x0, stats=st, **kw)
    assert x.shape == b.shape and x.data_ptr() != b.data_ptr()
    xh = x.cpu().numpy()
    assert len(st["route"]) == len(As) and st["iterations"].dtype.is_floating_point is False and st["iterations"].shape == (len(As),)
    for k, (A, o, (xr, it, conv, rel)) in enumerate(zip(As, offsets, ref)):
        got = xh[o:o + A.n]
        if k in nan_members:
            assert np.array_equal(got, xr, equal_nan=True), (tag, k, "x")
            assert np.array_equal(st["relres"][k:k + 1].numpy(), rel, equal_nan=True), (tag, k, "relres")
        else:
            assert np.array_equal(_bits(got), _bits(xr)), (tag, k, "x", float(np.max(np.abs(got - xr))))
            assert np.array_equal(_bits(st["relres"][k:k + 1].numpy()), _bits(rel)), (tag, k, "relres", float(st["relres"][k]), rel)
        assert int(st["iterations"][k]) == it, (tag, k, "iterations", int(st["iterations"][k]), it)
        assert bool(st["converged"][k]) == conv, (tag, k, "converged")
    return xh, st


# ---- 1. the shapes where the dot and the sweeps can go wrong ----
def test_every_shape_equals_the_loop():
    """n = 1, 2, 65 (one past a wave), 256 (exactly one chunk of the dot), 257 (one past the workgroup: 2 chunks of 129), 300 (2 chunks
    of 150), 513 (3 chunks of 171) and the five golden matrices (n = 150 - 400), ILUCP and ILUTP in turn, in one batch"""
    import torch
    mats = [_random(n, 70 + k, "csr") for k, n in enumerate([1, 2, 65, 256, 257, 300, 513])] + _golden_matrices()
    Ps = _mixed(mats)
    host, offsets = _pack([C.rhs(A.shape[0]) for A in mats])
    b = torch.from_numpy(host).cuda()
    As = _device(mats)
    ref = _loop(As, Ps, b, offsets, maxiter=8, check_every=0)
    xh, st = _batch_equals(As, Ps, b, offsets, ref, maxiter=8, check_every=0, tag="shapes")
    assert st["route"] == [0] * len(mats)
    assert any(it == 8 for _, it, _, _ in ref) and all(np.all(np.isfinite(x)) for x, _, _, _ in ref)       # (the loop ran, on numbers)
    mask = np.ones(host.shape[0], dtype=bool)
    for o, A in zip(offsets, mats):
        mask[o:o + A.shape[0]] = False
    assert np.all(_bits(xh[mask]) == 0)                                                               # (the gaps: zeros, untouched)


# ---- 2. convergence per member ----
DD_MEMBERS = [(100, 11), (150, 12), (233, 13), (256, 14), (300, 15), (411, 16), (513, 17), (600, 18)]      # (n, seed)
# preconditioners of different strength, chosen on the reference loop alone (one MI355X): it converges in 4, 3, 5, 2, 4, 3, 5, 4 iterations
# with check_every = 1 and in 6, 3, 6, 3, 6, 3, 6, 6 with check_every = 3
DD_PARAMS = [dict(fill_in=100, threshold=0.1), dict(fill_in=100, threshold=0.01), dict(fill_in=1, threshold=1.0), dict(fill_in=100, threshold=0.001),
             dict(fill_in=100, threshold=0.1), dict(fill_in=100, threshold=0.01), dict(fill_in=2, threshold=0.5), dict(fill_in=100, threshold=0.1)]


@pytest.fixture(scope="module")
def dd_members():
    import torch
    import ilupp_amd as ilupp
    mats = [_dd(n, seed) for n, seed in DD_MEMBERS]
    Ps = [(ilupp.ILUCPPreconditioner if k % 2 == 0 else ilupp.ILUTPPreconditioner)(A, **DD_PARAMS[k]) for k, A in enumerate(mats)]
    host, offsets = _pack([C.rhs(A.shape[0]) * (1.0 + k / 8.0) for k, A in enumerate(mats)])
    return _device(mats), Ps, torch.from_numpy(host).cuda(), offsets


@pytest.mark.parametrize("check_every", [1, 3])
def test_members_converge_each_at_its_own_iteration(dd_members, check_every):
    """eight diagonally dominant members of n = 100 - 600 with preconditioners of different strength, rtol = 1e-10: on the reference loop
    alone every member converges in fewer than 60 iterations and not all at the same one; the batch stops every member where the loop does"""
    As, Ps, b, offsets = dd_members
    kw = dict(maxiter=60, rtol=1e-10, check_every=check_every)
    ref = _loop(As, Ps, b, offsets, **kw)
    its = [it for _, it, _, _ in ref]
    print("check_every %d: iterations of the reference loop %s" % (check_every, its))
    assert all(conv for _, _, conv, _ in ref) and all(0 < it < 60 for it in its), its
    assert len(set(its)) >= 2, its
    assert all(float(rel[0]) <= 1e-10 for _, _, _, rel in ref)
    _, st = _batch_equals(As, Ps, b, offsets, ref, tag=("converge", check_every), **kw)
    assert st["route"] == [0] * len(As)


# ---- 3. x0 given ----
def test_a_start_vector_is_used_as_the_loop_uses_it(dd_members):
    import torch
    As, Ps, b, offsets = dd_members
    rng = np.random.default_rng(5)
    x0 = torch.from_numpy(rng.standard_normal(b.numel())).cuda()
    for kw in (dict(maxiter=4, check_every=0), dict(maxiter=60, rtol=1e-10, check_every=2)):
        ref = _loop(As, Ps, b, offsets, x0=x0, **kw)
        xh, _ = _batch_equals(As, Ps, b, offsets, ref, x0=x0, tag=("x0", kw["maxiter"]), **kw)
        mask = np.ones(b.numel(), dtype=bool)
        for o, A in zip(offsets, As):
            mask[o:o + A.n] = False
        assert np.array_equal(_bits(xh[mask]), _bits(x0.cpu().numpy()[mask]))                         # (the gaps keep x0's bits)


# ---- 4. isolation and breakdown ----
def test_a_zero_and_a_nan_member_leave_the_others_alone():
    """member 0: an all-zero right-hand side -- converged at once, 0 iterations, x = x0's slice; member 1: NaN and +-Inf in the right-hand
    side -- not converged, what the loop gives; members 2 and 3 keep the bits they have in a batch without the other two"""
    import torch
    mats = [_random(200, 700, "csr"), _random(200, 701, "csr"), _random(129, 702, "csr"), _dd(300, 703)]
    Ps = _mixed(mats)
    rhs = [C.rhs(A.shape[0]) for A in mats]
    rhs[0] = np.zeros(200)
    rhs[1][3], rhs[1][77], rhs[1][150] = np.nan, np.inf, -np.inf
    host, offsets = _pack(rhs)
    b = torch.from_numpy(host).cuda()
    x0 = torch.from_numpy(np.random.default_rng(6).standard_normal(b.numel())).cuda()
    As = _device(mats)
    kw = dict(maxiter=6, rtol=1e-12, check_every=2)
    ref = _loop(As, Ps, b, offsets, x0=x0, **kw)
    xh, st = _batch_equals(As, Ps, b, offsets, ref, x0=x0, nan_members=(1,), tag="isolation", **kw)
    assert st["route"] == [0, 0, 0, 0]
    x0h = x0.cpu().numpy()
    assert bool(st["converged"][0]) and int(st["iterations"][0]) == 0 and float(st["relres"][0]) == 0.0
    assert np.array_equal(_bits(xh[offsets[0]:offsets[0] + 200]), _bits(x0h[offsets[0]:offsets[0] + 200]))
    assert not bool(st["converged"][1]) and np.isnan(float(st["relres"][1]))
    assert int(st["iterations"][2]) > 0 and int(st["iterations"][3]) > 0
    # the clean members in a batch of their own
    _batch_equals(As[2:], Ps[2:], b, offsets[2:], ref[2:], x0=x0, tag="clean alone", **kw)


# ---- 5. more members than CUs ----
def test_more_members_than_compute_units():
    """300 ILUTP members of n = 40 with distinct seeds: one launch of 300 workgroups on 256 CUs"""
    import torch
    import ilupp_amd as ilupp
    mats = [_random(40, 1000 + k, "csr") for k in range(300)]
    Ps = ilupp.ILUTPPreconditioner.batch(mats)
    host, offsets = _pack([C.rhs(40) * (1.0 + k / 64.0) for k in range(300)], gap=1)
    b = torch.from_numpy(host).cuda()
    As = _device(mats)
    ref = _loop(As, Ps, b, offsets, maxiter=5)
    _, st = _batch_equals(As, Ps, b, offsets, ref, maxiter=5, tag="300")
    assert st["route"] == [0] * 300


# ---- 6. the cap and the route ----
def test_members_past_the_cap_take_the_single_solve(monkeypatch):
    """ILUPP_BATCH_APPLY_MAX_N = 128: members of n = 64 and 128 are solved in the launch, n = 129 and 300 by the single solve inside the
    same call; all four equal the loop"""
    import torch
    monkeypatch.setenv("ILUPP_BATCH_APPLY_MAX_N", "128")
    mats = [_random(n, 400 + k, "csr") for k, n in enumerate([64, 128, 129, 300])]
    Ps = _mixed(mats)
    host, offsets = _pack([C.rhs(A.shape[0]) for A in mats])
    b = torch.from_numpy(host).cuda()
    As = _device(mats)
    for kw in (dict(maxiter=6), dict(maxiter=40, rtol=1e-9, check_every=1)):
        ref = _loop(As, Ps, b, offsets, **kw)
        _, st = _batch_equals(As, Ps, b, offsets, ref, tag=("cap", kw["maxiter"]), **kw)
        assert st["route"] == [0, 0, 1, 1]


# ---- 7. stream ordering ----
def test_between_a_producer_and_a_consumer_on_a_side_stream():
    """b is filled on a side stream without a sync, bicgstab_batch runs on that stream, a consumer clone behind it: the results equal the
    default-stream call, the gaps keep x0's bits, and a single apply of a member right behind the batched call gives what it gives alone"""
    import torch
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    ns = [150, 65, 257, 40]
    mats = [_random(n, 500 + k, "csr") for k, n in enumerate(ns)]
    Ps = _mixed(mats)
    As = _device(mats)
    host, offsets = _pack([C.rhs(n) for n in ns], gap=7)
    pattern = np.int64(0x7FF4DEADBEEF0123)                   # (a signalling NaN's bits: arithmetic on it would not give it back)
    x0i = np.full(host.shape[0], pattern, dtype=np.int64)
    rng = np.random.default_rng(8)
    for o, n in zip(offsets, ns):
        x0i[o:o + n] = rng.standard_normal(n).view(np.int64)
    x0 = torch.from_numpy(x0i).cuda().view(torch.float64)
    kw = dict(maxiter=7, rtol=1e-13, check_every=3)
    st0 = {}
    want = ild.bicgstab_batch(As, torch.from_numpy(host).cuda(), offsets, Ps, x0=x0, stats=st0, **kw).cpu().numpy()
    v = torch.from_numpy(C.rhs(ns[2])).cuda()
    alone = v.clone()
    _native.set_caller_stream(torch.cuda.current_stream().cuda_stream, True)
    Ps[2].pr.apply_device(alone.data_ptr(), ns[2], sync=True)
    src = torch.from_numpy(host).pin_memory()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = torch.empty(host.shape[0], dtype=torch.float64, device="cuda")
        b.copy_(src, non_blocking=True)                      # the producer: no sync behind it
        x = ild.bicgstab_batch(As, b, offsets, Ps, x0=x0, **kw)
        out = x.clone()                                      # the consumer
        behind = v.clone()
        _native.set_caller_stream(side.cuda_stream, True)
        Ps[2].pr.apply_device(behind.data_ptr(), ns[2], sync=False)      # (the member's own stream waits for the launch that reads its factors and tmp)
    side.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    mask = np.ones(host.shape[0], dtype=bool)
    for o, n in zip(offsets, ns):
        mask[o:o + n] = False
    assert np.all(_bits(got[mask]) == pattern)
    assert np.array_equal(_bits(behind.cpu().numpy()), _bits(alone.cpu().numpy()))
    assert st0["route"] == [0, 0, 0, 0]
    _native.set_caller_stream(torch.cuda.current_stream().cuda_stream, True)


# ---- 8. the checks that need a device tensor ----
def test_argument_checks_on_device_tensors():
    import torch
    import ilupp_amd.device as ild
    mats = [_random(64, 900, "csr"), _random(65, 901, "csr")]
    Ps = _mixed(mats)
    As = _device(mats)
    b = torch.ones(140, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="does not lie inside b"):
        ild.bicgstab_batch(As, b, [0, 76], Ps)
    with pytest.raises(ValueError, match="does not lie inside b"):
        ild.bicgstab_batch(As, b, [-1, 70], Ps)
    with pytest.raises(ValueError, match="the matrix has dimension 65, the preconditioner 64"):
        ild.bicgstab_batch(As[::-1], b, [0, 70], Ps)
    with pytest.raises(ValueError, match="x0: expected shape"):
        ild.bicgstab_batch(As, b, [0, 70], Ps, x0=torch.ones(139, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="x0: expected a contiguous"):
        ild.bicgstab_batch(As, b, [0, 70], Ps, x0=torch.ones(140, dtype=torch.float32, device="cuda"))
    with pytest.raises(RuntimeError, match="appears twice"):
        ild.bicgstab_batch([As[0], As[0]], b, [0, 70], [Ps[0], Ps[0]])
    st = {}
    x = ild.bicgstab_batch([], b, [], [], stats=st)
    assert x.shape == b.shape and x.data_ptr() != b.data_ptr() and float(x.abs().sum()) == 0.0 and st["route"] == []
    # the adapter serves the 1-D solver too, and refuses a block
    M = ild.PivotedOperator(Ps[0])
    x1 = ild.bicgstab(As[0], b[:64].clone(), M, maxiter=3)
    x2 = ild.bicgstab(As[0], b[:64].clone()[:, None], M, maxiter=3)
    assert x1.shape == (64,) and x2.shape == (64, 1) and bool(torch.isfinite(x1).all())
    with pytest.raises(NotImplementedError):
        M.apply_(torch.ones((64, 2), dtype=torch.float64, device="cuda"))


# ---- 9. side by side, in wall time ----
def test_sixteen_solves_side_by_side_beat_the_loop():
    """16 ILUCP members built with .batch, diagonally dominant, n = 4 000, 20 iterations each (rtol = 0: the work is fixed): one
    bicgstab_batch call against the loop of the 16 reference solves on the same objects; medians of five after a warm-up of each"""
    import torch
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    n = 4000
    mats = [_dd(n, 500 + k) for k in range(16)]
    Ps = ilupp.ILUCPPreconditioner.batch(mats)
    As = _device(mats)
    host, offsets = _pack([C.rhs(n) * (1.0 + k / 16.0) for k in range(16)], gap=0)
    b = torch.from_numpy(host).cuda()
    Ms = [ild.PivotedOperator(P) for P in Ps]
    kw = dict(maxiter=20, rtol=0.0, check_every=0)

    def batched():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = ild.bicgstab_batch(As, b, offsets, Ms, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, x

    def looped():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X = [ild.bicgstab(A, b[o:o + n][:, None], M, **kw) for A, M, o in zip(As, Ms, offsets)]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, X

    ref = _loop(As, Ps, b, offsets, **kw)
    _, st = _batch_equals(As, Ps, b, offsets, ref, tag="side by side", **kw)
    assert st["route"] == [0] * 16 and all(it == 20 for _, it, _, _ in ref)
    _, xb = batched()
    _, Xl = looped()
    xb = xb.cpu().numpy()
    assert all(np.array_equal(_bits(xb[o:o + n]), _bits(x[:, 0].cpu().numpy())) for o, x in zip(offsets, Xl))
    t_batch = float(np.median([batched()[0] for _ in range(5)]))
    t_loop = float(np.median([looped()[0] for _ in range(5)]))
    print("ilucp n %d x 16, 20 iterations: t_batch %.5f s, t_loop %.5f s" % (n, t_batch, t_loop))
    assert t_batch < t_loop, (t_batch, t_loop)


# ---- 10. the C entry of the pivoting classes alone, which ilupp_amd.device does not call ----
def test_the_pivot_entry_called_directly_equals_bicgstab_batch(monkeypatch):
    """_native.pivot_bicgstab_batch_device with ILUPP_BATCH_APPLY_MAX_N = 600 on ILUCP / ILUTP members of n = 65, 300 (both sweep arrays
    in LDS: 16 n <= 8 * 600), 513 (one array, the hand-over through tmp) and 700 (route 1: not launched, not solved): the three launched
    members' solutions and their iterations / flags / rr / init words have the bits of device.bicgstab_batch on the same three members
    (and of _native.bicgstab_batch_device, the entry behind it, word for word); the fourth member's slice of x, its words and the gaps
    keep the bits they came with"""
    import torch
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    monkeypatch.setenv("ILUPP_BATCH_APPLY_MAX_N", "600")
    ns = [65, 300, 513, 700]
    mats = [_random(n, 600 + k, "csr") for k, n in enumerate(ns)]
    Ps = _mixed(mats)
    As = _device(mats)
    host, offsets = _pack([C.rhs(n) for n in ns])
    b = torch.from_numpy(host).cuda()
    natives = [P.pr for P in Ps]
    matrices = [(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr(), A.nnz) for A in As]
    pattern = np.int64(0x7FF4DEADBEEF0123)                   # (a signalling NaN's bits: arithmetic on it would not give it back)
    kw = dict(maxiter=7, rtol=0.0, check_every=0)

    def direct(entry, *dims):
        x = torch.full((host.shape[0],), int(pattern), dtype=torch.int64, device="cuda").view(torch.float64)
        work = torch.empty(7 * sum(ns), dtype=torch.float64, device="cuda")
        iters = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        flags = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        rr = torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
        init = torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
        _native.set_caller_stream(torch.cuda.current_stream().cuda_stream, True)
        route = entry(natives, *dims, matrices, b.data_ptr(), 0, x.data_ptr(), offsets, work.data_ptr(), work.numel(), kw["maxiter"],
                      kw["rtol"], kw["check_every"], iters.data_ptr(), flags.data_ptr(), rr.data_ptr(), init.data_ptr(), sync=True)
        torch.cuda.synchronize()
        return route, x.cpu().numpy(), iters.cpu().numpy(), flags.cpu().numpy(), rr, init

    route, xh, iters, flags, rr, init = direct(_native.pivot_bicgstab_batch_device)
    assert route == [0, 0, 0, 1]
    st = {}
    want = ild.bicgstab_batch(As[:3], b, offsets[:3], Ps[:3], stats=st, **kw).cpu().numpy()
    assert st["route"] == [0, 0, 0]
    relres = (torch.sqrt(rr) / init).cpu().numpy()           # (as bicgstab_batch computes it from the two words)
    for k in range(3):
        o, n = offsets[k], ns[k]
        assert np.array_equal(_bits(xh[o:o + n]), _bits(want[o:o + n])), (k, "x", float(np.max(np.abs(xh[o:o + n] - want[o:o + n]))))
        assert int(iters[k]) == int(st["iterations"][k]) == 7, (k, "iterations", int(iters[k]), int(st["iterations"][k]))
        assert bool(flags[k] & 2) == bool(st["converged"][k]) and not flags[k] & (4 | 8), (k, "flags", int(flags[k]))
        assert np.array_equal(_bits(relres[k:k + 1]), _bits(st["relres"][k:k + 1].numpy())), (k, "relres", float(relres[k]), float(st["relres"][k]))
        assert np.all(np.isfinite(xh[o:o + n]))
    # the same words from the entry bicgstab_batch goes through, all four members named
    route2, xh2, iters2, flags2, rr2, init2 = direct(_native.bicgstab_batch_device, ns)
    assert route2 == [0, 0, 0, 1]
    assert np.array_equal(_bits(xh), _bits(xh2))
    assert np.array_equal(iters, iters2) and np.array_equal(flags, flags2)
    assert np.array_equal(_bits(rr.cpu().numpy()), _bits(rr2.cpu().numpy())) and np.array_equal(_bits(init.cpu().numpy()), _bits(init2.cpu().numpy()))
    # the member that was not launched, and the gaps
    mask = np.ones(host.shape[0], dtype=bool)
    for o, n in zip(offsets[:3], ns[:3]):
        mask[o:o + n] = False
    assert np.all(_bits(xh[mask]) == pattern)
    assert int(iters[3]) == -1 and int(flags[3]) == -1 and float(rr.cpu()[3]) == -1.0 and float(init.cpu()[3]) == -1.0
