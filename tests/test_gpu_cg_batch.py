"""GPU tests of the batched apply and the batched CG solve of the NON-pivoting classes (ilupp_amd.device.apply_batch_ over
ilupp_hip_apply_batch_device: k_pivot_apply_batch on descriptors without a permutation; ilupp_amd.device.cg_batch over
ilupp_hip_cg_batch_device: one launch of k_cg_batch, one workgroup per system with the whole preconditioned loop inside it).  Parity is
bitwise throughout, against what exists without the batch, one member at a time: M.apply_ on a clone, and
ilupp_amd.device.cg(A_k, b_k[:, None], M_k, ...) -- the solution on its int64 view, the iteration count, the converged flag and the bits
of the relative residual."""
import ctypes
import time

import numpy as np
import pytest
import scipy.sparse as sp

import matgen

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 65, 256, 257, 300, 513]          # one row; a wave and one; one chunk of the dot, 2 chunks of 129, of 150, 3 chunks of 171
KINDS = ["ILU0", "ILUT", "ILUC", "IChol0", "ICholT"]
PATTERN = np.int64(0x7FF4DEADBEEF0123)          # (a signalling NaN's bits: arithmetic on it would not give it back)


def _spd(n, seed):
    A = sp.csr_matrix(matgen.symmetrize(*matgen.random_dd(n, 8, 25.0, seed)), shape=(n, n))
    A.sort_indices()
    return A


def _poisson(g):
    d, i, p = matgen.poisson3d(g)
    n = p.shape[0] - 1
    return sp.csr_matrix((d, i, p), shape=(n, n))


def _rhs(n, seed=0):
    return np.random.default_rng(1000 + seed).standard_normal(n) + 2.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


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


def _gaps(host_len, offsets, ns):
    mask = np.ones(host_len, dtype=bool)
    for o, n in zip(offsets, ns):
        mask[o:o + n] = False
    return mask


def _member(kind, A, dA, how, **params):
    """one member three ways: 0 = a DevicePreconditioner, 1 = the host class of the ctypes binding itself, 2 = a FactorOperator of it"""
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    if how == 0:
        return ild.DevicePreconditioner(kind, dA, **params)
    defaults = {"ILUT": dict(fill_in=100, threshold=0.1), "ILUC": dict(fill_in=100, threshold=0.1), "ICholT": dict(add_fill_in=0, threshold=0.0)}
    kw = dict(defaults.get(kind, {}))
    kw.update(params)
    P = getattr(ilupp, kind + "Preconditioner")(A, **kw)
    return P if how == 1 else ild.FactorOperator(P)


def _single(M):
    """what applies or solves with a member alone"""
    import ilupp_amd.device as ild
    return M if (M is None or hasattr(M, "apply_")) else ild.FactorOperator(M)


def _device(mats):
    import ilupp_amd.device as ild
    return [ild.DeviceCSR.from_scipy(A) for A in mats]


# ---- 1. apply parity ----
@pytest.fixture(scope="module")
def apply_members():
    mats = [_spd(n, 40 + k) for k, n in enumerate(SIZES)] + [_poisson(8)]
    dAs = _device(mats)
    members, ns = [], []
    for k, (A, dA) in enumerate(zip(mats, dAs)):
        for j, kind in enumerate(KINDS):
            members.append(_member(kind, A, dA, (k + j) % 3))
            ns.append(A.shape[0])
    return members, ns


@pytest.mark.parametrize("transpose", [False, True])
def test_apply_batch_equals_the_single_applies(apply_members, transpose):
    """all five kinds on every matrix (n = 1, 2, 65, 256, 257, 300, 513 and poisson3d(8)), DevicePreconditioners, host classes and
    FactorOperators in turn, in ONE call: every vector has the bits of M.apply_ on a clone, and the signalling-NaN pattern between the
    vectors survives"""
    import torch
    import ilupp_amd.device as ild
    members, ns = apply_members
    host, offsets = _pack([_rhs(n, k) for k, n in enumerate(ns)], gap=5)
    hi = host.view(np.int64)
    hi[_gaps(host.shape[0], offsets, ns)] = PATTERN
    x = torch.from_numpy(host.copy()).cuda()
    want = [_single(M).apply_(x[o:o + n].clone(), transpose=transpose).cpu().numpy() for M, o, n in zip(members, offsets, ns)]
    route = ild.apply_batch_(members, x, offsets, transpose=transpose)
    assert route == [0] * len(members)
    got = x.cpu().numpy()
    for k, (o, n, w) in enumerate(zip(offsets, ns, want)):
        assert np.array_equal(_bits(got[o:o + n]), _bits(w)), (k, KINDS[k % 5], n, transpose)
        assert np.all(np.isfinite(w))
    assert np.all(_bits(got)[_gaps(host.shape[0], offsets, ns)] == PATTERN)


STATIC_GRID = (6, 6, 6)          # the smallest cube whose IChol0 and ILU0 objects both apply through static sweeps (5^3: the CSR sweeps still)


def test_a_member_whose_single_apply_takes_a_static_form():
    """IChol0 and ILU0 of a box grid whose single applies run static sweeps (pr.path() says so) go to the launch all the same, swept from
    their CSR triangles, with the single applies' bits, in both directions"""
    import torch
    import ilupp_amd.device as ild
    d, i, p = matgen.poisson3d(*STATIC_GRID)
    n = p.shape[0] - 1
    A = sp.csr_matrix((d * (1.0 + 0.25 * np.random.default_rng(3).random(d.shape[0])), i, p), shape=(n, n))
    A = ((A + A.T) / 2).tocsr()
    A.sort_indices()
    dA = ild.DeviceCSR.from_scipy(A)
    members = [ild.DevicePreconditioner("IChol0", dA), ild.DevicePreconditioner("ILU0", dA), ild.DevicePreconditioner("ICholT", dA)]
    paths = [M.pr.path() for M in members]
    print("paths of the %s grid: %s" % (STATIC_GRID, paths))
    assert "static" in paths[0] and "static" in paths[1], paths
    assert n <= ild._native.cg_batch_max_n()
    v = torch.from_numpy(_rhs(n, 9)).cuda()
    before = [M.apply_(v.clone()).cpu().numpy() for M in members]
    for M in members[:2]:
        assert any(name.startswith(("k_sptrsv_st", "k_sptrsv_wv", "k_sptrsv_wx")) for name in M.pr.kernel_names()), M.pr.kernel_names()
    for transpose in (False, True):
        host, offsets = _pack([_rhs(n, k) for k in range(3)])
        x = torch.from_numpy(host).cuda()
        want = [M.apply_(x[o:o + n].clone(), transpose=transpose).cpu().numpy() for M, o in zip(members, offsets)]
        assert ild.apply_batch_(members, x, offsets, transpose=transpose) == [0, 0, 0]
        got = x.cpu().numpy()
        for k, (o, w) in enumerate(zip(offsets, want)):
            assert np.array_equal(_bits(got[o:o + n]), _bits(w)), (k, transpose)
    # and the objects still apply alone as before, on the same path
    assert [M.pr.path() for M in members] == paths
    for M, w in zip(members, before):
        assert np.array_equal(_bits(M.apply_(v.clone()).cpu().numpy()), _bits(w))


# ---- 2. solve parity ----
def _loop(As, Ms, b, offsets, x0=None, **kw):
    """the reference: one member at a time through device.cg; per member (x, iterations, converged, relres)"""
    import ilupp_amd.device as ild
    out = []
    for A, M, o in zip(As, Ms, offsets):
        st = {}
        x = ild.cg(A, b[o:o + A.n][:, None], _single(M), x0=None if x0 is None else x0[o:o + A.n][:, None], stats=st, **kw)
        out.append((x[:, 0].cpu().numpy(), int(st["iterations"][0]), bool(st["converged"][0]), st["relres"].numpy().copy()))
    return out


def _batch_equals(As, Ms, b, offsets, ref, x0=None, nan_members=(), tag="", **kw):
    """cg_batch against `ref` (what _loop gave): the solutions on their int64 views (equal_nan for the members of nan_members, whose
    NaNs need not share a payload), iterations, converged and the bits of relres.  Returns (x on the host, stats)."""
    import ilupp_amd.device as ild
    st = {}
    x = ild.cg_batch(As, b, offsets, Ms, x0=x0, stats=st, **kw)
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


SOLVE_KINDS = [("IChol0", {}), ("ICholT", dict(add_fill_in=0, threshold=0.0)), ("ICholT", dict(add_fill_in=8, threshold=1e-3)), ("ILU0", {}), (None, {})]


def _tiny_rhs(dA, M, base):
    """The right-hand side of a member of n <= 2: CG solves such a system in one or two steps, and where that leaves r exactly zero
    before the first check the loop divides 0 by 0 in the next iteration and stops as broken down instead of converged (which of the two
    happens is a matter of the last bit of b).  So: the first of a seeded sequence for which the single solve -- the reference alone --
    converges with check_every = 3.  (The break-down of such members is compared as well: the run with check_every = 0.)"""
    import torch
    import ilupp_amd.device as ild
    for seed in range(64):
        v = _rhs(dA.n, base + 1000 * seed)
        st = {}
        ild.cg(dA, torch.from_numpy(v).cuda()[:, None], _single(M), maxiter=40, rtol=1e-10, check_every=3, stats=st)
        if bool(st["converged"][0]):
            return v
    raise AssertionError("no right-hand side of 64 lets the single solve of a tiny member converge")


@pytest.fixture(scope="module")
def solve_members():
    import torch
    mats = [_spd(n, 60 + k) for k, n in enumerate(SIZES + [512])] + [_poisson(8)]
    dAs = _device(mats)
    As, Ms, rhs = [], [], []
    for k, (A, dA) in enumerate(zip(mats, dAs)):
        for j, (kind, params) in enumerate(SOLVE_KINDS):
            As.append(dA)
            Ms.append(None if kind is None else _member(kind, A, dA, (k + j) % 3, **params))
            rhs.append(_tiny_rhs(dA, Ms[-1], 7 * k + j) if A.shape[0] <= 2 else _rhs(A.shape[0], 7 * k + j) * (1.0 + j / 4.0))
    host, offsets = _pack(rhs)
    return As, Ms, torch.from_numpy(host).cuda(), offsets


@pytest.mark.parametrize("check_every", [0, 1, 3])
def test_solves_equal_the_loop(solve_members, check_every):
    """IChol0, ICholT(0, 0), ICholT with fill, ILU0 and no preconditioner on every matrix (n = 1, 2, 65, 256, 257, 300, 512, 513 and
    poisson3d(8)) in ONE batch.  check_every = 0: at most 6 iterations each, nobody converges (the members of n <= 2 are exact after one
    or two and break down or run on, as the last bit has it).  check_every = 1 and 3 with rtol = 1e-10, at most
    40 iterations: asserted on the LOOP's stats before the comparison -- every member converges, and not all at the same iteration
    (the matrices are diagonally dominant: the preconditioned members need a few iterations, the bare ones more, n = 1 one) -- so the
    comparison is of members that stop alone."""
    As, Ms, b, offsets = solve_members
    kw = dict(maxiter=6, check_every=0) if check_every == 0 else dict(maxiter=40, rtol=1e-10, check_every=check_every)
    ref = _loop(As, Ms, b, offsets, **kw)
    its = [it for _, it, _, _ in ref]
    print("check_every %d: iterations of the reference loop %s" % (check_every, its))
    if check_every:
        assert all(conv for _, _, conv, _ in ref), [k for k, r in enumerate(ref) if not r[2]]
        assert len(set(its)) >= 2 and all(0 < it < 40 for it in its), its
        assert all(float(rel[0]) <= 1e-10 for _, _, _, rel in ref)
    else:
        assert max(its) == 6 and not any(conv for _, _, conv, _ in ref)
    xh, st = _batch_equals(As, Ms, b, offsets, ref, tag=("solve", check_every), **kw)
    assert st["route"] == [0] * len(As)
    assert np.all(_bits(xh[_gaps(xh.shape[0], offsets, [A.n for A in As])]) == 0)          # (the gaps: zeros, untouched)


# ---- 3. x0 ----
def test_a_start_vector_and_an_exact_one(solve_members):
    """x0 given: used as the loop uses it, the gaps keep x0's bits; two members whose x0 is exact (b = A x0 by the library's
    own SpMV, so r is zero to the bit) leave at once: converged, 0 iterations, x = x0"""
    import torch
    As, Ms, b, offsets = solve_members
    As, Ms, offsets = As[10:25], Ms[10:25], offsets[10:25]
    ns = [A.n for A in As]
    x0i = np.full(b.numel(), PATTERN, dtype=np.int64)
    rng = np.random.default_rng(5)
    for o, n in zip(offsets, ns):
        x0i[o:o + n] = rng.standard_normal(n).view(np.int64)
    x0 = torch.from_numpy(x0i).cuda().view(torch.float64)
    b = b.clone()
    exact = (3, 9)
    for k in exact:
        o, n = offsets[k], ns[k]
        b[o:o + n] = As[k].matmat(x0[o:o + n].clone()[:, None])[:, 0]
    for kw in (dict(maxiter=4, check_every=0), dict(maxiter=40, rtol=1e-10, check_every=2)):
        ref = _loop(As, Ms, b, offsets, x0=x0, **kw)
        xh, st = _batch_equals(As, Ms, b, offsets, ref, x0=x0, tag=("x0", kw["maxiter"]), **kw)
        assert np.all(_bits(xh)[_gaps(xh.shape[0], offsets, ns)] == PATTERN)                  # (the gaps keep x0's bits)
        for k in exact:
            o, n = offsets[k], ns[k]
            assert bool(st["converged"][k]) and int(st["iterations"][k]) == 0 and float(st["relres"][k]) == 0.0
            assert np.array_equal(_bits(xh[o:o + n]), x0i[o:o + n])
        assert any(int(st["iterations"][k]) > 0 for k in range(len(As)) if k not in exact)


# ---- 4. isolation and breakdown ----
def test_zero_nan_and_indefinite_members_leave_the_others_alone():
    """member 0: an all-zero right-hand side -- converged at once, 0 iterations, x = x0's slice; member 1: NaN and +-Inf in the right-hand
    side -- not converged, what the loop gives; members 2 and 3: diag(+1, -1, +1, ...) of even size with b = ones, p^T A p = 0 in the
    first iteration -- they stop as not converged with the loop's x (= x0 = 0 for them); members 4 - 6 keep the bits they have in a batch
    without the others"""
    import torch
    import ilupp_amd.device as ild
    n_ind = 66
    ind = sp.diags(np.where(np.arange(n_ind) % 2 == 0, 1.0, -1.0), format="csr")
    mats = [_spd(200, 700), _spd(200, 701), ind, ind.copy(), _spd(129, 702), _spd(300, 703), _spd(257, 704)]
    As = _device(mats)
    Ms = [ild.DevicePreconditioner("IChol0", As[0]), ild.DevicePreconditioner("ILU0", As[1]), ild.DevicePreconditioner("ILU0", As[2]), None,
          ild.DevicePreconditioner("ICholT", As[4]), None, ild.DevicePreconditioner("IChol0", As[6])]
    rhs = [_rhs(A.shape[0], k) for k, A in enumerate(mats)]
    rhs[0] = np.zeros(200)
    rhs[1][3], rhs[1][77], rhs[1][150] = np.nan, np.inf, -np.inf
    rhs[2] = np.ones(n_ind)
    rhs[3] = np.ones(n_ind)
    host, offsets = _pack(rhs)
    b = torch.from_numpy(host).cuda()
    x0h = np.random.default_rng(6).standard_normal(b.numel())
    for k in (2, 3):
        x0h[offsets[k]:offsets[k] + n_ind] = 0.0
    x0 = torch.from_numpy(x0h).cuda()
    kw = dict(maxiter=6, rtol=1e-12, check_every=2)
    ref = _loop(As, Ms, b, offsets, x0=x0, **kw)
    xh, st = _batch_equals(As, Ms, b, offsets, ref, x0=x0, nan_members=(1,), tag="isolation", **kw)
    assert st["route"] == [0] * 7
    assert bool(st["converged"][0]) and int(st["iterations"][0]) == 0 and float(st["relres"][0]) == 0.0
    assert np.array_equal(_bits(xh[offsets[0]:offsets[0] + 200]), _bits(x0h[offsets[0]:offsets[0] + 200]))
    assert not bool(st["converged"][1]) and np.isnan(float(st["relres"][1]))
    for k in (2, 3):
        assert not bool(st["converged"][k]) and int(st["iterations"][k]) == 0 and float(st["relres"][k]) == 1.0
        assert np.all(xh[offsets[k]:offsets[k] + n_ind] == 0.0)
    assert all(int(st["iterations"][k]) > 0 for k in (4, 5, 6))
    # the clean members in a batch of their own
    _batch_equals(As[4:], Ms[4:], b, offsets[4:], ref[4:], x0=x0, tag="clean alone", **kw)


# ---- 5. more members than CUs ----
def test_more_members_than_compute_units():
    """300 members of n = 40 with distinct seeds, IChol0, none and ILU0 in turn: one launch of 300 workgroups on 256 CUs"""
    import torch
    import ilupp_amd.device as ild
    mats = [_spd(40, 1000 + k) for k in range(300)]
    As = _device(mats)
    Ms = [None if k % 3 == 1 else ild.DevicePreconditioner("IChol0" if k % 3 == 0 else "ILU0", A) for k, A in enumerate(As)]
    host, offsets = _pack([_rhs(40, k) * (1.0 + k / 64.0) for k in range(300)], gap=1)
    b = torch.from_numpy(host).cuda()
    ref = _loop(As, Ms, b, offsets, maxiter=4)
    _, st = _batch_equals(As, Ms, b, offsets, ref, maxiter=4, tag="300")
    assert st["route"] == [0] * 300


# ---- 6. the cap and the routes ----
def test_both_lds_paths_and_a_member_past_the_cap(monkeypatch):
    """ILUPP_BATCH_APPLY_MAX_N = 600 (4 800 bytes for the sweeps): n = 300 keeps both arrays in LDS (16 n = 4 800), n = 513 takes the
    one-array path through tmp (16 n > 4 800 >= 8 n), n = 700 exceeds the cap and goes through the single apply / single solve inside the
    same call; every member equals its single apply and its single solve"""
    import torch
    import ilupp_amd.device as ild
    monkeypatch.setenv("ILUPP_BATCH_APPLY_MAX_N", "600")
    assert ild._native.cg_batch_max_n() == 600
    mats = [_spd(n, 400 + k) for k, n in enumerate([300, 513, 700, 513, 300])]
    ns = [A.shape[0] for A in mats]
    As = _device(mats)
    Ms = [ild.DevicePreconditioner(kind, A) for kind, A in zip(["IChol0", "ICholT", "IChol0", "ILU0", "ILUT"], As)]
    host, offsets = _pack([_rhs(n, k) for k, n in enumerate(ns)])
    for transpose in (False, True):
        x = torch.from_numpy(host).cuda()
        want = [M.apply_(x[o:o + n].clone(), transpose=transpose).cpu().numpy() for M, o, n in zip(Ms, offsets, ns)]
        assert ild.apply_batch_(Ms, x, offsets, transpose=transpose) == [0, 0, 1, 0, 0]
        got = x.cpu().numpy()
        for k, (o, n, w) in enumerate(zip(offsets, ns, want)):
            assert np.array_equal(_bits(got[o:o + n]), _bits(w)), (k, transpose)
    b = torch.from_numpy(host).cuda()
    Ms[4] = None
    for kw in (dict(maxiter=5), dict(maxiter=40, rtol=1e-10, check_every=1)):
        ref = _loop(As, Ms, b, offsets, **kw)
        _, st = _batch_equals(As, Ms, b, offsets, ref, tag=("cap", kw["maxiter"]), **kw)
        assert st["route"] == [0, 0, 1, 0, 0]


# ---- 7. stream ordering ----
def test_between_a_producer_and_a_consumer_on_a_side_stream():
    """b is filled on a side stream without a sync, cg_batch runs on that stream, a consumer clone behind it: the results equal the
    default-stream call and the gaps keep x0's bits; a single apply_ of a member right behind the batched call gives what it gives
    alone; and an ILU(0) member re-factorised right behind the call, for other values, is not seen by the launch -- while the next
    batched apply and the next single apply see the new factor"""
    import torch
    import ilupp_amd.device as ild
    ns = [150, 65, 257, 40]
    mats = [_spd(n, 500 + k) for k, n in enumerate(ns)]
    As = _device(mats)
    Ms = [ild.DevicePreconditioner("IChol0", As[0]), ild.DevicePreconditioner("ILU0", As[1]), ild.DevicePreconditioner("ICholT", As[2]),
          ild.DevicePreconditioner("ILU0", As[3])]
    # member 1's matrix with other values on the same pattern, and what its new factor gives
    A1b = mats[1].copy()
    A1b.data = A1b.data * (1.0 + 0.5 * np.random.default_rng(2).random(A1b.nnz))
    A1b = ((A1b + A1b.T) / 2).tocsr()
    A1b.sort_indices()
    assert np.array_equal(A1b.indices, mats[1].indices)
    dA1b = ild.DeviceCSR.from_scipy(A1b)
    fresh = ild.DevicePreconditioner("ILU0", dA1b)
    v1 = torch.from_numpy(_rhs(ns[1], 11)).cuda()
    new_alone = fresh.apply_(v1.clone()).cpu().numpy()
    old_alone = Ms[1].apply_(v1.clone()).cpu().numpy()
    assert not np.array_equal(new_alone, old_alone)
    host, offsets = _pack([_rhs(n, k) for k, n in enumerate(ns)], gap=7)
    x0i = np.full(host.shape[0], PATTERN, dtype=np.int64)
    rng = np.random.default_rng(8)
    for o, n in zip(offsets, ns):
        x0i[o:o + n] = rng.standard_normal(n).view(np.int64)
    x0 = torch.from_numpy(x0i).cuda().view(torch.float64)
    kw = dict(maxiter=7, rtol=1e-13, check_every=3)
    st0 = {}
    want = ild.cg_batch(As, torch.from_numpy(host).cuda(), offsets, Ms, x0=x0, stats=st0, **kw).cpu().numpy()
    assert st0["route"] == [0, 0, 0, 0]
    v = torch.from_numpy(_rhs(ns[2], 12)).cuda()
    alone = Ms[2].apply_(v.clone()).cpu().numpy()
    src = torch.from_numpy(host).pin_memory()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = torch.empty(host.shape[0], dtype=torch.float64, device="cuda")
        b.copy_(src, non_blocking=True)                      # the producer: no sync behind it
        x = ild.cg_batch(As, b, offsets, Ms, x0=x0, **kw)
        out = x.clone()                                      # the consumer
        behind = Ms[2].apply_(v.clone())                     # a single apply of a member right behind the launch
        ild._on_current_stream()
        Ms[1].pr.refactor_device(dA1b.data.data_ptr(), dA1b.indices.data_ptr(), dA1b.indptr.data_ptr())      # (waits for the launch that reads the old factor)
        again = torch.stack([v1, v1]).reshape(-1).contiguous()
        ild.apply_batch_([Ms[1]], again, [0])                # a launch of one member: the new factor
        single = Ms[1].apply_(v1.clone())
    side.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.all(_bits(got)[_gaps(host.shape[0], offsets, ns)] == PATTERN)
    assert np.array_equal(_bits(behind.cpu().numpy()), _bits(alone))
    againh = again.cpu().numpy()
    assert np.array_equal(_bits(againh[:ns[1]]), _bits(new_alone)) and np.array_equal(_bits(againh[ns[1]:]), _bits(v1.cpu().numpy()))
    assert np.array_equal(_bits(single.cpu().numpy()), _bits(new_alone))
    ild._on_current_stream()


# ---- 8. the refusals that need built objects ----
def test_refusals_that_need_built_objects():
    import torch
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    mats = [_spd(64, 900), _spd(65, 901)]
    As = _device(mats)
    Ms = [ild.DevicePreconditioner("IChol0", A) for A in As]
    b = torch.ones(140, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="appears twice"):
        ild.cg_batch([As[0], As[0]], b, [0, 70], [Ms[0], Ms[0]])
    with pytest.raises(RuntimeError, match="appears twice"):
        ild.apply_batch_([Ms[0], Ms[0]], b, [0, 70])
    st = {}
    x = ild.cg_batch([], b, [], [], stats=st)
    assert x.shape == b.shape and x.data_ptr() != b.data_ptr() and float(x.abs().sum()) == 0.0 and st["route"] == []
    assert ild.apply_batch_([], b, []) == []
    # the C entries name a multilevel handle instead of reading it as a factor pair, and a dimension that is not the member's
    params = ilupp.iluplusplus_precond_parameter()
    params.default_configuration(1)
    ml = ild.DevicePreconditioner("ILUpp", As[0], params=params)
    lib, VP = _native.lib(), ctypes.c_void_p
    keep = b.clone()
    route = (ctypes.c_int32 * 1)()
    rc = lib.ilupp_hip_apply_batch_device(1, (VP * 1)(ml.pr._h), b.data_ptr(), (ctypes.c_int64 * 1)(0), 0, 1, route)
    assert rc == -1 and lib.ilupp_hip_last_error().decode() == "a multilevel preconditioner cannot be a member of a batch"
    with pytest.raises(RuntimeError, match="wrong size"):
        _native.cg_batch_device([Ms[0].pr], [65], [(As[1].data.data_ptr(), As[1].indices.data_ptr(), As[1].indptr.data_ptr(), As[1].nnz)],
                                b.data_ptr(), 0, b.data_ptr(), [0], b.data_ptr(), 5 * 65, 3, 0.0, 0, b.data_ptr(), b.data_ptr(), b.data_ptr(),
                                b.data_ptr())
    assert torch.equal(b, keep)
    # the adapter serves the 1-D solver and a block
    H = ilupp.IChol0Preconditioner(mats[0])
    M = ild.FactorOperator(H)
    assert (M.kind, M.n) == ("IChol0", 64)
    x1 = ild.cg(As[0], b[:64].clone(), M, maxiter=3)
    X2 = ild.cg(As[0], torch.stack([b[:64], 2.0 * b[:64]], dim=1).contiguous(), M, maxiter=3)
    assert x1.shape == (64,) and X2.shape == (64, 2) and bool(torch.isfinite(X2).all())
    assert np.array_equal(_bits(X2[:, 0].cpu().numpy()), _bits(ild.cg(As[0], b[:64].clone()[:, None], M, maxiter=3)[:, 0].cpu().numpy()))


# ---- 9. side by side, in wall time ----
def test_sixteen_solves_side_by_side_beat_the_loop():
    """16 IChol0 members, n = 4 000, 20 iterations each (rtol = 0: the work is fixed): one cg_batch call against the loop of the 16 single
    device.cg solves on the same objects, measured in this test; medians of five after a warm-up of each"""
    import torch
    import ilupp_amd.device as ild
    n = 4000
    mats = [_spd(n, 500 + k) for k in range(16)]
    As = _device(mats)
    Ms = [ild.DevicePreconditioner("IChol0", A) for A in As]
    host, offsets = _pack([_rhs(n, k) * (1.0 + k / 16.0) for k in range(16)], gap=0)
    b = torch.from_numpy(host).cuda()
    kw = dict(maxiter=20, rtol=0.0, check_every=0)

    def batched():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = ild.cg_batch(As, b, offsets, Ms, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, x

    def looped():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X = [ild.cg(A, b[o:o + n][:, None], M, **kw) for A, M, o in zip(As, Ms, offsets)]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, X

    ref = _loop(As, Ms, b, offsets, **kw)
    _, st = _batch_equals(As, Ms, b, offsets, ref, tag="side by side", **kw)
    assert st["route"] == [0] * 16 and all(it == 20 for _, it, _, _ in ref)
    batched(), looped()
    t_batch = float(np.median([batched()[0] for _ in range(5)]))
    t_loop = float(np.median([looped()[0] for _ in range(5)]))
    print("ichol0 n %d x 16, 20 iterations: t_batch %.5f s, t_loop %.5f s" % (n, t_batch, t_loop))
    assert t_batch < t_loop, (t_batch, t_loop)
