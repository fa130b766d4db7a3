"""GPU tests of the batched ILU(0) re-factorisation (ilupp_amd.device.refactor_batch_ over ilupp_hip_ilu0_refactor_batch_device: one launch
of k_ilu0_refactor_batch, one workgroup per member) and of DevicePreconditioner.refactor_.  Every comparison is bitwise on int64 views.
The reference for the FACTORS is a freshly constructed DevicePreconditioner("ILU0", A') (factor_copy of L and U: pointers and indices equal,
values bit-equal); the reference for BEHAVIOUR is a twin object re-factorised by the single refactor_device.  A' is A with every value
scaled by 1 + 0.1 u, u uniform in [0, 1) from a fixed seed, the diagonal included: it stays diagonally dominant."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import matgen

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 65, 256, 257, 300, 513]          # one row; two; a wave and one; the workgroup's 256 lanes, one more (a second round); odd sizes


def _csr(t):
    d, i, p = t
    n = p.shape[0] - 1
    A = sp.csr_matrix((np.asarray(d, dtype=np.float64), i, p), shape=(n, n))
    A.sort_indices()
    return A


def _random(n, seed, k=8):
    return _csr(matgen.random_dd(n, k, 25.0, seed))


def _spd(n, seed):
    A = sp.csr_matrix(matgen.symmetrize(*matgen.random_dd(n, 8, 25.0, seed)), shape=(n, n))
    A.sort_indices()
    return A


def _arrow(n):
    """diagonal plus a full last row and a full last column, unsymmetric values, diagonally dominant"""
    rng = np.random.default_rng(77)
    A = sp.lil_matrix((n, n))
    A.setdiag(25.0 + rng.random(n))
    A[n - 1, :n - 1] = rng.random(n - 1)
    A[:n - 1, n - 1] = rng.random((n - 1, 1))
    A[n - 1, n - 1] = float(n) + 25.0
    A = A.tocsr()
    A.sort_indices()
    return A


def _scaled(A, seed):
    """A': the same pattern, every value scaled by 1 + 0.1 u"""
    B = A.copy()
    B.data = A.data * (1.0 + 0.1 * np.random.default_rng(seed).random(A.data.shape[0]))
    return B


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _dev(A):
    import ilupp_amd.device as ild
    return ild.DeviceCSR.from_scipy(A)


def _member(A, dA, how):
    """one ILU0 member three ways: 0 = a DevicePreconditioner, 1 = the host class of the ctypes binding itself, 2 = a FactorOperator of it"""
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    if how == 0:
        return ild.DevicePreconditioner("ILU0", dA)
    P = ilupp.ILU0Preconditioner(A)
    return P if how == 1 else ild.FactorOperator(P)


def _single(M):
    import ilupp_amd.device as ild
    return M if hasattr(M, "apply_") else ild.FactorOperator(M)


def _native_of(M):
    return M.pr


def _factors(M):
    """(L, U) as (data, indices, indptr) triples from factor_copy"""
    return [(f[0], f[1], f[2]) for f in _native_of(M).factors_info()]


def _same_factors(F, G):
    return len(F) == len(G) == 2 and all(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(_bits(a[0]), _bits(b[0]))
                                         for a, b in zip(F, G))


def _refactor_single(M, dA):
    import ilupp_amd.device as ild
    ild._on_current_stream()
    _native_of(M).refactor_device(dA.data.data_ptr(), dA.indices.data_ptr(), dA.indptr.data_ptr())


def _rhs(n, seed=0):
    return np.random.default_rng(2000 + seed).standard_normal(n) + 2.0


def _three_applies(M, n, seed):
    """apply_ in both directions and a block apply_ of k = 3, on clones: the host copies"""
    import torch
    S = _single(M)
    v = torch.from_numpy(_rhs(n, seed)).cuda()
    X = torch.from_numpy(np.random.default_rng(3000 + seed).standard_normal((n, 3)) + 2.0).cuda().contiguous()
    return [S.apply_(v.clone()).cpu().numpy(), S.apply_(v.clone(), transpose=True).cpu().numpy(), S.apply_(X.clone()).cpu().numpy()]


# ---- 1. parity, routes and stale copies: one batch of every kind of member ----
def _parity_matrices():
    mats = [("random_dd(%d)" % n, _random(n, 500 + k)) for k, n in enumerate(SIZES)]
    mats.append(("laplace1d(300)", _csr(matgen.laplace1d(300))))          # every row waits for the one before: the longest chain
    mats.append(("poisson2d(16)", _csr(matgen.poisson2d(16))))            # 5-point: takes no static form
    mats.append(("arrow(300)", _arrow(300)))                              # a row as long as n: above the row cap, route 1
    mats.append(("random_dd(1100, 19)", _random(1100, 520, k=19)))        # level-ordered factor path: fperm set, lvl[] copies after an apply
    mats.append(("poisson3d(6)", _csr(matgen.poisson3d(6))))              # static form: route 2
    return mats


@pytest.fixture(scope="module")
def parity():
    import ilupp_amd.device as ild
    mats = _parity_matrices()
    out = dict(names=[m[0] for m in mats], ns=[m[1].shape[0] for m in mats])
    As = [m[1] for m in mats]
    A2 = [_scaled(A, 40 + k) for k, A in enumerate(As)]
    dAs, dA2 = [_dev(A) for A in As], [_dev(A) for A in A2]
    members = [_member(A, dA, k % 3) for k, (A, dA) in enumerate(zip(As, dAs))]
    twins = [_member(A, dA, k % 3) for k, (A, dA) in enumerate(zip(As, dAs))]
    out["paths"] = [_native_of(M).path() for M in members]
    out["old"] = [_factors(M) for M in members]
    # stale copies: packed, transposed and level-ordered copies of the OLD values exist in every member before the call
    out["before"] = [_three_applies(M, n, k) for k, (M, n) in enumerate(zip(members, out["ns"]))]
    out["routes"] = ild.refactor_batch_(members, dA2)
    out["got"] = [_factors(M) for M in members]
    out["after"] = [_three_applies(M, n, k) for k, (M, n) in enumerate(zip(members, out["ns"]))]
    out["fresh"] = [_factors(ild.DevicePreconditioner("ILU0", dA)) for dA in dA2]
    for T, dA in zip(twins, dA2):
        _refactor_single(T, dA)
    out["twin"] = [_factors(T) for T in twins]
    out["twin_after"] = [_three_applies(T, n, k) for k, (T, n) in enumerate(zip(twins, out["ns"]))]
    return out


def test_factors_equal_a_fresh_construction(parity):
    print("paths: %s" % list(zip(parity["names"], parity["paths"], parity["routes"])))
    for k, name in enumerate(parity["names"]):
        assert _same_factors(parity["got"][k], parity["fresh"][k]), name
        assert _same_factors(parity["got"][k], parity["twin"][k]), name
        if parity["ns"][k] > 1:
            assert not _same_factors(parity["got"][k], parity["old"][k]), name          # (the values did change)


def test_routes(parity):
    names, routes, paths = parity["names"], parity["routes"], parity["paths"]
    print("routes: %s" % list(zip(names, paths, routes)))
    for name, path, rt in zip(names, paths, routes):
        assert rt == (2 if "static" in path else 1 if name == "arrow(300)" else 0), (name, path, rt)
    for name, rt in zip(names, routes):
        if name.startswith("random_dd") or name in ("poisson2d(16)", "laplace1d(300)"):
            assert rt == 0, (name, rt)
    assert routes[names.index("poisson3d(6)")] == 2
    assert parity["paths"][names.index("random_dd(1100, 19)")] == "ilu0:level-order"


def test_applies_after_the_call_equal_the_twins(parity):
    """apply_ in both directions and a block apply_ of k = 3: every member had run all three BEFORE the call (so that the packed, the
    transposed and the level-ordered copies of the old values existed), and has the twin's bits afterwards"""
    for k, name in enumerate(parity["names"]):
        for j in range(3):
            assert np.array_equal(_bits(parity["after"][k][j]), _bits(parity["twin_after"][k][j])), (name, j)
            assert np.all(np.isfinite(parity["after"][k][j])), (name, j)
            if parity["ns"][k] > 1:
                assert not np.array_equal(_bits(parity["after"][k][j]), _bits(parity["before"][k][j])), (name, j)


# ---- 2. the public single re-factorisation ----
def test_refactor_on_the_public_surface():
    import ilupp_amd.device as ild
    A = _random(300, 530)
    A2 = _scaled(A, 61)
    dA, dA2 = _dev(A), _dev(A2)
    M = ild.DevicePreconditioner("ILU0", dA)
    assert M.refactor_(dA2) is M
    assert _same_factors(_factors(M), _factors(ild.DevicePreconditioner("ILU0", dA2)))
    with pytest.raises(ValueError, match="dimension"):
        M.refactor_(_dev(_random(257, 531)))
    with pytest.raises(NotImplementedError):
        ild.DevicePreconditioner("ILUT", dA).refactor_(dA2)


# ---- 3. no host wait is needed for correctness ----
def test_ordering_without_a_host_wait():
    """refactor_batch_(check=False) on a side stream behind a producer that writes A''s values, followed at once by apply_batch_ and
    cg_batch: the bits of the singles on the twins; two calls in a row with two value sets leave the second set's factors"""
    import torch
    import ilupp_amd.device as ild
    ns = [65, 257, 300, 256]
    mats = [_spd(n, 540 + k) for k, n in enumerate(ns[:3])] + [_csr(matgen.poisson2d(16))]
    A1 = [_scaled(A, 70 + k) for k, A in enumerate(mats)]
    A2 = [_scaled(A, 80 + k) for k, A in enumerate(mats)]
    for A in A1 + A2:                                                    # (scaled entry by entry: symmetric again, for CG)
        S = ((A + A.T) / 2).tocsr()
        S.sort_indices()
        A.data[:] = S.data
    dAs = [_dev(A) for A in mats]                                        # the buffers the producer writes into
    members = [_member(A, dA, k % 3) for k, (A, dA) in enumerate(zip(mats, dAs))]
    twins = [_member(A, dA, k % 3) for k, (A, dA) in enumerate(zip(mats, dAs))]
    d1, d2 = [_dev(A) for A in A1], [_dev(A) for A in A2]
    for T, dA in zip(twins, d2):
        _refactor_single(T, dA)
    offsets, total = [], 3
    for n in ns:
        offsets.append(total)
        total += n + 3
    host = np.zeros(total)
    for k, (o, n) in enumerate(zip(offsets, ns)):
        host[o:o + n] = _rhs(n, 50 + k)
    kw = dict(maxiter=6, rtol=0.0, check_every=0)
    want_apply = [_single(T).apply_(torch.from_numpy(host[o:o + n]).cuda()).cpu().numpy() for T, o, n in zip(twins, offsets, ns)]
    want_cg = [ild.cg(dA, torch.from_numpy(host[o:o + n]).cuda()[:, None], _single(T), **kw).cpu().numpy()[:, 0]
               for dA, T, o, n in zip(d2, twins, offsets, ns)]
    fresh2 = [_factors(ild.DevicePreconditioner("ILU0", dA)) for dA in d2]
    src1 = [torch.from_numpy(A.data.copy()).pin_memory() for A in A1]
    src2 = [torch.from_numpy(A.data.copy()).pin_memory() for A in A2]
    bsrc = torch.from_numpy(host).pin_memory()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for dA, s in zip(dAs, src1):
            dA.data.copy_(s, non_blocking=True)                          # the producer: no sync behind it
        r1, s1 = ild.refactor_batch_(members, dAs, check=False)
        keep = [dA.data.clone() for dA in dAs]
        for dA, s in zip(dAs, src2):
            dA.data.copy_(s, non_blocking=True)                          # (behind the first launch on this stream: it read the first set)
        r2, s2 = ild.refactor_batch_(members, dAs, check=False)
        x = torch.empty(total, dtype=torch.float64, device="cuda")
        x.copy_(bsrc, non_blocking=True)
        b = x.clone()
        ild.apply_batch_(members, x, offsets)
        y = ild.cg_batch(dAs, b, offsets, members, **kw)
    side.synchronize()
    assert r1 == [0] * 4 and r2 == [0] * 4
    assert s1.cpu().tolist() == [0] * 4 and s2.cpu().tolist() == [0] * 4
    for k, A in enumerate(A1):
        assert np.array_equal(_bits(keep[k].cpu().numpy()), _bits(A.data))
    xh, yh = x.cpu().numpy(), y.cpu().numpy()
    for k, (o, n) in enumerate(zip(offsets, ns)):
        assert np.array_equal(_bits(xh[o:o + n]), _bits(want_apply[k])), k
        assert np.array_equal(_bits(yh[o:o + n]), _bits(want_cg[k])), k
        assert _same_factors(_factors(members[k]), fresh2[k]), k
    ild._on_current_stream()


# ---- 4. a pattern that differs ----
def test_pattern_mismatch_leaves_the_member_unchanged():
    import torch
    import ilupp_amd.device as ild
    mats = [_random(65, 550 + k) for k in range(3)]
    dAs = [_dev(A) for A in mats]
    members = [_member(A, dA, k % 3) for k, (A, dA) in enumerate(zip(mats, dAs))]
    A2 = [_scaled(A, 90 + k) for k, A in enumerate(mats)]
    # member 1: the same n and nnz, one column index moved (the row stays sorted)
    B = A2[1].copy()
    moved = False
    for r in range(B.shape[0]):
        cols = B.indices[B.indptr[r]:B.indptr[r + 1]]
        for q, c in enumerate(cols):
            if c != r and c + 1 != r and c + 1 < B.shape[0] and c + 1 not in cols:
                B.indices[B.indptr[r] + q] = c + 1
                moved = True
                break
        if moved:
            break
    assert moved and B.nnz == mats[1].nnz and not np.array_equal(B.indices, mats[1].indices)
    bad = ild.DeviceCSR(torch.from_numpy(B.data.copy()).cuda(), torch.from_numpy(B.indices.astype(np.int32)).cuda(),
                        torch.from_numpy(B.indptr.astype(np.int32)).cuda())
    d2 = [_dev(A2[0]), bad, _dev(A2[2])]
    old = [_factors(M) for M in members]
    v = torch.from_numpy(_rhs(65, 7)).cuda()
    old_apply = _single(members[1]).apply_(v.clone()).cpu().numpy()
    routes, status = ild.refactor_batch_(members, d2, check=False)
    assert routes == [0, 0, 0]
    assert status.cpu().tolist() == [0, 1, 0]
    assert _same_factors(_factors(members[1]), old[1])
    assert np.array_equal(_bits(_single(members[1]).apply_(v.clone()).cpu().numpy()), _bits(old_apply))
    for k in (0, 2):
        assert _same_factors(_factors(members[k]), _factors(ild.DevicePreconditioner("ILU0", d2[k]))), k
    with pytest.raises(ValueError, match="member 1 of the batch"):
        ild.refactor_batch_(members, d2)
    assert _same_factors(_factors(members[1]), old[1])
    # a wrong nnz is refused before any launch: nobody's factor changes
    now = [_factors(M) for M in members]
    C = mats[1].copy()
    C.data[C.indptr[3]] = 0.0
    C.eliminate_zeros()
    assert C.nnz == mats[1].nnz - 1
    d3 = [dAs[0], _dev(C), dAs[2]]
    with pytest.raises(RuntimeError, match="member 1 of the batch: the matrix does not have the analysed pattern"):
        ild.refactor_batch_(members, d3)
    for k in range(3):
        assert _same_factors(_factors(members[k]), now[k]), k
    # a refusal that needs a built object: a member of another class
    with pytest.raises(TypeError, match="ILU0 kind only"):
        ild.refactor_batch_([ild.DevicePreconditioner("IChol0", _dev(_spd(65, 560)))], [dAs[0]])


# ---- 5. zero pivots and NaN: what the single call gives ----
def test_non_finite_values_match_the_single_call():
    import ilupp_amd.device as ild
    mats = [_random(65, 570 + k) for k in range(4)]
    dAs = [_dev(A) for A in mats]
    members = [_member(A, dA, k % 3) for k, (A, dA) in enumerate(zip(mats, dAs))]
    twins = [_member(A, dA, k % 3) for k, (A, dA) in enumerate(zip(mats, dAs))]
    A2 = [_scaled(A, 100 + k) for k, A in enumerate(mats)]
    A2[0].data[A2[0].indptr[0] + list(A2[0].indices[A2[0].indptr[0]:A2[0].indptr[1]]).index(0)] = 0.0      # a_00 = 0: a zero pivot
    A2[2].data[A2[2].indptr[20] + 1] = np.nan
    d2 = [ild.DeviceCSR.from_scipy(A) for A in A2]
    assert [d.nnz for d in d2] == [A.nnz for A in mats]                  # (the stored zero stays stored)
    routes, status = ild.refactor_batch_(members, d2, check=False)
    assert routes == [0] * 4 and status.cpu().tolist() == [0] * 4         # (neither is an error)
    for T, dA in zip(twins, d2):
        _refactor_single(T, dA)
    got = [_factors(M) for M in members]
    for k in range(4):
        assert _same_factors(got[k], _factors(twins[k])), k
    assert not np.all(np.isfinite(got[0][1][0])) and not np.all(np.isfinite(got[2][1][0]))
    for k in (1, 3):                                                      # the clean neighbours
        assert np.all(np.isfinite(got[k][0][0])) and np.all(np.isfinite(got[k][1][0]))
        assert _same_factors(got[k], _factors(ild.DevicePreconditioner("ILU0", d2[k]))), k


# ---- 6. more workgroups than CUs ----
def test_many_members():
    """300 members of n = 40, built from A': re-factorised with A (the factors change), then with A' again (the construction's bits)"""
    import ilupp_amd.device as ild
    mats = [_random(40, 600 + k) for k in range(300)]
    d1 = [_dev(A) for A in mats]
    d2 = [_dev(_scaled(A, 700 + k)) for k, A in enumerate(mats)]
    members = [ild.DevicePreconditioner("ILU0", dA) for dA in d2]
    built = [_factors(M) for M in members]
    assert ild.refactor_batch_(members, d1) == [0] * 300
    mid = [_factors(M) for M in members]
    assert not any(_same_factors(a, b) for a, b in zip(mid, built))
    assert _same_factors(mid[299], _factors(ild.DevicePreconditioner("ILU0", d1[299])))
    assert ild.refactor_batch_(members, d2) == [0] * 300
    for k, M in enumerate(members):
        assert _same_factors(_factors(M), built[k]), k


# ---- 7. the cap ----
def test_cap_routes_large_members_to_the_single_path(monkeypatch):
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    assert _native.ilu0_refactor_batch_max_n() >= 4000
    monkeypatch.setenv("ILUPP_BATCH_APPLY_MAX_N", "600")
    assert _native.ilu0_refactor_batch_max_n() == 600
    mats = [_random(700, 580), _random(513, 581)]
    dAs = [_dev(A) for A in mats]
    members = [ild.DevicePreconditioner("ILU0", dA) for dA in dAs]
    twins = [ild.DevicePreconditioner("ILU0", dA) for dA in dAs]
    d2 = [_dev(_scaled(A, 110 + k)) for k, A in enumerate(mats)]
    routes, status = ild.refactor_batch_(members, d2, check=False)
    assert routes == [1, 0] and status.cpu().tolist() == [0, 0]
    for k, (T, dA) in enumerate(zip(twins, d2)):
        _refactor_single(T, dA)
        assert _same_factors(_factors(members[k]), _factors(T)), k
        for a, b in zip(_three_applies(members[k], mats[k].shape[0], k), _three_applies(T, mats[k].shape[0], k)):
            assert np.array_equal(_bits(a), _bits(b)), k


def _band(n, half, wide_row=None):
    """a banded matrix, `half` entries on either side of the diagonal (row `wide_row`: one more on either side), diagonally dominant"""
    rng = np.random.default_rng(91)
    A = sp.lil_matrix((n, n))
    for i in range(n):
        h = half + (1 if i == wide_row else 0)
        for j in range(max(0, i - h), min(n, i + h + 1)):
            A[i, j] = 3.0 * n + rng.random() if i == j else rng.random()
    A = A.tocsr()
    A.sort_indices()
    return A


def test_row_cap_routes_long_rows_to_the_single_path():
    """the launch keeps a lane's working row in LDS: a longest row of 31 entries is the most it takes (route 0), one row of 33 sends the
    member to the single path (route 1); both have the twin's bits, and the rows of the band depend on each other"""
    import ilupp_amd.device as ild
    mats = [_band(96, 15), _band(96, 15, wide_row=40)]
    assert [int(np.diff(A.indptr).max()) for A in mats] == [31, 33]
    dAs = [_dev(A) for A in mats]
    members = [ild.DevicePreconditioner("ILU0", dA) for dA in dAs]
    twins = [ild.DevicePreconditioner("ILU0", dA) for dA in dAs]
    d2 = [_dev(_scaled(A, 130 + k)) for k, A in enumerate(mats)]
    routes, status = ild.refactor_batch_(members, d2, check=False)
    assert routes == [0, 1] and status.cpu().tolist() == [0, 0]
    for k, (T, dA) in enumerate(zip(twins, d2)):
        _refactor_single(T, dA)
        assert _same_factors(_factors(members[k]), _factors(T)), k
        assert _same_factors(_factors(members[k]), _factors(ild.DevicePreconditioner("ILU0", dA))), k


# ---- 8. speed ----
def test_batched_call_beats_the_loop_at_16_members():
    """16 members of n = 4 000: the median of five batched calls (host clock around the call plus a device synchronisation, after two
    warm-up calls) is below the median of the loop of single re-factorisations over the same objects"""
    import torch
    import ilupp_amd.device as ild
    mats = [_random(4000, 900 + k) for k in range(16)]
    dAs = [_dev(A) for A in mats]
    d2 = [_dev(_scaled(A, 120 + k)) for k, A in enumerate(mats)]
    members = [ild.DevicePreconditioner("ILU0", dA) for dA in dAs]
    ild._on_current_stream()

    def batched():
        ild.refactor_batch_(members, d2, check=False)

    def looped():
        for M, dA in zip(members, d2):
            M.pr.refactor_device(dA.data.data_ptr(), dA.indices.data_ptr(), dA.indptr.data_ptr())

    def median(fn):
        ts = []
        for it in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts[2:])) * 1e3

    t_loop = median(looped)
    t_batch = median(batched)
    print("16 members of n = 4000: batched %.3f ms, looped %.3f ms (%.1f x)" % (t_batch, t_loop, t_loop / t_batch))
    assert t_batch < t_loop
