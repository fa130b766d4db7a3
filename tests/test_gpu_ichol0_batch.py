"""GPU tests of IChol(0) for many small SPD systems: the batched first construction (ilupp_amd.device.ichol0_batch over
ilupp_hip_ichol0_create_batch_device: k_ichol0_symbolic_batch, k_ichol0_create_batch), the batched re-factorisation
(ichol0_refactor_batch_ over ilupp_hip_ichol0_refactor_batch_device: one launch of k_ichol0_refactor_batch, one workgroup per member) and the
single re-factorisation ichol0_refactor_.  Every comparison is bitwise on int64 views.  The reference for the FACTORS is a freshly
constructed DevicePreconditioner("IChol0", A') (factor_copy of L: pointers and indices equal, values bit-equal); the reference for
BEHAVIOUR is a twin object, built alone and re-factorised by the single ichol0_refactor_.  A' is A scaled entry by entry with 1 + 0.1 u,
u uniform in [0, 1) from a fixed seed, and then made symmetric again ((A' + A'^T) / 2 on the same pattern)."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import matgen

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 65, 256, 257, 300, 513]          # one row; two; a wave and one; the workgroup's 256 lanes, one more (a second round); odd sizes
LONGEST = [1, 2, 20, 25, 21, 24, 22]            # the longest row of L of _spd(n, 500 + k)


def _csr(t):
    d, i, p = t
    n = p.shape[0] - 1
    A = sp.csr_matrix((np.asarray(d, dtype=np.float64), i, p), shape=(n, n))
    A.sort_indices()
    return A


def _spd(n, seed):
    return _csr(matgen.symmetrize(*matgen.random_dd(n, 8, 25.0, seed)))


def _arrow(n, full):
    """diagonal plus a full row and column `full`, symmetric and diagonally dominant"""
    rng = np.random.default_rng(77)
    A = sp.lil_matrix((n, n))
    A.setdiag(25.0 + rng.random(n))
    for j in range(n):
        if j != full:
            A[full, j] = A[j, full] = 0.01 + 0.01 * rng.random()
    A = A.tocsr()
    A.sort_indices()
    return A


def _scaled(A, seed):
    """A': the same pattern, every value scaled by 1 + 0.1 u, symmetric again"""
    B = A.copy()
    B.data = A.data * (1.0 + 0.1 * np.random.default_rng(seed).random(A.data.shape[0]))
    S = ((B + B.T) / 2).tocsr()
    S.sort_indices()
    assert np.array_equal(S.indices, A.indices) and np.array_equal(S.indptr, A.indptr)
    B.data[:] = S.data
    return B


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _dev(A):
    import ilupp_amd.device as ild
    return ild.DeviceCSR.from_scipy(A)


def _dev_raw(A):
    """the arrays as they are (no sorting, no checks)"""
    import torch
    import ilupp_amd.device as ild
    return ild.DeviceCSR(torch.from_numpy(A.data.astype(np.float64)).cuda(), torch.from_numpy(A.indices.astype(np.int32)).cuda(),
                         torch.from_numpy(A.indptr.astype(np.int32)).cuda())


def _fresh(dA):
    import ilupp_amd.device as ild
    return ild.DevicePreconditioner("IChol0", dA)


def _member(A, dA, how):
    """one IChol0 member three ways: 0 = a DevicePreconditioner, 1 = the host class of the ctypes binding itself, 2 = a FactorOperator of it"""
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    if how == 0:
        return _fresh(dA)
    P = ilupp.IChol0Preconditioner(A)
    return P if how == 1 else ild.FactorOperator(P)


def _single(M):
    import ilupp_amd.device as ild
    return M if hasattr(M, "apply_") else ild.FactorOperator(M)


def _factors(M):
    """[L] as (data, indices, indptr) triples from factor_copy"""
    return [(f[0], f[1], f[2]) for f in M.pr.factors_info()]


def _same_factors(F, G):
    return len(F) == len(G) == 1 and all(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(_bits(a[0]), _bits(b[0]))
                                         for a, b in zip(F, G))


def _rhs(n, seed=0):
    return np.random.default_rng(2000 + seed).standard_normal(n) + 2.0


def _three_applies(M, n, seed):
    """apply_ in both directions and a block apply_ of k = 3, on clones: the host copies"""
    import torch
    S = _single(M)
    v = torch.from_numpy(_rhs(n, seed)).cuda()
    X = torch.from_numpy(np.random.default_rng(3000 + seed).standard_normal((n, 3)) + 2.0).cuda().contiguous()
    return [S.apply_(v.clone()).cpu().numpy(), S.apply_(v.clone(), transpose=True).cpu().numpy(), S.apply_(X.clone()).cpu().numpy()]


def _same_applies(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _build_with_routes(dAs):
    """ichol0_batch through the native entry, which hands the routes out"""
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    ild._on_current_stream()
    routes = []
    natives = _native.IChol0Preconditioner_batch_device([(A.data.data_ptr(), A.indices.data_ptr(), A.indptr.data_ptr(), A.n, A.nnz) for A in dAs],
                                                        True, routes)
    return natives, routes


def _packed(ns, seed):
    offsets, total = [], 3
    for n in ns:
        offsets.append(total)
        total += n + 3
    host = np.zeros(total)
    for k, (o, n) in enumerate(zip(offsets, ns)):
        host[o:o + n] = _rhs(n, seed + k)
    return offsets, host


# ---- 1. parity and routes: one batch of every kind of member, for construction and for re-factorisation ----
def _parity_matrices():
    mats = [("spd(%d)" % n, _spd(n, 500 + k)) for k, n in enumerate(SIZES)]
    mats.append(("laplace1d(300)", _csr(matgen.laplace1d(300))))          # every row waits for the one before: the longest chain
    mats.append(("poisson2d(16)", _csr(matgen.poisson2d(16))))
    mats.append(("diagonal(65)", sp.diags(25.0 + np.arange(65.0)).tocsr()))            # no row has a lower entry
    mats.append(("arrow_first(300)", _arrow(300, 0)))                     # rows of L of two entries, row 0 of LcT of 300: the binary search
    mats.append(("arrow_last(300)", _arrow(300, 299)))                    # a row of L as long as n: above the row cap, route 1
    return mats


@pytest.fixture(scope="module")
def parity():
    import ilupp_amd.device as ild
    mats = _parity_matrices()
    out = dict(names=[m[0] for m in mats], ns=[m[1].shape[0] for m in mats])
    As = [m[1] for m in mats]
    out["longest"] = [int(np.diff(sp.tril(A).tocsr().indptr).max()) for A in As]
    A2 = [_scaled(A, 40 + k) for k, A in enumerate(As)]
    dAs, dA2 = [_dev(A) for A in As], [_dev(A) for A in A2]
    out["create_routes"] = _build_with_routes(dAs)[1]
    members = ild.ichol0_batch(dAs)
    twins = [_fresh(dA) for dA in dAs]
    out["kinds"] = [M.kind for M in members]
    out["paths"] = [M.pr.path() for M in members]
    out["twin_paths"] = [T.pr.path() for T in twins]
    out["nnz"] = [(M.pr.total_nnz, T.pr.total_nnz, sp.tril(A).nnz) for M, T, A in zip(members, twins, As)]
    out["built"] = [_factors(M) for M in members]
    out["twin_built"] = [_factors(T) for T in twins]
    out["before"] = [_three_applies(M, n, k) for k, (M, n) in enumerate(zip(members, out["ns"]))]
    out["twin_before"] = [_three_applies(T, n, k) for k, (T, n) in enumerate(zip(twins, out["ns"]))]
    out["routes"] = ild.ichol0_refactor_batch_(members, dA2)
    out["got"] = [_factors(M) for M in members]
    out["paths_after"] = [M.pr.path() for M in members]
    out["after"] = [_three_applies(M, n, k) for k, (M, n) in enumerate(zip(members, out["ns"]))]
    out["fresh"] = [_factors(_fresh(dA)) for dA in dA2]
    for T, dA in zip(twins, dA2):
        assert ild.ichol0_refactor_(T, dA) is T
    out["twin"] = [_factors(T) for T in twins]
    out["twin_after"] = [_three_applies(T, n, k) for k, (T, n) in enumerate(zip(twins, out["ns"]))]
    return out


def test_the_matrices_are_what_the_cases_say(parity):
    assert parity["longest"][:len(SIZES)] == LONGEST
    assert parity["longest"][parity["names"].index("arrow_first(300)")] == 2
    assert parity["longest"][parity["names"].index("arrow_last(300)")] == 300


def test_construction_equals_the_single_constructor(parity):
    print("construction: %s" % list(zip(parity["names"], parity["paths"], parity["create_routes"])))
    for k, name in enumerate(parity["names"]):
        want = 1 if name == "arrow_last(300)" else 0
        assert parity["create_routes"][k] == want, name
        assert parity["kinds"][k] == "IChol0"
        assert (parity["paths"][k] == "ichol0:batch") == (want == 0), (name, parity["paths"][k])
        if want == 1:
            assert parity["paths"][k] == parity["twin_paths"][k], name
        assert _same_factors(parity["built"][k], parity["twin_built"][k]), name
        assert parity["nnz"][k][0] == parity["nnz"][k][1] == parity["nnz"][k][2], name
        assert _same_applies(parity["before"][k], parity["twin_before"][k]), name
        assert all(np.all(np.isfinite(x)) for x in parity["before"][k]), name


def test_refactored_factors_equal_a_fresh_construction(parity):
    print("re-factorisation: %s" % list(zip(parity["names"], parity["paths"], parity["routes"])))
    for k, name in enumerate(parity["names"]):
        path = parity["paths"][k]
        assert parity["routes"][k] == (0 if path == "ichol0:batch" else 2 if "static" in path else 1), (name, path)
        assert parity["paths_after"][k] == path, name
        assert _same_factors(parity["got"][k], parity["fresh"][k]), name
        assert _same_factors(parity["got"][k], parity["twin"][k]), name
        assert not _same_factors(parity["got"][k], parity["built"][k]), name          # (the values did change)
    assert parity["routes"][parity["names"].index("arrow_last(300)")] != 0


def test_applies_after_the_call_equal_the_twins(parity):
    """apply_ in both directions and a block apply_ of k = 3: every member had run all three BEFORE the call and has the twin's bits afterwards"""
    for k, name in enumerate(parity["names"]):
        assert _same_applies(parity["after"][k], parity["twin_after"][k]), name
        if not name.startswith(("laplace", "poisson")):                   # (scaled entry by entry these two need not stay positive definite)
            assert all(np.all(np.isfinite(x)) for x in parity["after"][k]), name
        assert not _same_applies(parity["after"][k], parity["before"][k]), name


# ---- 2. the transposed copy stays current, and no host wait is needed for correctness ----
@pytest.mark.parametrize("warm, forms", [(True, False), (False, False), (True, True)])
def test_transposed_copy_stays_current_without_a_host_wait(warm, forms):
    """warm: one cg_batch before the re-factorisations builds LcT, which every launch then rewrites; cold: no LcT exists when the
    re-factorisations run, the batched apply behind them builds it from the new factor.  forms: members built alone, in the three forms"""
    import torch
    import ilupp_amd.device as ild
    ns = [65, 257, 300, 256]
    mats = [_spd(n, 540 + k) for k, n in enumerate(ns[:3])] + [_csr(matgen.poisson2d(16))]
    A1 = [_scaled(A, 70 + k) for k, A in enumerate(mats)]
    A2 = [_scaled(A, 80 + k) for k, A in enumerate(mats)]
    dAs = [_dev(A) for A in mats]                                        # the buffers the producer writes into
    members = [_member(A, dA, k % 3) for k, (A, dA) in enumerate(zip(mats, dAs))] if forms else ild.ichol0_batch(dAs)
    twins = [_fresh(dA) for dA in dAs]
    d2 = [_dev(A) for A in A2]
    for T, dA in zip(twins, d2):
        ild.ichol0_refactor_(T, dA)
    offsets, host = _packed(ns, 50)
    total = host.shape[0]
    kw = dict(maxiter=6, rtol=0.0, check_every=0)
    want_apply = [_single(T).apply_(torch.from_numpy(host[o:o + n]).cuda()).cpu().numpy() for T, o, n in zip(twins, offsets, ns)]
    want_cg = [ild.cg(dA, torch.from_numpy(host[o:o + n]).cuda()[:, None], _single(T), **kw).cpu().numpy()[:, 0]
               for dA, T, o, n in zip(d2, twins, offsets, ns)]
    fresh2 = [_factors(_fresh(dA)) for dA in d2]
    paths = [(M.pr if hasattr(M, "pr") else M).path() for M in members]
    if warm:
        ild.cg_batch(dAs, torch.from_numpy(host).cuda(), offsets, members, **kw)
    src1 = [torch.from_numpy(A.data.copy()).pin_memory() for A in A1]
    src2 = [torch.from_numpy(A.data.copy()).pin_memory() for A in A2]
    bsrc = torch.from_numpy(host).pin_memory()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for dA, s in zip(dAs, src1):
            dA.data.copy_(s, non_blocking=True)                          # the producer: no sync behind it
        r1, s1 = ild.ichol0_refactor_batch_(members, dAs, check=False)
        keep = [dA.data.clone() for dA in dAs]
        for dA, s in zip(dAs, src2):
            dA.data.copy_(s, non_blocking=True)                          # (behind the first launch on this stream: it read the first set)
        r2, s2 = ild.ichol0_refactor_batch_(members, dAs, check=False)
        x = torch.empty(total, dtype=torch.float64, device="cuda")
        x.copy_(bsrc, non_blocking=True)
        b = x.clone()
        ild.apply_batch_(members, x, offsets)
        y = ild.cg_batch(dAs, b, offsets, members, **kw)
    side.synchronize()
    want_routes = [0 if p == "ichol0:batch" else 2 if "static" in p else 0 for p in paths]
    print("warm %s forms %s: paths %s routes %s" % (warm, forms, paths, r2))
    assert r1 == want_routes and r2 == want_routes
    assert s1.cpu().tolist() == [0] * 4 and s2.cpu().tolist() == [0] * 4
    for k, A in enumerate(A1):
        assert np.array_equal(_bits(keep[k].cpu().numpy()), _bits(A.data))
    xh, yh = x.cpu().numpy(), y.cpu().numpy()
    for k, (o, n) in enumerate(zip(offsets, ns)):
        assert np.array_equal(_bits(xh[o:o + n]), _bits(want_apply[k])), k
        assert np.array_equal(_bits(yh[o:o + n]), _bits(want_cg[k])), k
        assert _same_factors(_factors(_single(members[k])), fresh2[k]), k
    ild._on_current_stream()


# ---- 3. stale copies: packed, transposed and level-ordered copies of the OLD values exist before the call ----
def test_stale_copies_of_the_old_values_go():
    import ilupp_amd.device as ild
    mats = [_spd(1100, 520), _spd(300, 521), _spd(1100, 522), _spd(257, 523)]          # (n >= 1024 with long rows: the level-ordered sweeps)
    dAs = [_dev(A) for A in mats]
    members = ild.ichol0_batch(dAs[:2]) + [_fresh(dAs[2]), _fresh(dAs[3])]
    twins = [_fresh(dA) for dA in dAs]
    d2 = [_dev(_scaled(A, 60 + k)) for k, A in enumerate(mats)]
    before = [_three_applies(M, A.shape[0], k) for k, (M, A) in enumerate(zip(members, mats))]
    old = [_factors(M) for M in members]
    routes = ild.ichol0_refactor_batch_(members, d2)
    assert routes == [0] * 4
    for k, (M, T, A) in enumerate(zip(members, twins, mats)):
        ild.ichol0_refactor_(T, d2[k])
        assert _same_factors(_factors(M), _factors(T)), k
        assert not _same_factors(_factors(M), old[k]), k
        after = _three_applies(M, A.shape[0], k)
        assert _same_applies(after, _three_applies(T, A.shape[0], k)), k
        assert not _same_applies(after, before[k]), k


# ---- 4. a pattern that differs ----
def _move(B, r, old, new):
    """row r of B: the entry of column `old` becomes one of column `new` (not stored yet); the row sorted again, the values kept in place"""
    a, b = B.indptr[r], B.indptr[r + 1]
    cols = list(B.indices[a:b])
    assert old in cols and new not in cols
    cols[cols.index(old)] = new
    B.indices[a:b] = sorted(cols)


def _pick(A, pred):
    """the first (row, stored column, free column) with pred(r, stored, free)"""
    n = A.shape[0]
    for r in range(2, n - 2):
        cols = set(A.indices[A.indptr[r]:A.indptr[r + 1]])
        for c in sorted(cols):
            for f in range(n):
                if f not in cols and pred(r, c, f):
                    return r, c, f
    raise AssertionError("no such entry")


def test_pattern_mismatch_leaves_the_member_unchanged():
    import torch
    import ilupp_amd.device as ild
    n = 65
    mats = [_spd(n, 550 + k) for k in range(5)]
    dAs = [_dev(A) for A in mats]
    members = ild.ichol0_batch(dAs)
    offsets, host = _packed([n] * 5, 20)
    kw = dict(maxiter=5, rtol=0.0, check_every=0)
    b = torch.from_numpy(host).cuda()
    y_old = ild.cg_batch(dAs, b, offsets, members, **kw).cpu().numpy()   # (builds the transposed copies)
    A2 = [_scaled(A, 90 + k) for k, A in enumerate(mats)]
    # member 0: as analysed.  1: one lower column moved, as many entries.  2: one lower entry more (an upper one fewer).  3: one lower
    # entry fewer (an upper one more).  4: differs only above the diagonal
    _move(A2[1], *_pick(A2[1], lambda r, c, f: c < r and f < r))
    _move(A2[2], *_pick(A2[2], lambda r, c, f: c > r and f < r))
    _move(A2[3], *_pick(A2[3], lambda r, c, f: c < r and f > r))
    _move(A2[4], *_pick(A2[4], lambda r, c, f: c > r and f > r))
    for k in range(1, 5):
        assert A2[k].nnz == mats[k].nnz and not np.array_equal(A2[k].indices, mats[k].indices)
    assert [sp.tril(A2[k]).nnz - sp.tril(mats[k]).nnz for k in range(5)] == [0, 0, 1, -1, 0]
    d2 = [_dev_raw(A) for A in A2]
    old = [_factors(M) for M in members]
    routes, status = ild.ichol0_refactor_batch_(members, d2, check=False)
    assert routes == [0] * 5
    assert status.cpu().tolist() == [0, 1, 1, 1, 0]
    y_new = ild.cg_batch(dAs, b, offsets, members, **kw).cpu().numpy()
    for k in (1, 2, 3):
        assert _same_factors(_factors(members[k]), old[k]), k
        o = offsets[k]
        assert np.array_equal(_bits(y_new[o:o + n]), _bits(y_old[o:o + n])), k
    for k in (0, 4):                                                      # (4: the factor of its lower triangle)
        assert _same_factors(_factors(members[k]), _factors(_fresh(d2[k]))), k
        o = offsets[k]
        assert not np.array_equal(_bits(y_new[o:o + n]), _bits(y_old[o:o + n])), k
        T = _fresh(d2[k])
        want = ild.cg(dAs[k], b[o:o + n].clone()[:, None], T, **kw).cpu().numpy()[:, 0]
        assert np.array_equal(_bits(y_new[o:o + n]), _bits(want)), k
    with pytest.raises(ValueError, match="member 1 of the batch"):
        ild.ichol0_refactor_batch_(members, d2)
    for k in (1, 2, 3):
        assert _same_factors(_factors(members[k]), old[k]), k
    # the single re-factorisation refuses the same matrices and leaves the factor as it was (a batch-built and a singly built object)
    T = _fresh(dAs[2])
    t_old = _factors(T)
    for M, keep in ((members[2], old[2]), (T, t_old)):
        with pytest.raises(RuntimeError, match="IChol0 refactor: the matrix does not have the analysed pattern|the matrix does not have the analysed pattern"):
            ild.ichol0_refactor_(M, d2[2])
        assert _same_factors(_factors(M), keep)
    # a wrong number of stored entries is refused before any launch: nobody's factor changes
    now = [_factors(M) for M in members]
    C = mats[1].copy()
    C.data[C.indptr[3]] = 0.0
    C.eliminate_zeros()
    assert C.nnz == mats[1].nnz - 1
    with pytest.raises(RuntimeError, match="member 1 of the batch: the matrix does not have the analysed pattern"):
        ild.ichol0_refactor_batch_(members, [dAs[0], _dev(C)] + dAs[2:])
    for k in range(5):
        assert _same_factors(_factors(members[k]), now[k]), k
    # a refusal that needs a built object: a member of another class
    with pytest.raises(TypeError, match="IChol0 kind only"):
        ild.ichol0_refactor_batch_([ild.DevicePreconditioner("ILU0", dAs[0])], [dAs[0]])


# ---- 5. negative and zero pivots: what the single constructor and the single re-factorisation give ----
def test_non_finite_values_match_the_single_calls():
    import ilupp_amd.device as ild
    n = 65
    mats = [_spd(n, 570 + k) for k in range(4)]
    A2 = [_scaled(A, 100 + k) for k, A in enumerate(mats)]
    for A, v in ((A2[0], -3.0), (A2[2], 0.0)):                            # a negative and a zero diagonal in row n / 2
        r = n // 2
        A.data[A.indptr[r] + list(A.indices[A.indptr[r]:A.indptr[r + 1]]).index(r)] = v
    d1, d2 = [_dev(A) for A in mats], [_dev(A) for A in A2]
    assert [d.nnz for d in d2] == [A.nnz for A in mats]                  # (the stored zero stays stored)
    # through the batched construction
    built = ild.ichol0_batch(d2)
    single = [_fresh(dA) for dA in d2]
    for k in range(4):
        assert built[k].pr.path() == "ichol0:batch"
        assert _same_factors(_factors(built[k]), _factors(single[k])), k
    # through the batched re-factorisation, against the single one on twins
    members, twins = ild.ichol0_batch(d1), [_fresh(dA) for dA in d1]
    routes, status = ild.ichol0_refactor_batch_(members, d2, check=False)
    assert routes == [0] * 4 and status.cpu().tolist() == [0] * 4         # (neither is an error)
    for T, dA in zip(twins, d2):
        ild.ichol0_refactor_(T, dA)
    got = [_factors(M) for M in members]
    for k in range(4):
        assert _same_factors(got[k], _factors(twins[k])), k
        assert _same_factors(got[k], _factors(single[k])), k
    assert not np.all(np.isfinite(got[0][0][0])) and not np.all(np.isfinite(got[2][0][0]))
    for k in (1, 3):                                                      # the clean neighbours
        assert np.all(np.isfinite(got[k][0][0])), k


# ---- 6. construction failures ----
def test_construction_failures():
    import ilupp_amd.device as ild
    mats = [_spd(65, 590 + k) for k in range(3)]
    B = mats[1].copy()
    B.data[B.indptr[3] + list(B.indices[B.indptr[3]:B.indptr[4]]).index(3)] = 0.0
    B.eliminate_zeros()                                                   # no diagonal entry in row 3
    with pytest.raises(RuntimeError, match="matrix 1 of the batch: IChol0: structurally missing diagonal entry in row 3"):
        ild.ichol0_batch([_dev(mats[0]), _dev(B), _dev(mats[2])])
    # an unsorted row (two lower entries swapped, the diagonal still behind them): the single constructor inside the call
    C = mats[1].copy()
    r = next(r for r in range(65) if np.sum(C.indices[C.indptr[r]:C.indptr[r + 1]] < r) >= 2)
    a = C.indptr[r]
    C.indices[[a, a + 1]] = C.indices[[a + 1, a]]
    C.data[[a, a + 1]] = C.data[[a + 1, a]]
    dC = [_dev(mats[0]), _dev_raw(C), _dev(mats[2])]
    natives, routes = _build_with_routes(dC)
    assert routes == [0, 1, 0]
    assert [p.path() == "ichol0:batch" for p in natives] == [True, False, True]
    for pr, dA in zip(natives, dC):
        T = _fresh(dA)
        assert all(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(_bits(a[0]), _bits(b[0]))
                   for a, b in zip(pr.factors_info(), T.pr.factors_info()))


# ---- 7. the caps ----
def test_caps_and_single_members(monkeypatch):
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    assert _native.ichol0_refactor_batch_max_n() >= 4000
    mats = [_spd(700, 580), _spd(513, 581)]
    dAs = [_dev(A) for A in mats]
    d2 = [_dev(_scaled(A, 110 + k)) for k, A in enumerate(mats)]
    # a batch of one is the single constructor's object
    one = ild.ichol0_batch([dAs[1]])
    assert len(one) == 1 and one[0].pr.path() == _fresh(dAs[1]).pr.path() != "ichol0:batch"
    assert _same_factors(_factors(one[0]), _factors(_fresh(dAs[1])))
    # the single re-factorisation of a batch-built member
    both = ild.ichol0_batch(dAs)
    assert [M.pr.path() for M in both] == ["ichol0:batch"] * 2
    assert ild.ichol0_refactor_(both[0], d2[0]) is both[0]
    assert both[0].pr.path() == "ichol0:batch"
    assert _same_factors(_factors(both[0]), _factors(_fresh(d2[0])))
    assert _same_applies(_three_applies(both[0], 700, 1), _three_applies(_fresh(d2[0]), 700, 1))
    with pytest.raises(ValueError, match="dimension"):
        ild.ichol0_refactor_(both[0], d2[1])
    # the n cap
    monkeypatch.setenv("ILUPP_BATCH_APPLY_MAX_N", "600")
    assert _native.ichol0_refactor_batch_max_n() == 600
    natives, routes = _build_with_routes(dAs)
    assert routes == [1, 0] and natives[0].path() != "ichol0:batch" and natives[1].path() == "ichol0:batch"
    members = ild.ichol0_batch(dAs)
    twins = [_fresh(dA) for dA in dAs]
    for M, T in zip(members, twins):
        assert _same_factors(_factors(M), _factors(T))
    routes, status = ild.ichol0_refactor_batch_(members, d2, check=False)
    assert routes == [2 if "static" in members[0].pr.path() else 1, 0] and status.cpu().tolist() == [0, 0]
    for k, (T, dA) in enumerate(zip(twins, d2)):
        ild.ichol0_refactor_(T, dA)
        assert _same_factors(_factors(members[k]), _factors(T)), k
        assert _same_applies(_three_applies(members[k], mats[k].shape[0], k), _three_applies(T, mats[k].shape[0], k)), k


def test_static_member_takes_the_single_path():
    """an object whose constructor ran the static form (a 7-point mesh) is re-factorised by the single path inside the batched call, route 2;
    its neighbours by the launch"""
    import ilupp_amd.device as ild
    d, i, p = matgen.poisson3d(8)
    rng = np.random.default_rng(7)
    D = sp.diags(1.0 + 0.5 * rng.random(512))
    mesh = (D @ sp.csr_matrix((d, i, p), shape=(512, 512)) @ D).tocsr()       # (a symmetric scaling keeps it positive definite)
    mesh.sort_indices()
    D2 = sp.diags(1.0 + 0.5 * rng.random(512))
    mesh2 = (D2 @ mesh @ D2).tocsr()
    mesh2.sort_indices()
    mats = [mesh, _spd(65, 585), _spd(257, 586)]
    A2 = [mesh2, _scaled(mats[1], 115), _scaled(mats[2], 116)]
    dAs, d2 = [_dev(A) for A in mats], [_dev(A) for A in A2]
    members, twins = [_fresh(dA) for dA in dAs], [_fresh(dA) for dA in dAs]
    assert members[0].pr.path() == "ichol0:static-level-major"
    before = _three_applies(members[0], 512, 3)
    routes, status = ild.ichol0_refactor_batch_(members, d2, check=False)
    assert routes == [2, 0, 0] and status.cpu().tolist() == [0, 0, 0]
    for k, (M, T) in enumerate(zip(members, twins)):
        ild.ichol0_refactor_(T, d2[k])
        assert _same_factors(_factors(M), _factors(T)), k
        assert _same_factors(_factors(M), _factors(_fresh(d2[k]))), k
        n = mats[k].shape[0]
        assert _same_applies(_three_applies(M, n, k), _three_applies(_fresh(d2[k]), n, k)), k
    assert not _same_applies(_three_applies(members[0], 512, 3), before)
    assert members[0].pr.path() == "ichol0:static-level-major"


# ---- 8. many members ----
def test_64_members():
    import ilupp_amd.device as ild
    mats = [_spd(65, 600 + k) for k in range(64)]
    d1 = [_dev(A) for A in mats]
    d2 = [_dev(_scaled(A, 700 + k)) for k, A in enumerate(mats)]
    natives, routes = _build_with_routes(d1)
    assert routes == [0] * 64
    members = ild.ichol0_batch(d1)
    for k, M in enumerate(members):
        assert _same_factors(_factors(M), _factors(_fresh(d1[k]))), k
        assert _same_factors(_factors(M), [(f[0], f[1], f[2]) for f in natives[k].factors_info()]), k
    assert ild.ichol0_refactor_batch_(members, d2) == [0] * 64
    for k, M in enumerate(members):
        assert _same_factors(_factors(M), _factors(_fresh(d2[k]))), k


# ---- 9. speed ----
def test_batched_calls_beat_the_loops_at_16_members():
    """16 members of n = 4 000 (longest row of L: 26, which fits with 20 bytes of LDS per working entry and lane): the median of five
    batched calls (host clock around the call plus a device synchronisation, after two warm-up calls) is below the median of the loop of
    single calls over the same objects -- for the re-factorisation and for the construction"""
    import torch
    import ilupp_amd.device as ild
    mats = [_spd(4000, 900 + k) for k in range(16)]
    assert int(np.diff(sp.tril(mats[0]).tocsr().indptr).max()) == 26
    dAs = [_dev(A) for A in mats]
    d2 = [_dev(_scaled(A, 120 + k)) for k, A in enumerate(mats)]
    natives, routes = _build_with_routes(dAs)
    assert routes == [0] * 16
    del natives
    members = ild.ichol0_batch(dAs)
    singles = [_fresh(dA) for dA in dAs]
    r, s = ild.ichol0_refactor_batch_(members, d2, check=False)
    assert r == [0] * 16 and s.cpu().tolist() == [0] * 16
    ild._on_current_stream()

    def median(fn):
        ts = []
        for it in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts[2:])) * 1e3

    def looped_refactor():
        for M, dA in zip(singles, d2):
            ild.ichol0_refactor_(M, dA)

    t_loop = median(looped_refactor)
    t_batch = median(lambda: ild.ichol0_refactor_batch_(members, d2, check=False))
    print("16 members of n = 4000, re-factorisation: batched %.3f ms, looped %.3f ms (%.1f x)" % (t_batch, t_loop, t_loop / t_batch))
    assert t_batch < t_loop
    c_loop = median(lambda: [_fresh(dA) for dA in dAs])
    c_batch = median(lambda: ild.ichol0_batch(dAs))
    print("16 members of n = 4000, construction: batched %.3f ms, looped %.3f ms (%.1f x)" % (c_batch, c_loop, c_loop / c_batch))
    assert c_batch < c_loop
