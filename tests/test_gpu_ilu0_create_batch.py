"""GPU tests of the batched FIRST construction of ILU(0) members (ilupp_amd.ILU0Preconditioner.batch over ilupp_hip_ilu0_create_batch,
ilupp_amd.device.DevicePreconditioner.batch over ilupp_hip_ilu0_create_batch_device: a symbolic launch, one read-back and a create launch,
one workgroup per member).  Every comparison is bitwise on int64 views; the reference is the object the single constructor builds from the
same matrix -- ILU0Preconditioner(A) for the host class, DevicePreconditioner("ILU0", dA) for the device class.  The shapes are the ones
tests/test_gpu_refactor_batch.py runs at routes 0 and 1 (the two launches share the re-factorisation's caps)."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import matgen

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 65, 256, 257, 300, 513]          # one row; two; a wave and one; the 256 lanes, one more (the scan's carry); odd sizes
BATCH = "ilu0:batch"


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


def _single(M):
    import ilupp_amd.device as ild
    return M if hasattr(M, "apply_") else ild.FactorOperator(M)


def _factors(M):
    """the factors as (data, indices, indptr, is_csr) from factor_copy"""
    return [(f[0], f[1], f[2], f[3]) for f in M.pr.factors_info()]


def _same_factors(F, G):
    return len(F) == len(G) == 2 and all(a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and
                                         np.array_equal(_bits(a[0]), _bits(b[0])) for a, b in zip(F, G))


def _rhs(n, seed=0):
    return np.random.default_rng(2000 + seed).standard_normal(n) + 2.0


def _three_applies(M, n, seed):
    """apply_ in both directions and a block apply_ of k = 3, on clones: the host copies"""
    import torch
    S = _single(M)
    v = torch.from_numpy(_rhs(n, seed)).cuda()
    X = torch.from_numpy(np.random.default_rng(3000 + seed).standard_normal((n, 3)) + 2.0).cuda().contiguous()
    return [S.apply_(v.clone()).cpu().numpy(), S.apply_(v.clone(), transpose=True).cpu().numpy(), S.apply_(X.clone()).cpu().numpy()]


def _build_batch(mode, mats):
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    if mode == "device":
        return ild.DevicePreconditioner.batch("ILU0", [_dev(A) for A in mats])
    return ilupp.ILU0Preconditioner.batch([A.tocsc() if mode == "host-csc" else A for A in mats])


def _build_single(mode, A):
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    if mode == "device":
        return ild.DevicePreconditioner("ILU0", _dev(A))
    return ilupp.ILU0Preconditioner(A.tocsc() if mode == "host-csc" else A)


# ---- 1. one mixed batch, three ways ----
def _mixed_matrices():
    mats = [("random_dd(%d)" % n, _random(n, 500 + k)) for k, n in enumerate(SIZES)]
    mats.append(("laplace1d(300)", _csr(matgen.laplace1d(300))))          # every row waits for the one before: the longest chain
    mats.append(("poisson2d(16)", _csr(matgen.poisson2d(16))))
    mats.append(("poisson3d(6)", _csr(matgen.poisson3d(6))))              # singly the static form; here route 0
    mats.append(("random_dd(1100, 19)", _random(1100, 520, k=19)))        # singly ilu0:level-order; here route 0
    mats.append(("arrow(300)", _arrow(300)))                              # a row as long as n: route 1
    mats.append(("band(96, 31)", _band(96, 15)))                          # the row cap itself: route 0
    mats.append(("band(96, 33)", _band(96, 15, wide_row=40)))             # one row of 33: route 1
    return mats


ROUTE_1 = ("arrow(300)", "band(96, 33)")
ROW_CAP = 31                                     # the longest row the launches take (n is far below the cap of the flags here)


@pytest.fixture(scope="module", params=["host-csr", "host-csc", "device"])
def mixed(request):
    mode = request.param
    mats = _mixed_matrices()
    names, As = [m[0] for m in mats], [m[1] for m in mats]
    assert [int(np.diff(A.indptr).max()) for A in As[-2:]] == [31, 33]
    members = _build_batch(mode, As)
    twins = [_build_single(mode, A) for A in As]
    out = dict(mode=mode, names=names, ns=[A.shape[0] for A in As])
    # the matrix that is factored is the row-major view of what is handed in: for CSC input the transposed one, whose rows are A's columns
    longest = [int(np.diff((A.tocsc() if mode == "host-csc" else A).indptr).max()) for A in As]
    out["single"] = [name for name, m in zip(names, longest) if m > ROW_CAP]
    if mode != "host-csc":
        assert tuple(out["single"]) == ROUTE_1
    assert set(ROUTE_1) <= set(out["single"]) and "band(96, 31)" not in out["single"]
    for key, objs in (("got", members), ("want", twins)):
        out[key] = dict(path=[M.pr.path() for M in objs], factors=[_factors(M) for M in objs],
                        nnz=[M.pr.total_nnz for M in objs], timings=[M.pr.timings() for M in objs])
        out[key]["path_after_factors"] = [M.pr.path() for M in objs]
        out[key]["applies"] = [_three_applies(M, n, k) for k, (M, n) in enumerate(zip(objs, out["ns"]))]
    if mode != "device":
        # the host class as a LinearOperator (host vectors through ilupp_hip_apply)
        out["got"]["matvec"] = [P @ _rhs(n, 9) for P, n in zip(members, out["ns"])]
        out["want"]["matvec"] = [P @ _rhs(n, 9) for P, n in zip(twins, out["ns"])]
        out["reprs"] = [(repr(P), repr(T)) for P, T in zip(members, twins)]
    return out


def test_mixed_batch_paths_and_routes(mixed):
    got, want = mixed["got"], mixed["want"]
    print("%s: %s" % (mixed["mode"], list(zip(mixed["names"], got["path"], want["path"]))))
    for name, g, w, g2 in zip(mixed["names"], got["path"], want["path"], got["path_after_factors"]):
        # a member the launches built says so; one the single constructor built inside the call is the object the single call builds
        assert g == (w if name in mixed["single"] else BATCH), (name, g, w)
        assert g2 == g, name
    assert "static" in want["path"][mixed["names"].index("poisson3d(6)")]
    assert want["path"][mixed["names"].index("random_dd(1100, 19)")] == "ilu0:level-order"
    for name in ROUTE_1:
        assert want["path"][mixed["names"].index(name)] != BATCH


def test_mixed_batch_factors_are_the_single_constructor_s(mixed):
    got, want = mixed["got"], mixed["want"]
    for k, name in enumerate(mixed["names"]):
        assert _same_factors(got["factors"][k], want["factors"][k]), name
        assert got["nnz"][k] == want["nnz"][k], name
        assert all(np.all(np.isfinite(f[0])) for f in got["factors"][k]), name
        assert all(f[3] == (mixed["mode"] != "host-csc") for f in got["factors"][k]), name
    # the two launches' times, shared by the members they built
    launched = [k for k, name in enumerate(mixed["names"]) if name not in mixed["single"]]
    t0 = got["timings"][launched[0]]
    assert t0["numeric_ms"] > 0 and t0["analysis_ms"] > 0
    for k in launched:
        assert got["timings"][k]["numeric_ms"] == t0["numeric_ms"] and got["timings"][k]["analysis_ms"] == t0["analysis_ms"]


def test_mixed_batch_applies_are_the_single_constructor_s(mixed):
    """apply_, transposed apply_ and a block apply_ of k = 3: the single paths' tables of a launched member are built at its first apply"""
    got, want = mixed["got"], mixed["want"]
    for k, name in enumerate(mixed["names"]):
        for j in range(3):
            assert np.array_equal(_bits(got["applies"][k][j]), _bits(want["applies"][k][j])), (name, j)
            assert np.all(np.isfinite(got["applies"][k][j])), (name, j)
    if mixed["mode"] != "device":
        for k, name in enumerate(mixed["names"]):
            assert np.array_equal(_bits(got["matvec"][k]), _bits(want["matvec"][k])), name
            assert mixed["reprs"][k][0] == mixed["reprs"][k][1], name


# ---- 2. straight into the batched launches, before any single apply ----
def _packed(ns, seed):
    offsets, total = [], 3
    for n in ns:
        offsets.append(total)
        total += n + 3
    host = np.zeros(total)
    for k, (o, n) in enumerate(zip(offsets, ns)):
        host[o:o + n] = _rhs(n, seed + k)
    return offsets, host


def test_batch_built_members_go_straight_into_the_launches():
    import torch
    import ilupp_amd.device as ild
    ns = [65, 257, 300, 256]
    spd = [_spd(n, 540 + k) for k, n in enumerate(ns[:3])] + [_csr(matgen.poisson2d(16))]
    gen = [_random(n, 640 + k) for k, n in enumerate(ns)]
    offsets, host = _packed(ns, 50)
    kw = dict(maxiter=6, rtol=0.0, check_every=0)
    for mats, solver in ((spd, ild.cg_batch), (gen, ild.bicgstab_batch)):
        dAs = [_dev(A) for A in mats]
        members = ild.DevicePreconditioner.batch("ILU0", dAs)
        singles = [ild.DevicePreconditioner("ILU0", dA) for dA in dAs]
        assert [M.pr.path() for M in members] == [BATCH] * 4
        res = {}
        for key, Ms in (("got", members), ("want", singles)):
            x = torch.from_numpy(host).cuda()
            r1 = ild.apply_batch_(Ms, x, offsets)
            xt = torch.from_numpy(host).cuda()
            r2 = ild.apply_batch_(Ms, xt, offsets, transpose=True)
            st = {}
            y = solver(dAs, torch.from_numpy(host).cuda(), offsets, Ms, stats=st, **kw)
            res[key] = (x.cpu().numpy(), xt.cpu().numpy(), y.cpu().numpy(), r1, r2, list(st["route"]), st["iterations"].tolist())
        for j in range(3):
            assert np.array_equal(_bits(res["got"][j]), _bits(res["want"][j])), (solver.__name__, j)
            assert np.all(np.isfinite(res["got"][j]))
        assert res["got"][3:] == res["want"][3:]
        assert res["got"][3] == [0] * 4 and res["got"][4] == [0] * 4 and res["got"][5] == [0] * 4
        assert [M.pr.path() for M in members] == [BATCH] * 4


# ---- 3. re-factorisation ----
def test_refactor_batch_takes_batch_built_members_at_route_0():
    import ilupp_amd.device as ild
    mats = [_random(n, 700 + k) for k, n in enumerate([65, 257, 513])] + [_random(1100, 520, k=19)]
    A2 = [_scaled(A, 40 + k) for k, A in enumerate(mats)]
    dAs, dA2 = [_dev(A) for A in mats], [_dev(A) for A in A2]
    members = ild.DevicePreconditioner.batch("ILU0", dAs)
    old = [_factors(M) for M in members]
    routes, status = ild.refactor_batch_(members, dA2, check=False)
    assert routes == [0] * 4 and status.cpu().tolist() == [0] * 4
    fresh = [_factors(ild.DevicePreconditioner("ILU0", dA)) for dA in dA2]
    for k in range(4):
        assert _same_factors(_factors(members[k]), fresh[k]), k
        assert not _same_factors(_factors(members[k]), old[k]), k
    # alone in the call with n >= 1 000: a singly built member takes the single path there, which this member does not have
    routes, status = ild.refactor_batch_(members[3:], dAs[3:], check=False)
    assert routes == [0] and status.cpu().tolist() == [0]
    assert _same_factors(_factors(members[3]), old[3])
    assert [M.pr.path() for M in members] == [BATCH] * 4


def test_single_refactor_of_a_batch_built_member():
    import torch
    import ilupp_amd.device as ild
    mats = [_random(300, 530), _random(1100, 521, k=19)]
    dAs = [_dev(A) for A in mats]
    dA2 = [_dev(_scaled(A, 61 + k)) for k, A in enumerate(mats)]
    members = ild.DevicePreconditioner.batch("ILU0", dAs)
    for M, dA, A in zip(members, dA2, mats):
        n = A.shape[0]
        v = torch.from_numpy(_rhs(n, 3)).cuda()
        before = M.apply_(v.clone()).cpu().numpy()                       # (the single sweeps' tables exist before the re-factorisation)
        assert M.refactor_(dA) is M
        fresh = ild.DevicePreconditioner("ILU0", dA)
        assert _same_factors(_factors(M), _factors(fresh))
        after = M.apply_(v.clone()).cpu().numpy()
        assert np.array_equal(_bits(after), _bits(fresh.apply_(v.clone()).cpu().numpy()))
        assert not np.array_equal(_bits(after), _bits(before))
        for a, b in zip(_three_applies(M, n, 4), _three_applies(fresh, n, 4)):
            assert np.array_equal(_bits(a), _bits(b))
    C = mats[0].copy()
    C.data[C.indptr[3]] = 0.0
    C.eliminate_zeros()
    assert C.nnz == mats[0].nnz - 1
    with pytest.raises(RuntimeError, match="^ILU0 refactor: the matrix does not have the analysed pattern"):
        members[0].refactor_(_dev(C))                                    # (another number of stored entries: refused as the single path refuses it)


# ---- 4. errors and edge cases ----
def _without_diagonal(A, row):
    B = A.tolil()
    B[row, row] = 0.0
    B = B.tocsr()
    B.eliminate_zeros()
    B.sort_indices()
    assert B.nnz == A.nnz - 1
    return B


def test_missing_diagonal_fails_as_the_single_constructor_does():
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    good = [_random(65, 800), _random(300, 801)]
    bad = _without_diagonal(_random(257, 802), 3)
    with pytest.raises(RuntimeError, match="ILU0: structurally missing diagonal entry in row 3") as single:
        ild.DevicePreconditioner("ILU0", _dev(bad))
    assert str(single.value) == "ILU0: structurally missing diagonal entry in row 3"
    live = _native.live_blocks()
    for build in (lambda ms: ild.DevicePreconditioner.batch("ILU0", [_dev(A) for A in ms]), ilupp.ILU0Preconditioner.batch):
        with pytest.raises(RuntimeError, match="^matrix 1 of the batch: ILU0: structurally missing diagonal entry in row 3") as batch:
            build([good[0], bad, good[1]])
        assert type(batch.value) is type(single.value)
        assert _native.live_blocks() == live                             # (every object of the failed call is gone)
        members = build(good)                                            # (a following batch of the good members succeeds)
        assert [M.pr.path() for M in members] == [BATCH] * 2
        for k, A in enumerate(good):
            assert _same_factors(_factors(members[k]), _factors(ild.DevicePreconditioner("ILU0", _dev(A)))), k
        del members


def test_unsorted_row_goes_to_the_single_constructor():
    """two entries behind the diagonal of one row change places: the single constructor builds something from such a matrix (no row it
    waits for changes), and the batch gives exactly that"""
    import torch
    import ilupp_amd.device as ild
    mats = [_random(65, 810), _random(257, 811), _random(65, 812)]
    B = mats[1].copy()
    row = next(r for r in range(B.shape[0]) if np.sum(B.indices[B.indptr[r]:B.indptr[r + 1]] > r) >= 2)
    q = B.indptr[row + 1] - 2
    B.indices[[q, q + 1]] = B.indices[[q + 1, q]]
    B.data[[q, q + 1]] = B.data[[q + 1, q]]
    unsorted = ild.DeviceCSR(torch.from_numpy(B.data.copy()).cuda(), torch.from_numpy(B.indices.astype(np.int32)).cuda(),
                             torch.from_numpy(B.indptr.astype(np.int32)).cuda())
    dAs = [_dev(mats[0]), unsorted, _dev(mats[2])]
    twin = ild.DevicePreconditioner("ILU0", unsorted)
    members = ild.DevicePreconditioner.batch("ILU0", dAs)
    assert [M.pr.path() for M in members] == [BATCH, twin.pr.path(), BATCH]
    assert _same_factors(_factors(members[1]), _factors(twin))
    for k in (0, 2):
        assert _same_factors(_factors(members[k]), _factors(ild.DevicePreconditioner("ILU0", dAs[k]))), k


def test_non_finite_values_match_the_single_constructor():
    import ilupp_amd.device as ild
    mats = [_random(65, 570 + k) for k in range(4)]
    first_row = list(mats[0].indices[mats[0].indptr[0]:mats[0].indptr[1]])
    mats[0].data[mats[0].indptr[0] + first_row.index(0)] = 0.0           # a_00 = 0: a zero pivot
    mats[2].data[mats[2].indptr[20] + 1] = np.nan
    dAs = [ild.DeviceCSR.from_scipy(A) for A in mats]
    assert [d.nnz for d in dAs] == [A.nnz for A in mats]                 # (the stored zero stays stored)
    members = ild.DevicePreconditioner.batch("ILU0", dAs)
    assert [M.pr.path() for M in members] == [BATCH] * 4                 # (neither is an error)
    got = [_factors(M) for M in members]
    for k, dA in enumerate(dAs):
        assert _same_factors(got[k], _factors(ild.DevicePreconditioner("ILU0", dA))), k
    assert not np.all(np.isfinite(got[0][1][0])) and not np.all(np.isfinite(got[2][1][0]))
    for k in (1, 3):                                                      # the clean neighbours
        assert np.all(np.isfinite(got[k][0][0])) and np.all(np.isfinite(got[k][1][0]))


# ---- 5. more workgroups than CUs ----
def test_many_members():
    import ilupp_amd.device as ild
    mats = [_random(40, 600 + k) for k in range(300)]
    dAs = [_dev(A) for A in mats]
    members = ild.DevicePreconditioner.batch("ILU0", dAs)
    assert len(members) == 300 and all(M.pr.path() == BATCH for M in members)
    for k, (M, dA) in enumerate(zip(members, dAs)):
        assert _same_factors(_factors(M), _factors(ild.DevicePreconditioner("ILU0", dA))), k


# ---- 6. the cap ----
def test_cap_routes_large_members_to_the_single_constructor(monkeypatch):
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    assert _native.ilu0_refactor_batch_max_n() >= 4000
    monkeypatch.setenv("ILUPP_BATCH_APPLY_MAX_N", "600")
    assert _native.ilu0_refactor_batch_max_n() == 600
    mats = [_random(700, 580), _random(513, 581)]
    dAs = [_dev(A) for A in mats]
    members = ild.DevicePreconditioner.batch("ILU0", dAs)
    twins = [ild.DevicePreconditioner("ILU0", dA) for dA in dAs]
    assert [M.pr.path() for M in members] == [twins[0].pr.path(), BATCH]
    for k in range(2):
        assert _same_factors(_factors(members[k]), _factors(twins[k])), k
        for a, b in zip(_three_applies(members[k], mats[k].shape[0], k), _three_applies(twins[k], mats[k].shape[0], k)):
            assert np.array_equal(_bits(a), _bits(b)), k


def test_a_batch_of_one_is_the_single_constructor_s_object():
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    A = _random(300, 590)
    dA = _dev(A)
    for M, T in ((ild.DevicePreconditioner.batch("ILU0", [dA])[0], ild.DevicePreconditioner("ILU0", dA)),
                 (ilupp.ILU0Preconditioner.batch([A])[0], ilupp.ILU0Preconditioner(A))):
        assert M.pr.path() == T.pr.path() != BATCH
        assert _same_factors(_factors(M), _factors(T))


# ---- 7. speed ----
def test_batched_construction_beats_the_loop_at_16_members():
    """16 members of n = 1 000: the median of five batched constructions (host clock around the call plus a device synchronisation, after
    two warm-up calls) is below the median of the loop of single constructions over the same matrices in the same process"""
    import torch
    import ilupp_amd.device as ild
    dAs = [_dev(_random(1000, 900 + k)) for k in range(16)]
    ild._on_current_stream()

    def batched():
        return ild.DevicePreconditioner.batch("ILU0", dAs)

    def looped():
        return [ild.DevicePreconditioner("ILU0", dA) for dA in dAs]

    def median(fn):
        ts = []
        for it in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            del keep
        return float(np.median(ts[2:])) * 1e3

    t_loop = median(looped)
    t_batch = median(batched)
    print("16 members of n = 1000: batched %.3f ms, looped %.3f ms (%.1f x)" % (t_batch, t_loop, t_loop / t_batch))
    assert t_batch < t_loop
