"""GPU tests of the tables the batched entries keep from call to call (BatchScratch in api_batch.h: descriptor tables, error and status
words, the hand-over block, the packed staging block): a table that exists and holds a cached upload is freed and allocated again when a
call brings more members than any call before it.  Every test goes from 5 members to 70 (the descriptor tables start at 64 entries) and
back, and compares every operation bitwise on int64 views with the same operation done one member at a time -- on twin objects the
single constructors built, or, for the pivoting classes, by the member's own single apply.  The routes are asserted (all 0 at these
sizes): a member that took the single path inside the call would say nothing about the launch.

Matrices: matgen.random_dd(n, 8, 25.0, seed) with n cycling over 3, 17, 40, 65 (one round of rows, a partial wave, one past a wave; every
n > 2, which BiCGstab needs); the re-factorisations take every value scaled by 1 + 0.1 u.  Every solve runs 4 iterations with rtol = 0.
The multilevel members (sections 4) are tiny objects of their own: see the `multilevel` fixture."""
import numpy as np
import pytest
import scipy.sparse as sp

import matgen

pytestmark = pytest.mark.gpu

NS = [3, 17, 40, 65]
SMALL, LARGE = 5, 70
KW = dict(maxiter=4, rtol=0.0, check_every=0)


def _csr(t):
    d, i, p = t
    n = p.shape[0] - 1
    A = sp.csr_matrix((np.asarray(d, dtype=np.float64), i, p), shape=(n, n))
    A.sort_indices()
    return A


def _random(n, seed):
    return _csr(matgen.random_dd(n, 8, 25.0, seed))


def _spd(n, seed):
    A = sp.csr_matrix(matgen.symmetrize(*matgen.random_dd(n, 8, 25.0, seed)), shape=(n, n))
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


def _factors(M):
    return [(f[0], f[1], f[2], f[3]) for f in M.pr.factors_info()]


def _same_factors(F, G):
    return len(F) == len(G) == 2 and all(a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and
                                         np.array_equal(_bits(a[0]), _bits(b[0])) for a, b in zip(F, G))


def _rhs(n, seed):
    return np.random.default_rng(2000 + seed).standard_normal(n) + 2.0


def _packed(ns, lo=0):
    """member k's vector (that of twin lo + k) at offsets[k] of one packed vector, three untouched words between neighbours"""
    offsets, total = [], 3
    for n in ns:
        offsets.append(total)
        total += n + 3
    host = np.full(total, -7.0)
    for k, (o, n) in enumerate(zip(offsets, ns)):
        host[o:o + n] = _rhs(n, lo + k)
    return offsets, host


def _matrices(count, seed):
    return [_random(NS[k % len(NS)], seed + k) for k in range(count)]


# ---- what the members one at a time give: computed once on the twins, for the original values and for the scaled ones ----
def _single_results(twins, dAs, ns):
    """factors, total_nnz, apply_ in both directions and 4 iterations of bicgstab of every twin, on member k's slice of _packed(ns)"""
    import torch
    import ilupp_amd.device as ild
    offsets, host = _packed(ns)
    out = dict(factors=[_factors(T) for T in twins], nnz=[T.pr.total_nnz for T in twins], apply=[], apply_t=[], bicgstab=[])
    for T, dA, o, n in zip(twins, dAs, offsets, ns):
        v = torch.from_numpy(host[o:o + n]).cuda()
        out["apply"].append(T.apply_(v.clone()).cpu().numpy())
        out["apply_t"].append(T.apply_(v.clone(), transpose=True).cpu().numpy())
        out["bicgstab"].append(ild.bicgstab(dA, v[:, None], T, **KW).cpu().numpy()[:, 0])
    return out


@pytest.fixture(scope="module")
def plain():
    """70 matrices, their scaled versions, and the results of 70 singly built twins before and after their single re-factorisation"""
    import ilupp_amd.device as ild
    mats = _matrices(LARGE, 9000)
    ns = [A.shape[0] for A in mats]
    d1 = [_dev(A) for A in mats]
    d2 = [_dev(_scaled(A, 9500 + k)) for k, A in enumerate(mats)]
    twins = [ild.DevicePreconditioner("ILU0", dA) for dA in d1]
    want1 = _single_results(twins, d1, ns)
    for T, dA in zip(twins, d2):
        assert T.refactor_(dA) is T
    want2 = _single_results(twins, d2, ns)
    return dict(mats=mats, ns=ns, d1=d1, d2=d2, want1=want1, want2=want2)


def _check_factors(members, want, lo, tag):
    for k, M in enumerate(members):
        assert _same_factors(_factors(M), want["factors"][lo + k]), (tag, k)
        assert M.pr.total_nnz == want["nnz"][lo + k], (tag, k)


def _check_launches(members, dAs, ns, want, lo, tag):
    """apply_batch_ in both directions and bicgstab_batch over `members` (the twins lo, lo + 1, ...): every member on route 0 with its
    twin's bits, and nothing written between the vectors"""
    import torch
    import ilupp_amd.device as ild
    offsets, host = _packed(ns, lo)
    inside = np.zeros(host.shape[0], dtype=bool)
    for o, n in zip(offsets, ns):
        inside[o:o + n] = True
    for key, transpose in (("apply", False), ("apply_t", True)):
        x = torch.from_numpy(host).cuda()
        assert ild.apply_batch_(members, x, offsets, transpose=transpose) == [0] * len(members), (tag, key)
        xh = x.cpu().numpy()
        assert np.array_equal(xh[~inside], host[~inside]), (tag, key)
        for k, (o, n) in enumerate(zip(offsets, ns)):
            assert np.array_equal(_bits(xh[o:o + n]), _bits(want[key][lo + k])), (tag, key, k)
    st = {}
    y = ild.bicgstab_batch(dAs, torch.from_numpy(host).cuda(), offsets, members, stats=st, **KW).cpu().numpy()
    assert list(st["route"]) == [0] * len(members), tag
    for k, (o, n) in enumerate(zip(offsets, ns)):
        assert np.array_equal(_bits(y[o:o + n]), _bits(want["bicgstab"][lo + k])), (tag, "bicgstab", k)


def _refactor(members, dAs, tag):
    import ilupp_amd.device as ild
    routes, status = ild.refactor_batch_(members, dAs, check=False)
    assert routes == [0] * len(members) and status.cpu().tolist() == [0] * len(members), tag


def _check_cg(tag):
    """cg_batch over batch-built members of three symmetrised matrices against cg with singly built twins"""
    import torch
    import ilupp_amd.device as ild
    mats = [_spd(n, 9800 + k) for k, n in enumerate(NS[1:])]
    ns = [A.shape[0] for A in mats]
    dAs = [_dev(A) for A in mats]
    members = ild.DevicePreconditioner.batch("ILU0", dAs)
    twins = [ild.DevicePreconditioner("ILU0", dA) for dA in dAs]
    offsets, host = _packed(ns)
    st = {}
    y = ild.cg_batch(dAs, torch.from_numpy(host).cuda(), offsets, members, stats=st, **KW).cpu().numpy()
    assert list(st["route"]) == [0] * len(members), tag
    for k, (T, dA, o, n) in enumerate(zip(twins, dAs, offsets, ns)):
        want = ild.cg(dA, torch.from_numpy(host[o:o + n]).cuda()[:, None], T, **KW).cpu().numpy()[:, 0]
        assert np.array_equal(_bits(y[o:o + n]), _bits(want)), (tag, k)


# ---- 1. non-pivoting members on the device entries ----
def test_device_entries_grow_their_tables_from_5_to_70_members(plain):
    import ilupp_amd.device as ild
    ns, d1, d2, want1, want2 = plain["ns"], plain["d1"], plain["d2"], plain["want1"], plain["want2"]
    s = SMALL
    # (a) the construction of 5
    few = ild.DevicePreconditioner.batch("ILU0", d1[:s])
    assert [M.pr.path() for M in few] == ["ilu0:batch"] * s
    _check_factors(few, want1, 0, "a")
    # (b) every launch with 5: applies and a solve, the re-factorisation (its table was cached by the construction), the same again
    _check_launches(few, d1[:s], ns[:s], want1, 0, "b, first values")
    _refactor(few, d2[:s], "b")
    _check_factors(few, want2, 0, "b")
    _check_launches(few, d2[:s], ns[:s], want2, 0, "b, scaled values")
    _check_cg("b")
    # (c) the construction of 70: the create records and the re-factorisation's table grow, the latter with a cached table in it
    many = ild.DevicePreconditioner.batch("ILU0", d1)
    assert [M.pr.path() for M in many] == ["ilu0:batch"] * LARGE
    _check_factors(many, want1, 0, "c")
    _check_factors(few, want2, 0, "c, the 5 of before")
    # (d) every launch with 70: the apply's table, the error words, the hand-over block and the systems' table grow
    _check_launches(many, d1, ns, want1, 0, "d, first values")
    _refactor(many, d2, "d")
    _check_factors(many, want2, 0, "d")
    _check_launches(many, d2, ns, want2, 0, "d, scaled values")
    # (e) 5 of them twice in a row (an upload into the grown tables, then a cache hit), then the 70 again (a miss without growth)
    for again in range(2):
        _refactor(many[:s], d2[:s], ("e", again))
        _check_factors(many[:s], want2, 0, ("e", again))
        _check_launches(many[:s], d2[:s], ns[:s], want2, 0, ("e", again))
    _refactor(many, d1, "e, the 70")
    _check_factors(many, want1, 0, "e, the 70")
    _check_launches(many, d1, ns, want1, 0, "e, the 70")
    # members in the middle of the list: other offsets, other slices of the hand-over block
    _check_launches(many[30:41], d1[30:41], ns[30:41], want1, 30, "e, members 30 - 40")


# ---- 2. pivoting members on the host entry: the packed staging block of the vectors grows ----
@pytest.mark.parametrize("kind", ["ilucp", "ilutp"])
def test_pivot_apply_batch_grows_its_staging_from_5_to_70_vectors(kind):
    import ilupp_amd as ilupp
    from ilupp_amd import _native
    cls = ilupp.ILUCPPreconditioner if kind == "ilucp" else ilupp.ILUTPPreconditioner
    mats = _matrices(LARGE, 9100)
    rhs = [_rhs(A.shape[0], 100 + k) for k, A in enumerate(mats)]
    few, many = cls.batch(mats[:SMALL]), cls.batch(mats)
    want = [(P @ b, P.T @ b) for P, b in zip(many, rhs)]                 # every member's single apply
    for k, (P, b) in enumerate(zip(few, rhs)):
        assert np.array_equal(_bits(P @ b), _bits(want[k][0])) and np.array_equal(_bits(P.T @ b), _bits(want[k][1])), k
    for tag, B in (("5", few), ("70", many), ("5 again", few), ("5 of the 70", many[:SMALL])):
        for transpose in (False, True):
            x = [b.copy() for b in rhs[:len(B)]]
            assert _native.pivot_apply_batch([P.pr for P in B], x, transpose) == [0] * len(B), (tag, transpose)
            for k in range(len(B)):
                assert np.array_equal(_bits(x[k]), _bits(want[k][1 if transpose else 0])), (tag, transpose, k)
                assert np.all(np.isfinite(x[k])), (tag, transpose, k)


# ---- 3. non-pivoting members on the host entry: the packed staging block of the matrices grows ----
def test_host_construction_grows_its_staging_from_5_to_70_matrices(plain):
    import ilupp_amd as ilupp
    mats, ns = plain["mats"], plain["ns"]
    twins = [ilupp.ILU0Preconditioner(A) for A in mats]
    want = [(_factors(T), T.pr.total_nnz, T @ _rhs(n, 200 + k)) for k, (T, n) in enumerate(zip(twins, ns))]
    for count in (SMALL, LARGE, SMALL):
        members = ilupp.ILU0Preconditioner.batch(mats[:count])
        assert [M.pr.path() for M in members] == ["ilu0:batch"] * count      # (route 0: a member of route 1 has the single constructor's path)
        for k, M in enumerate(members):
            assert _same_factors(_factors(M), want[k][0]), (count, k)
            assert M.pr.total_nnz == want[k][1], (count, k)
            assert np.array_equal(_bits(M @ _rhs(ns[k], 200 + k)), _bits(want[k][2])), (count, k)


# ---- 4. multilevel members: the member table, the level table and the staging block of the batched multilevel apply grow ----
@pytest.fixture(scope="module")
def multilevel():
    """70 multilevel members built the way tests/test_gpu_ml_apply_batch.py builds its smallest ones -- n = 1 and n = 2, the family without
    pivoting under its "t0.1" set and default-constructed parameters, CSR and CSC --, every matrix scaled by a factor of its own so that no
    two members apply alike; their right-hand sides and their single applies in both directions, computed once"""
    import ilupp_amd as ilupp
    import ml_cases
    _, thr, pre, knobs = {p[0]: p for p in ml_cases.PARAMS}["t0.1"]
    one, two = np.array([[2.0]]), np.array([[2.0, 1.0], [0.5, 3.0]])
    t01 = ml_cases.engine_params(ilupp, thr, pre, knobs)
    build = [lambda s: ilupp.ILUppPreconditioner(sp.csr_matrix(one * s), params=t01),
             lambda s: ilupp.ILUppPreconditioner(sp.csr_matrix(two * s), params=t01),
             lambda s: ilupp.ILUppPreconditioner(sp.csr_matrix(one * s)),
             lambda s: ilupp.ILUppPreconditioner(sp.csc_matrix(two * s))]
    members = [build[k % 4](1.0 + k / 8.0) for k in range(LARGE)]
    ns = [P.shape[0] for P in members]
    rhs = [_rhs(n, 300 + k) for k, n in enumerate(ns)]
    want = dict(apply=[P @ b for P, b in zip(members, rhs)], apply_t=[P.T @ b for P, b in zip(members, rhs)])
    return dict(members=members, ns=ns, rhs=rhs, want=want)


def _ml_packed(ns, rhs):
    """_packed with the multilevel members' own right-hand sides"""
    offsets, host = _packed(ns)
    for o, b in zip(offsets, rhs):
        host[o:o + b.shape[0]] = b
    return offsets, host


def _check_ml_launch(ml, lo, hi, tag):
    """ml_apply_batch_ in both directions over the members lo .. hi - 1: every member on route 0 with its single apply's bits, and nothing
    written between the vectors"""
    import torch
    import ilupp_amd.device as ild
    members, ns, rhs = ml["members"][lo:hi], ml["ns"][lo:hi], ml["rhs"][lo:hi]
    offsets, host = _ml_packed(ns, rhs)
    inside = np.zeros(host.shape[0], dtype=bool)
    for o, n in zip(offsets, ns):
        inside[o:o + n] = True
    for key, transpose in (("apply", False), ("apply_t", True)):
        x = torch.from_numpy(host).cuda()
        assert ild.ml_apply_batch_(members, x, offsets, transpose=transpose) == [0] * len(members), (tag, key)
        xh = x.cpu().numpy()
        assert np.array_equal(xh[~inside], host[~inside]), (tag, key)
        for k, (o, n) in enumerate(zip(offsets, ns)):
            assert np.array_equal(_bits(xh[o:o + n]), _bits(ml["want"][key][lo + k])), (tag, key, k)


def test_ml_apply_batch_device_grows_its_tables_from_5_to_70_members(multilevel):
    s = SMALL
    _check_ml_launch(multilevel, 0, s, "5")
    _check_ml_launch(multilevel, 0, LARGE, "70")                 # (both tables grow with a cached upload in them)
    for again in range(2):                                      # (an upload into the grown tables, then a cache hit)
        _check_ml_launch(multilevel, 0, s, ("5 again", again))
    _check_ml_launch(multilevel, 0, LARGE, "70 again")           # (a miss without growth)
    _check_ml_launch(multilevel, 30, 41, "members 30 - 40")      # (other offsets, other places in the level table)


def test_ml_apply_batch_host_grows_its_staging_from_5_to_70_vectors(multilevel):
    """the host entry: the packed staging block it shares with the pivoting classes' host entry"""
    from ilupp_amd import _native
    members, rhs, want = multilevel["members"], multilevel["rhs"], multilevel["want"]
    for tag, lo, hi in (("5", 0, SMALL), ("70", 0, LARGE), ("5 again", 0, SMALL), ("5 of the middle", 30, 35)):
        for key, transpose in (("apply", False), ("apply_t", True)):
            x = [b.copy() for b in rhs[lo:hi]]
            assert _native.ml_apply_batch([P.pr for P in members[lo:hi]], x, transpose) == [0] * (hi - lo), (tag, key)
            for k in range(hi - lo):
                assert np.array_equal(_bits(x[k]), _bits(want[key][lo + k])), (tag, key, k)


def test_plain_and_multilevel_applies_interleaved_on_one_scratch(plain, multilevel):
    """a plain apply_batch_, an ml_apply_batch_, the same plain apply_batch_ again: the two descriptor paths of the one scaffold keep their
    cached tables apart, and all three have the single applies' bits"""
    import torch
    import ilupp_amd.device as ild
    s, ns, d1, want1 = 11, plain["ns"], plain["d1"], plain["want1"]
    members = ild.DevicePreconditioner.batch("ILU0", d1[:s])
    offsets, host = _packed(ns[:s])

    def plain_apply(tag):
        x = torch.from_numpy(host).cuda()
        assert ild.apply_batch_(members, x, offsets) == [0] * s, tag
        xh = x.cpu().numpy()
        for k, (o, n) in enumerate(zip(offsets, ns[:s])):
            assert np.array_equal(_bits(xh[o:o + n]), _bits(want1["apply"][k])), (tag, k)

    plain_apply("before")
    _check_ml_launch(multilevel, 0, s, "between")
    plain_apply("after")


# ---- 5. ILUT members: the descriptors, the ticket maps and the records of the batched ILUT construction grow ----
def test_ilut_construction_grows_its_tables_from_5_to_70_matrices(plain):
    import ilupp_amd as ilupp
    mats = plain["mats"]
    want = [_factors(ilupp.ILUTPreconditioner(A)) for A in mats]
    for count in (SMALL, LARGE, SMALL):
        members = ilupp.ILUTPreconditioner.batch(mats[:count])
        assert [M.pr.path() for M in members] == ["ilut:batch"] * count      # (route 0: a member of route 1 has the single constructor's path)
        for k, M in enumerate(members):
            assert _same_factors(_factors(M), want[k]), (count, k)
