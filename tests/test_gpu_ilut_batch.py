"""GPU tests of the batched FIRST construction of ILUT members (ilupp_amd.ILUTPreconditioner.batch over ilupp_hip_ilut_create_batch,
ilupp_amd.device.ilut_batch over ilupp_hip_ilut_create_batch_device: the rows of all members in one launch of k_ilut_rows_batch per LDS
class, one count-and-scan launch, one read-back, one fill launch).  Every comparison is bitwise on int64 views; the reference is the
object the single constructor builds from the same matrix -- ILUTPreconditioner(A, ...) for the host class, DevicePreconditioner("ILUT",
dA, ...) for the device class -- and, for the designed cases of tests/ilut_cases.py, the oracle's factor and the route ilut_ref predicts.
Seeds move with ILUPP_FUZZ_OFFSET."""
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import ilut_cases as C
import ilut_ref as R
import matgen
from capture_util import Env as _Env, Stderr as _Stderr

pytestmark = pytest.mark.gpu

BATCH = "ilut:batch"
OFF = int(os.environ.get("ILUPP_FUZZ_OFFSET", "0"))
PARAMS = [(10, 1e-4), (100, 0.1)]
MODES = ["host", "host-csc", "device"]
# the ticket map: a member of one row first and last, members shorter and longer than a wave and than the count launch's 256 lanes; two
# members of one row (one round); more members than a wave has lanes
TICKET_CASES = {"mixed": [1, 300, 2, 65, 257], "mixed-reversed": [257, 65, 2, 300, 1], "two-of-one": [1, 1], "seventy": [40] * 70}
_RE_MEMBER = re.compile(r"\[ilupp\] ilut_batch: member (\d+): (\d+) of (\d+) rows outgrew LDS \(pool (\d+), U slots (\d+), kept (\d+)\), (\d+) of them "
                        r"the pool-in-LDS tier too, status (-?\d+)")


def _csr(t):
    d, i, p = t
    n = p.shape[0] - 1
    A = sp.csr_matrix((np.asarray(d, dtype=np.float64), i, p), shape=(n, n))
    A.sort_indices()
    return A


def _random(n, seed, k=8):
    return _csr(matgen.random_dd(n, k, 25.0, seed + OFF))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _dev(A):
    import ilupp_amd.device as ild
    return ild.DeviceCSR.from_scipy(A)


def _single(M):
    import ilupp_amd.device as ild
    return M if hasattr(M, "apply_") else ild.FactorOperator(M)


def _factors(M):
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


def _build_batch(mode, mats, fill, tau):
    """(members, routes) of one batched construction; the routes are taken off the native layer on the way"""
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    name = "ILUTPreconditioner_batch_device" if mode == "device" else "ILUTPreconditioner_batch"
    real, routes = getattr(_native, name), []

    def spy(ms, is_csr, fill_in, threshold):
        return real(ms, is_csr, fill_in, threshold, routes)

    setattr(_native, name, spy)
    try:
        if mode == "device":
            members = ild.ilut_batch([_dev(A) for A in mats], fill_in=fill, threshold=tau)
        else:
            members = ilupp.ILUTPreconditioner.batch([A.tocsc() if mode == "host-csc" else A for A in mats], fill_in=fill, threshold=tau)
    finally:
        setattr(_native, name, real)
    return members, routes


def _build_single(mode, A, fill, tau):
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    if mode == "device":
        return ild.DevicePreconditioner("ILUT", _dev(A), fill_in=fill, threshold=tau)
    return ilupp.ILUTPreconditioner(A.tocsc() if mode == "host-csc" else A, fill_in=fill, threshold=tau)


def _compare(mode, mats, fill, tau, members, what):
    """every member against the singly built object of the same matrix: factors, total_nnz, the three applies"""
    for k, (A, M) in enumerate(zip(mats, members)):
        T = _build_single(mode, A, fill, tau)
        tag = (what, mode, fill, tau, k, A.shape[0])
        assert _same_factors(_factors(M), _factors(T)), tag
        assert M.pr.total_nnz == T.pr.total_nnz, tag
        assert all(f[3] == (mode != "host-csc") for f in _factors(M)), tag
        for a, b in zip(_three_applies(M, A.shape[0], k), _three_applies(T, A.shape[0], k)):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), tag


# ---- 1. the ticket map ----
@pytest.mark.parametrize("fill,tau", PARAMS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(TICKET_CASES))
def test_ticket_map(case, mode, fill, tau):
    sizes = TICKET_CASES[case]
    mats = [_random(n, 7000 + 31 * k + fill) for k, n in enumerate(sizes)]
    members, routes = _build_batch(mode, mats, fill, tau)
    assert routes == [0] * len(sizes), (case, mode, routes)
    assert [M.pr.path() for M in members] == [BATCH] * len(sizes)
    _compare(mode, mats, fill, tau, members, case)
    assert [M.pr.path() for M in members] == [BATCH] * len(sizes)          # (factors() and the applies leave it what it is)
    # the rows launches' time, shared by the call's members
    t = [M.pr.timings() for M in members]
    assert t[0]["numeric_ms"] > 0 and all(x["numeric_ms"] == t[0]["numeric_ms"] for x in t)


# ---- 2. members whose slabs have different pitches ----
@pytest.mark.parametrize("mode", MODES)
def test_differing_slab_pitch(mode):
    """fill_in = 100: p clamps to n = 7, equals n = 100, and is the budget itself at n = 101 and 300 -- the first member runs in the
    small LDS class, the others in the large one: two rows launches in one call"""
    sizes = [7, 100, 101, 300]
    mats = [_random(n, 7300 + k) for k, n in enumerate(sizes)]
    members, routes = _build_batch(mode, mats, 100, 0.1)
    assert routes == [0, 0, 0, 0] and [M.pr.path() for M in members] == [BATCH] * 4
    _compare(mode, mats, 100, 0.1, members, "pitch")
    members, routes = _build_batch(mode, mats, 100, 0.0)                  # (nothing dropped by the threshold: rows as long as the budget allows)
    assert routes == [0, 0, 0, 0]
    _compare(mode, mats, 100, 0.0, members, "pitch, tau = 0")


# ---- 3. the tier ladder inside a batch ----
def _groups():
    g = {}
    for name, c in C.CASES.items():
        g.setdefault((c.p, c.tau), []).append(name)
    return g


GROUPS = _groups()


@functools.lru_cache(maxsize=None)
def _random_member(p, tau):
    """the plain member every group gets: its matrix, the oracle's factors and the model's rows (computed once per parameter set)"""
    from oracle import oracle as O
    A = _random(65, 7500)
    orc = O.orc()
    Lo, Uo = orc.ilut((A.data.astype(np.float64), A.indices.astype(np.int32), A.indptr.astype(np.int32), True), p, tau)
    rows = R.ilut(A.indptr, A.indices, A.data, p, tau, orc.sort_slots_by_abs_desc)[2]
    return A, Lo, Uo, rows


@pytest.mark.parametrize("key", list(GROUPS), ids=["p%d_tau%g" % k for k in GROUPS])
def test_tier_ladder(key):
    """the cases of ilut_cases that share a parameter set, and one random member, as ONE batch in the device mode: rows that outgrow
    tier 1, rows that move to tier 3 and rows that give up run next to plain members on shared waves.  Every member has the oracle's
    bits; a launched member's tier counters are what ilut_ref predicts for it, and so is their sum over the group"""
    import test_gpu_ilut_tiers as T
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    p, tau = key
    names = GROUPS[key]
    A_r, Lo_r, Uo_r, rows_r = _random_member(p, tau)
    mats = [C.matrix(name) for name in names] + [A_r]
    want = [T._expected(name, "csr")[:2] for name in names] + [(Lo_r, Uo_r)]
    rows = [T._rows(name) for name in names] + [rows_r]
    routes = []
    dAs = [_dev(A) for A in mats]
    ild._on_current_stream()
    with _Env(ILUPP_DEBUG="1"), _Stderr() as cap:
        natives = _native.ILUTPreconditioner_batch_device(
            [(d.data.data_ptr(), d.indices.data_ptr(), d.indptr.data_ptr(), d.n, d.nnz) for d in dAs], True, p, tau, routes)
    seen = {int(m[0]): tuple(int(v) for v in m[1:]) for m in _RE_MEMBER.findall(cap.err)}
    total_seen, total_want = np.zeros(5, dtype=np.int64), np.zeros(5, dtype=np.int64)
    for k, (A, pr, (Lo, Uo)) in enumerate(zip(mats, natives, want)):
        tag = (key, (names + ["random"])[k])
        n = A.shape[0]
        predicted, _ = R.route(rows[k], n, p)
        F = pr.factors_info()
        for f, Fo in zip(F, (Lo, Uo)):
            assert np.array_equal(f[2], Fo[2]) and np.array_equal(f[1], Fo[1]), tag + ("pattern",)
            assert np.array_equal(_bits(f[0]), _bits(Fo[0])), tag + ("values",)
        assert pr.total_nnz == int(Lo[2][-1]) + int(Uo[2][-1]) - n, tag
        if predicted[0] is None:
            # the largest capacity class at once: never in the launch
            assert routes[k] == 1 and k not in seen and pr.path() == "ilut", tag + (routes[k],)
            continue
        assert k in seen, tag + ("no line of the launch",)
        outgrew, of_n, pool, uslots, kept, left2, status = seen[k]
        assert of_n == n and (outgrew, pool, uslots, kept, left2, status) == predicted[:6], tag + (seen[k], predicted)
        assert routes[k] == (1 if status == 3 else 0) and pr.path() == ("ilut" if status == 3 else BATCH), tag
        total_seen += (outgrew, pool, uslots, kept, left2)
        total_want += predicted[:5]
    assert np.array_equal(total_seen, total_want), (key, total_seen, total_want)
    if len(mats) > 1 and R.route(rows_r, 65, p)[0][0] is not None:
        assert routes[-1] == 0                                          # (the plain member is built by the launch whatever its neighbours do)


# ---- 4. route 1 ----
def test_a_batch_of_one_is_the_single_constructor_s_object():
    A = _random(300, 7600)
    for mode in MODES:
        members, routes = _build_batch(mode, [A], 10, 1e-4)
        assert routes == [1] and members[0].pr.path() == "ilut"
        _compare(mode, [A], 10, 1e-4, members, "one")


def test_budget_of_the_largest_class_goes_to_the_single_constructor():
    """fill_in = 300 at n = 320: p - 1 >= 256, the selection queue of the launch's LDS classes does not hold it"""
    mats = [_random(320, 7610), _random(320, 7611)]
    for mode in ("host", "device"):
        members, routes = _build_batch(mode, mats, 300, 0.0)
        assert routes == [1, 1] and [M.pr.path() for M in members] == ["ilut"] * 2
        _compare(mode, mats, 300, 0.0, members, "largest class")
    # (the same budget clamped by n = 200 stays in the launch)
    small = [_random(200, 7612), _random(200, 7613)]
    members, routes = _build_batch("device", small, 300, 0.0)
    assert routes == [0, 0]
    _compare("device", small, 300, 0.0, members, "clamped")


STATUS3 = [name for name, c in C.CASES.items() if c.route[5] == 3]


def test_status_3_member_is_rebuilt_by_the_single_constructor():
    """a member with a row that outgrows the 64 K pieces next to a plain one: route 1 for the first, route 0 for its neighbour"""
    small = [name for name in STATUS3 if C.matrix(name).shape[0] <= 40000]
    if not small:
        pytest.skip("ilut_cases has no status-3 case of n <= 40 000: %s" % STATUS3)
    import test_gpu_ilut_tiers as T
    name = min(small, key=lambda s: C.matrix(s).shape[0])
    c = C.CASES[name]
    mats = [_random(65, 7620), C.matrix(name)]
    members, routes = _build_batch("device", mats, c.p, c.tau)
    assert routes == [0, 1] and [M.pr.path() for M in members] == [BATCH, "ilut"]
    Lo, Uo = T._expected(name, "csr")[:2]
    for f, Fo in zip(_factors(members[1]), (Lo, Uo)):
        assert np.array_equal(f[2], Fo[2]) and np.array_equal(f[1], Fo[1]) and np.array_equal(_bits(f[0]), _bits(Fo[0])), name
    T0 = _build_single("device", mats[0], c.p, c.tau)
    assert _same_factors(_factors(members[0]), _factors(T0))


# ---- 5. exact zeros ----
def test_an_entry_cancelled_to_exact_zero_is_absent():
    """row 1 = (1, 3, 1) under row 0 = (2, 0, 2): l_10 = 0.5 and u_12 = 1 - 0.5 * 2 = 0.0 exactly -- no entry of the factor"""
    n = 40
    A = sp.lil_matrix((n, n))
    A.setdiag(4.0)
    A[0, 0], A[0, 2] = 2.0, 2.0
    A[1, 0], A[1, 1], A[1, 2] = 1.0, 3.0, 1.0
    A[5, 1], A[5, 2] = 1.0, 1.0
    A = A.tocsr(); A.sort_indices()
    mats = [_random(65, 7700), A, _random(40, 7701)]
    for mode in MODES:
        members, routes = _build_batch(mode, mats, 10, 0.0)
        assert routes == [0, 0, 0]
        T = _build_single(mode, A, 10, 0.0)
        assert _same_factors(_factors(members[1]), _factors(T)), mode
        if mode != "host-csc":
            U = _factors(members[1])[1]
            assert list(U[1][U[2][1]:U[2][2]]) == [1], (mode, U[1][U[2][1]:U[2][2]])      # row 1 of U: the pivot alone
            assert np.all(U[0] != 0.0) and np.all(_factors(members[1])[0][0] != 0.0)


# ---- 6. failure ----
def _zero_pivot(n, r):
    """row r = (1 at column 0, 1 at column r) under row 0 = (1 at column 0, 1 at column r): w_rr = 1 - 1 * 1 = 0"""
    A = sp.lil_matrix((n, n))
    A.setdiag(2.0)
    A[0, 0], A[0, r] = 1.0, 1.0
    A[r, 0], A[r, r] = 1.0, 1.0
    A = A.tocsr(); A.sort_indices()
    return A


def test_zero_pivot_fails_as_the_single_constructor_does():
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    good = [_random(65, 7800), _random(300, 7801)]
    bad = _zero_pivot(257, 5)
    with pytest.raises(RuntimeError, match="ILUT_heap: encountered zero pivot in row 5") as single:
        ild.DevicePreconditioner("ILUT", _dev(bad), fill_in=10, threshold=1e-4)
    assert str(single.value) == "ILUT_heap: encountered zero pivot in row 5"
    live = _native.live_blocks()
    for mode in MODES:
        got = None
        with pytest.raises(RuntimeError, match="^matrix 1 of the batch: ILUT_heap: encountered zero pivot in row 5") as batch:
            got = _build_batch(mode, [good[0], bad, good[1]], 10, 1e-4)
        assert got is None and type(batch.value) is type(single.value)
        assert _native.live_blocks() == live, mode                       # (every object of the failed call is gone)
        members, routes = _build_batch(mode, good, 10, 1e-4)             # (a following batch of the good members succeeds)
        assert routes == [0, 0]
        _compare(mode, good, 10, 1e-4, members, "after a failure")
        del members
        assert _native.live_blocks() == live, mode


# ---- 7. downstream ----
@pytest.mark.parametrize("mode", ["host", "device"])
def test_members_go_into_the_batched_apply_and_bicgstab(mode):
    import torch
    import ilupp_amd.device as ild
    ns = [300] * 8
    mats = [_random(n, 7900 + k) for k, n in enumerate(ns)]
    dAs = [_dev(A) for A in mats]
    offsets = [int(v) for v in np.cumsum([0] + ns[:-1])]
    total = sum(ns)
    wrap = (lambda M: M) if mode == "device" else (lambda M: ild.FactorOperator(M))
    x0 = torch.from_numpy(_rhs(total, 5)).cuda()
    outs = []
    for build in ("batch", "batch", "single"):
        if build == "batch":
            members, routes = _build_batch(mode, mats, 10, 1e-4)
            assert routes == [0] * 8
        else:
            members = [_build_single(mode, A, 10, 1e-4) for A in mats]
        Ms = [wrap(M) for M in members]
        res = []
        for tr in (False, True):
            x = x0.clone()
            r = ild.apply_batch_(Ms, x, offsets, transpose=tr)
            assert list(r) == [0] * 8
            res.append(x.cpu().numpy())
        stats = {}
        y = ild.bicgstab_batch(dAs, x0, offsets, Ms, maxiter=5, stats=stats)
        assert list(stats["route"]) == [0] * 8 and list(stats["iterations"]) == [5] * 8
        res.append(y.cpu().numpy())
        if build == "batch":
            assert [M.pr.path() for M in members] == [BATCH] * 8
        outs.append(res)
    for k, what in enumerate(("apply_batch_", "apply_batch_ transposed", "bicgstab_batch")):
        assert np.all(np.isfinite(outs[0][k])), what
        assert np.array_equal(_bits(outs[0][k]), _bits(outs[1][k])), (what, "the same batch built twice")
        assert np.array_equal(_bits(outs[0][k]), _bits(outs[2][k])), (what, "singly built members")
