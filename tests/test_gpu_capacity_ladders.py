"""The capacity ladders of ILUC, partial ILUC and ICholT on the GPU: which class produced a result, not only the result.  Every case
(tests/capacity_cases.py) is compared bit for bit with the oracle -- index arrays, values as uint64, apply and apply_trans, both input
orientations -- and asserts the ROUTE, the list of (class, status) attempts parsed from the ILUPP_DEBUG lines on stderr, against the CPU
model of the per-step demands: rows exactly on a capacity, rows one past it, every hop of every ladder (each a restart on pool blocks a
half-finished attempt just gave back), every class forced, the errors of the reference from upper classes, the refusals past the largest
class."""
import os
import re
import time

import numpy as np
import pytest
import scipy.sparse as sp

import capacity_cases as K
import matgen
import ml_cases as C

pytestmark = pytest.mark.gpu

_RE = {
    "iluc": re.compile(r"\[ilupp\] iluc: class (\d+), T (\d+), waves (\d+): status (-?\d+)"),
    "icholt": re.compile(r"\[ilupp\] icholt: class (\d+), T (\d+), waves (\d+): status (-?\d+)"),
}
_RE_PILUC = re.compile(r"\[ilupp\] piluc: n (\d+) class (\d+) \(slots (\d+)\) T (\d+) waves (\d+) store (\d+): status (-?\d+)")
_RE_SCHUR = re.compile(r"\[ilupp\] piluc: Schur rows (\d+): status (-?\d+)")
_RE_CHAIN = re.compile(r"\[ilupp\] piluc \(chain[^)]*\): n (\d+), launch (\d+) .*: status (-?\d+)")


class _Env:
    """environment variables set around a call (the library reads them per call)"""

    def __init__(self, **kw):
        self.kw = {k: v for k, v in kw.items() if v is not None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update({k: str(v) for k, v in self.kw.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _traced(capfd, f, **env):
    """f() under ILUPP_DEBUG and `env`: (result or the exception it raised, stderr)"""
    capfd.readouterr()
    out = None
    with _Env(ILUPP_DEBUG=1, **env):
        try:
            out = f()
        except (RuntimeError, NotImplementedError) as e:
            out = e
    return out, capfd.readouterr().err


def _route(err, family):
    return [(int(m.group(1)), int(m.group(4))) for m in _RE[family].finditer(err)]


def _cause(status):
    return None if status == 0 else (K.RECORDS if status in (12, 15) else (K.ENTRIES if status in (11, 13, 14) else "status %d" % status))


def _oracle():
    from oracle import oracle as O
    return O.ref() if O.ref_available() else O.orc()


def _bits(F, Fo, what):
    """a factor of the package (scipy) against the oracle's (data, indices, indptr, is_csr): bit for bit"""
    assert isinstance(F, sp.csr_matrix) == bool(Fo[3]), what
    assert np.array_equal(F.indptr, Fo[2]) and np.array_equal(F.indices, Fo[1]), what
    assert np.array_equal(np.ascontiguousarray(F.data).view(np.uint64), np.ascontiguousarray(Fo[0]).view(np.uint64)), what


def _same_vec(x, y, what):
    assert np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)), what


def _orientations(A):
    """the matrix as row input, and the column input that hands the kernel the SAME major-order view (the CSC arrays of A^T are the CSR
    arrays of A): the same demands and the same route, through the other labelling of the inputs and of the results"""
    A = sp.csr_matrix(A); A.sort_indices()
    T = A.T.tocsc(); T.sort_indices()
    return (("csr", A), ("csc", T))


# =====================================================================================================================================
# ILUC
# =====================================================================================================================================
_iluc_oracle = {}


def _iluc_expected(key, M, fill):
    """the oracle's factors and applies of a case, computed once and left unchanged"""
    from oracle import oracle as O
    if key not in _iluc_oracle:
        Lo, Uo = _oracle().iluc(K.as_input(M), fill, 0.0)
        b = C.rhs(M.shape[0])
        _iluc_oracle[key] = (Lo, Uo, b, O.orc().apply_lu(Lo, Uo, b, O.ID), O.orc().apply_lu(Lo, Uo, b, O.TRANSPOSE))
    return _iluc_oracle[key]


def _iluc_run(capfd, name, A, fill, expected, force=None):
    """factorise in both orientations: the oracle's bits, and the route `expected` = [(class, cause or None)]"""
    import ilupp_amd as ilupp
    for fmt, M in _orientations(A):
        Lo, Uo, b, xo, xto = _iluc_expected((name, fmt), M, fill)
        P, err = _traced(capfd, lambda: ilupp.ILUCPreconditioner(M, fill_in=fill, threshold=0.0), ILUPP_ILUC_CLASS=force)
        seen = _route(err, "iluc")
        what = "%s (%s, forced %s): route seen %s, expected %s" % (name, fmt, force, seen, expected)
        assert [(c, _cause(s)) for c, s in seen] == [(c, cause) for c, cause in expected], what
        assert not isinstance(P, Exception), (what, P)
        L, U = P.factors()
        _bits(L, Lo, what); _bits(U, Uo, what)
        x = b.copy(); P.apply(x); _same_vec(x, xo, what)
        x = b.copy(); P.apply_trans(x); _same_vec(x, xto, what)


@pytest.mark.parametrize("name", sorted(K.ILUC_TABLE) + sorted(K.ILUC_TWINS))
def test_iluc_routes(capfd, name):
    """the natural routes of the table and the edge twins (ILUPP_ILUC_CLASS where the natural start is lower than the class of the edge)"""
    from oracle import oracle as O
    A, fill, forced, classes = K.iluc_case(name)
    dem, deps, start, route = K.iluc_model(name, O.orc())
    assert route is not None and K.classes_of(route) == classes
    _iluc_run(capfd, name, A, fill, route, force=forced)


def _forced_cases():
    for name in sorted(K.ILUC_TABLE):
        for cls in range(5):
            yield name, cls


@pytest.mark.parametrize("name,cls", list(_forced_cases()))
def test_iluc_forced_into_every_class_that_holds_it(capfd, name, cls):
    """the same bits from every class that can hold the case; from a class that cannot, the ladder goes on from there"""
    from oracle import oracle as O
    A, fill, forced, classes = K.iluc_case(name)
    dem, deps, start, _ = K.iluc_model(name, O.orc())
    route = K.iluc_route(dem, deps, A.shape[0], cls)
    assert route is not None and route[0][0] == cls and route[-1][1] is None
    _iluc_run(capfd, name, A, fill, route, force=cls)


def test_iluc_zero_pivot_after_the_hop(capfd):
    """arrow_last(140) without the diagonal entries of rows 5 and 20: the steps above a missing pivot run on a stand-in, the attempt in
    class 0 stops on the records of the last row, and class 3 reports the reference's error: the smallest k"""
    import ilupp_amd as ilupp
    from oracle import oracle as O
    B = K.without_diagonal(K.arrow_last(140), (5, 20))
    for fmt, M in _orientations(B):
        with pytest.raises(O.OracleError) as eo:
            _oracle().iluc(K.as_input(M), 5, 0.0)
        assert eo.value.code == O.ERR_ZERO_PIVOT and eo.value.row == 5
        P, err = _traced(capfd, lambda: ilupp.ILUCPreconditioner(M, fill_in=5, threshold=0.0))
        seen = _route(err, "iluc")
        assert [(c, _cause(s)) for c, s in seen] == [(0, K.RECORDS), (3, None)], (fmt, seen)
        assert isinstance(P, RuntimeError) and "zero pivot" in str(P) and "k=5" in str(P), (fmt, P)


def test_iluc_memory_error_from_class_2(capfd):
    """dense first row and column, N = 60, fill 60: the factors fill completely and exceed the reference's reservation -- its "insufficient
    memory reserved", from the class the estimate starts in"""
    import ilupp_amd as ilupp
    from oracle import oracle as O
    F = K.arrow_first(60)
    for fmt, M in _orientations(F):
        with pytest.raises(O.OracleError) as eo:
            _oracle().iluc(K.as_input(M), 60, 0.0)
        assert eo.value.code == O.ERR_MEMORY
        P, err = _traced(capfd, lambda: ilupp.ILUCPreconditioner(M, fill_in=60, threshold=0.0))
        assert _route(err, "iluc") == [(2, 0)], (fmt, _route(err, "iluc"))
        assert isinstance(P, RuntimeError) and "insufficient memory reserved" in str(P), (fmt, P)


def test_iluc_largest_class_holds_16384_slots(capfd):
    """row_first(16384): the global class has 16 384 slots and A's part of step 0 fills every one"""
    t0 = time.perf_counter()
    A = K.row_first(16384)
    _iluc_run(capfd, "row_first_16384", A, 5, [(0, K.ENTRIES), (1, K.ENTRIES), (2, K.ENTRIES), (4, None)])
    print("row_first(16384), both orientations with the oracle: %.2f s" % (time.perf_counter() - t0))


def test_iluc_class_4_forced_on_a_long_row(capfd):
    """row_first(1023) started in the global class: 1 024 slots for 1 023 entries"""
    _iluc_run(capfd, "row_first_1023", K.row_first(1023, True), 5, [(4, None)], force=4)


def test_iluc_refuses_16385(capfd):
    """one entry more than the largest class holds: refused, never answered, never hung"""
    import ilupp_amd as ilupp
    A = K.row_first(16385)
    for fmt, M in _orientations(A):
        P, err = _traced(capfd, lambda: ilupp.ILUCPreconditioner(M, fill_in=5, threshold=0.0))
        seen = _route(err, "iluc")
        assert [(c, _cause(s)) for c, s in seen] == [(0, K.ENTRIES), (1, K.ENTRIES), (2, K.ENTRIES), (4, K.ENTRIES)], (fmt, seen)
        assert isinstance(P, NotImplementedError) and K.ILUC_REFUSAL in str(P), (fmt, P)


def test_iluc_hop_on_used_blocks(capfd):
    """every hop restarts on blocks the failed attempt gave back; here the blocks also hold the slabs and touch records of an older
    factorisation of the same n with large indices that completed in the target class (the scheme of test_error_path_on_reused_slabs)"""
    import ilupp_amd as ilupp
    from oracle import oracle as O
    rng = np.random.default_rng(11)
    for name in ("arrow_last_140", "row_first_600", "comb_119_8_7"):
        A, fill, forced, classes = K.iluc_case(name)
        n = A.shape[0]
        route = K.iluc_model(name, O.orc())[3]
        for _ in range(2):
            B = (sp.random(n, n, density=min(1.0, 6.0 / n), random_state=rng, format="csr") + sp.eye(n) * 4.0).tocsr()
            B.sort_indices()
            with _Env(ILUPP_ILUC_CLASS=classes[-1]):
                P = ilupp.ILUCPreconditioner(B, fill_in=fill, threshold=0.0)
            del P
            _iluc_run(capfd, name, A, fill, route)


# =====================================================================================================================================
# partial ILUC (the multilevel preconditioner without pivoting, no preprocessing, threshold 0: one level)
# =====================================================================================================================================
NOPRE = (0.0, (), {})
PQ = ("NORMALIZE_COLUMNS", "NORMALIZE_ROWS", "PQ_ORDERING")

PILUC_CASES = {
    # name -> (builder, forced class or None)
    "arrow_last_34": (lambda: K.arrow_last(34), None), "arrow_last_140": (lambda: K.arrow_last(140), None),
    "arrow_last_600": (lambda: K.arrow_last(600), None),
    "row_first_129": (lambda: K.row_first(129, True), None), "row_first_300": (lambda: K.row_first(300), None),
    "row_first_600": (lambda: K.row_first(600, True), None), "row_first_2500": (lambda: K.row_first(2500), None),
    "comb_31_8_7": (lambda: K.comb(31, 8, 7), None), "comb_31_8_8": (lambda: K.comb(31, 8, 8), None),
    "comb_63_12_11": (lambda: K.comb(63, 12, 11), 1), "comb_63_12_12": (lambda: K.comb(63, 12, 12), 1),
    "comb_127_8_7": (lambda: K.comb(127, 8, 7), 2), "comb_127_8_8": (lambda: K.comb(127, 8, 8), 2),
    "comb_95_8_7": (lambda: K.comb(95, 8, 7), 3), "comb_95_8_8": (lambda: K.comb(95, 8, 8), 3),
}
# the classes each case must try with the chain kernel switched off (the model reproduces them from the oracle's level)
PILUC_ROUTES = {
    "arrow_last_34": [0, 2], "arrow_last_140": [0, 2, 3], "arrow_last_600": [0, 2, 3, 4],
    "row_first_129": [0, 1], "row_first_300": [0, 1, 2], "row_first_600": [0, 1, 2, 4], "row_first_2500": [0, 1, 2, 4, 4],
    "comb_31_8_7": [0], "comb_31_8_8": [0, 1], "comb_63_12_11": [1], "comb_63_12_12": [1, 2], "comb_127_8_7": [2], "comb_127_8_8": [2, 4],
    "comb_95_8_7": [3], "comb_95_8_8": [3, 4],
}
_piluc_models = {}


def _piluc_expected(name):
    from oracle import oracle as O
    if name not in _piluc_models:
        A = PILUC_CASES[name][0]()
        Q = O.orc().ml(K.as_input(A), C.oracle_params(O, *NOPRE))
        assert Q.levels() == 1
        route = K.piluc_model(A, Q.level(0), PILUC_CASES[name][1])[3]
        assert route is not None and [c for c, _, _ in route] == PILUC_ROUTES[name], (name, route)
        _piluc_models[name] = (A, route)
    return _piluc_models[name]


def _piluc_attempts(err):
    """[(class, slots, store, status)] of the dataflow attempts, and the statuses of the chain kernel's launches"""
    return ([(int(m.group(2)), int(m.group(3)), int(m.group(6)), int(m.group(7))) for m in _RE_PILUC.finditer(err)],
            [int(m.group(3)) for m in _RE_CHAIN.finditer(err)])


def _without_store_growth(seen):
    """the attempts that did not end with "stores too small" (status 16).  The stores of a level start from 3 nnz + 2 n + 1024 entries per
    factor and the waves take them in chunks, so even a small level can run out: the same class comes again with twice the stores (four
    times in the global class).  The demand model knows nothing of stores; the rule is asserted here"""
    for a, b in zip(seen, seen[1:]):
        if a[3] == 16:
            assert b[0] == a[0] and b[1] == a[1] and b[2] == a[2] * (4 if a[0] == 4 else 2), seen
    assert not seen or seen[-1][3] != 16, seen
    return [a for a in seen if a[3] != 16]


def _ml_against_oracle(capfd, M, params, **env):
    from test_gpu_ml import _against_oracle
    capfd.readouterr()
    with _Env(ILUPP_DEBUG=1, **env):
        levels = _against_oracle(M, params)
    return levels, capfd.readouterr().err


@pytest.mark.parametrize("name", sorted(PILUC_CASES))
def test_piluc_routes_without_the_chain(capfd, name):
    """ILUPP_NO_PILUC_CHAIN=1: records 0 -> 2 -> 3 -> 4, entries or slots 0 -> 1 -> 2 -> 4; the global class starts with 2 048 slots and
    comes again with 8 192"""
    A, route = _piluc_expected(name)
    # (the multilevel construction turns column input into row storage of the same matrix: the same view, the same route)
    for fmt, M in (("csr", A), ("csc", A.tocsc())):
        _, err = _ml_against_oracle(capfd, M, NOPRE, ILUPP_NO_PILUC_CHAIN=1, ILUPP_PILUC_CLASS=PILUC_CASES[name][1])
        seen, chain = _piluc_attempts(err)
        what = "%s (%s): route seen %s, expected %s" % (name, fmt, seen, route)
        assert [(c, g, _cause(s)) for c, g, _, s in _without_store_growth(seen)] == route, what
        assert chain == [], what


@pytest.mark.parametrize("mem_chain_off", [False, True])
@pytest.mark.parametrize("name", sorted(n for n in PILUC_CASES if PILUC_ROUTES[n][-1] == 4))
def test_piluc_routes_with_the_chain(capfd, name, mem_chain_off):
    """without the switch the ladder hands over to the chain kernel where it would enter the global class: the same classes below it, the
    same bits.  ILUPP_NO_PILUC_MEM_CHAIN=1 keeps the chain's vectors in LDS: what does not fit there comes back to the global class"""
    A, route = _piluc_expected(name)
    below = [(c, g, cause) for c, g, cause in route if c < 4]
    _, err = _ml_against_oracle(capfd, A, NOPRE, ILUPP_PILUC_CLASS=PILUC_CASES[name][1], ILUPP_NO_PILUC_MEM_CHAIN=1 if mem_chain_off else None)
    seen, chain = _piluc_attempts(err)
    what = "%s: route seen %s + chain %s, expected %s + chain" % (name, seen, chain, below)
    assert [(c, g, _cause(s)) for c, g, _, s in _without_store_growth(seen) if c < 4] == below, what
    assert len(chain) >= 1, what
    if chain[-1] == 0:
        assert all(c < 4 for c, _, _, _ in seen), what                  # (the chain completed: the global class never ran)
    else:
        assert seen[-1][0] == 4 and seen[-1][3] == 0, what


@pytest.mark.parametrize("knobs", [{}, {"fill_in": 6}], ids=["unbounded", "fill6"])
@pytest.mark.parametrize("cls", [0, 1, 2, 3, 4])
def test_piluc_every_class_on_many_levels(capfd, cls, knobs):
    """weak diagonals: five levels and more, every level but the last with a Schur complement -- the elimination launch and the Schur launch
    of k_piluc_df in every class, every level against the oracle"""
    A = C.weak_random(700, 0.01, 0.3, 7)
    levels, err = _ml_against_oracle(capfd, A, (0.05, PQ, knobs), ILUPP_PILUC_CLASS=cls, ILUPP_NO_PILUC_CHAIN=1)
    seen, chain = _piluc_attempts(err)
    assert levels >= 5 and chain == []
    # one ladder per level: it starts in the forced class, every hop is the one piluc_level makes for the code seen, and it ends with status 0
    ladders, cur = [], []
    for a in _without_store_growth(seen):
        cur.append(a)
        if a[3] == 0:
            ladders.append(cur); cur = []
    assert cur == [] and levels - 1 <= len(ladders) <= levels, (cls, seen)
    for lad in ladders:
        assert lad[0][0] == cls, (cls, lad)
        for a, b in zip(lad, lad[1:]):
            if a[0] < 4:
                assert _cause(a[3]) in (K.RECORDS, K.ENTRIES) and b[0] == K.piluc_next(a[0], _cause(a[3])), (cls, lad)
            else:
                assert b[0] == 4 and _cause(a[3]) == K.ENTRIES and (b[1] == 4 * a[1] or b[1] == a[1]), (cls, lad)
    if "fill_in" in knobs:
        # (bounded fill keeps the rows of the Schur complements short: every level completes in the class it is started in, so both
        #  launches of k_piluc_df ran in class `cls`)
        assert all(len(lad) == 1 for lad in ladders), (cls, ladders)
    schur = [int(m.group(2)) for m in _RE_SCHUR.finditer(err)]
    assert schur.count(0) >= levels - 1, (cls, schur)


def test_piluc_store_doubling(capfd):
    """exact factors of a random matrix exceed the stores a level starts with (3 nnz + 2 n + 1024).  On its natural route the matrix leaves
    the LDS classes on entries before the stores run out, and the hop to the global class raises the stores to 16 nnz + 8 n + 1024, which
    hold it: no status 16 there.  Started IN the global class the stores are the small ones: status 16, the same class again with four times
    the stores, until the factors fit"""
    from oracle import oracle as O
    d, i, p = matgen.random_dd(300, k=9)
    A = sp.csr_matrix((d, i, p), shape=(300, 300))
    first = 3 * A.nnz + 2 * 300 + 1024
    Q = O.orc().ml(K.as_input(A), C.oracle_params(O, *NOPRE))
    assert Q.levels() == 1 and Q.level(0)["U"][2][-1] > first and Q.level(0)["L"][2][-1] > first
    _, err = _ml_against_oracle(capfd, A, NOPRE, ILUPP_NO_PILUC_CHAIN=1)
    seen, _ = _piluc_attempts(err)
    print("natural route (class, slots, store, status):", seen)
    route = K.piluc_model(A, Q.level(0))[3]
    assert route is not None and [c for c, _, _ in route] == [0, 1, 2, 4]
    assert [(c, g, _cause(s)) for c, g, _, s in _without_store_growth(seen)] == route, (seen, route)
    assert seen[0][2] == first and seen[-1][2] >= 16 * A.nnz + 8 * 300 + 1024, seen
    _, err = _ml_against_oracle(capfd, A, NOPRE, ILUPP_NO_PILUC_CHAIN=1, ILUPP_PILUC_CLASS=4)
    seen, _ = _piluc_attempts(err)
    print("started in the global class (class, slots, store, status):", seen)
    assert seen[0][:3] == (4, 2048, first) and seen[0][3] == 16 and seen[-1][3] == 0, seen
    assert [a[0] for a in _without_store_growth(seen)] == [4], seen
    assert seen[-1][2] == first * 4 ** (len(seen) - 1) and seen[-1][2] > Q.level(0)["U"][2][-1], seen


def test_piluc_hop_on_used_blocks(capfd):
    import ilupp_amd as ilupp
    from test_gpu_ml import _native_ml
    rng = np.random.default_rng(12)
    for name in ("arrow_last_140", "row_first_300"):
        A, route = _piluc_expected(name)
        n = A.shape[0]
        for _ in range(2):
            B = (sp.random(n, n, density=min(1.0, 6.0 / n), random_state=rng, format="csr") + sp.eye(n) * 4.0).tocsr()
            with _Env(ILUPP_PILUC_CLASS=route[-1][0], ILUPP_NO_PILUC_CHAIN=1):
                P = _native_ml(B, C.engine_params(ilupp, *NOPRE))
            del P
            _, err = _ml_against_oracle(capfd, A, NOPRE, ILUPP_NO_PILUC_CHAIN=1)
            seen, _ = _piluc_attempts(err)
            assert [(c, g, _cause(s)) for c, g, _, s in _without_store_growth(seen)] == route, (name, seen, route)


# =====================================================================================================================================
# ICholT
# =====================================================================================================================================
def _spd_from(d, i, p, shift):
    ds, is_, ps = matgen.symmetrize(d, i, p)
    n = ps.shape[0] - 1
    S = (sp.csr_matrix((ds, is_, ps), shape=(n, n)) + shift * sp.identity(n, format="csr")).tocsr()
    S.sort_indices()
    return S


def _icholt_seeded(case):
    """the five matrices of test_gpu_parity.test_icholt_dataflow_vs_oracle_seeded with the smallest of their parameters"""
    if case == "grid_40":
        d, i, p = matgen.poisson3d(40)
    elif case == "grid_ragged":
        d, i, p = matgen.poisson3d(23, 9, 31)
    elif case == "rand_spd":
        return _spd_from(*matgen.random_dd(4000, 9, 0.0, 21), 12.0)
    elif case == "rand_spd_dense_rows":
        return _spd_from(*matgen.random_dd(600, 40, 0.0, 5), 60.0)
    else:
        d, i, p = matgen.laplace1d(3000)
    n = p.shape[0] - 1
    return sp.csr_matrix((d, i, p), shape=(n, n))


def _icholt_run(capfd, A, fill, tau, expected, force=None, formats=("csr", "csc")):
    """ICholT against the oracle, bit for bit, and the route [(class, status)]; expected None: returned, not asserted"""
    import ilupp_amd as ilupp
    from oracle import oracle as O
    A = sp.csr_matrix(A); A.sort_indices()
    b = C.rhs(A.shape[0])
    seen = None
    for fmt in formats:
        M = A if fmt == "csr" else A.tocsc()
        Lo = O.orc().icholt(K.as_input(M), fill, tau)
        P, err = _traced(capfd, lambda: ilupp.ICholTPreconditioner(M, add_fill_in=fill, threshold=tau), ILUPP_ICHOLT_CLASS=force)
        seen = _route(err, "icholt")
        what = "ICholT (%s, forced %s): route seen %s, expected %s" % (fmt, force, seen, expected)
        if expected is not None:
            assert seen == expected, what
        assert not isinstance(P, Exception), (what, P)
        L, = P.factors()
        _bits(L, Lo, what)
        x = b.copy(); P.apply(x); _same_vec(x, O.orc().apply_llt(Lo, b, O.ID), what)
        x = b.copy(); P.apply_trans(x); _same_vec(x, O.orc().apply_llt(Lo, b, O.TRANSPOSE), what)
    return seen


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("case", ["grid_40", "grid_ragged", "rand_spd", "rand_spd_dense_rows", "chain"])
def test_icholt_forced_classes(capfd, case, cls):
    """ILUPP_ICHOLT_CLASS = 1 and 2 as A/B: the ladder starts there and the bits are the oracle's"""
    seen = _icholt_run(capfd, _icholt_seeded(case), 0, 0.0, None, force=cls, formats=("csr",))
    assert seen[0][0] == cls and seen[-1][1] == 0 and [c for c, _ in seen] == list(range(cls, cls + len(seen))), (case, cls, seen)
    if case in ("grid_40", "grid_ragged", "chain"):
        # (7-point stencils and a chain without fill: columns of a few entries, reached by a few -- every class holds them)
        assert seen == [(cls, 0)], (case, cls, seen)


def test_icholt_arrow_on_the_record_capacity(capfd):
    """T = 16 in classes 0..2 for these short average rows; spd_arrow_last(N)'s last row is reached by N - 1 columns"""
    assert K.icholt_T(2 * 17 - 1, 17, 0, 0) == 16
    _icholt_run(capfd, K.spd_arrow_last(17), 0, 0.0, [(0, 0)])
    _icholt_run(capfd, K.spd_arrow_last(18), 0, 0.0, [(0, 1), (1, 1), (2, 1), (3, 0)])


def test_icholt_2048_rows_in_a_column(capfd):
    """a column with 2 048 rows fills the slots of the largest class.  With threshold 0 every later column gathers what is left of that
    column and the 2 048 dependent steps take 6.3 s per factorisation in the one-wave-per-CU class; threshold 0.01 drops the column's
    off-diagonal entries (0.5 / sqrt(2048) against a norm of sqrt(2048)) after the step has gathered, hashed and ranked all 2 048 slots,
    and the rest is a diagonal"""
    _icholt_run(capfd, K.spd_arrow_first(2048), 0, 0.01, [(0, 1), (1, 1), (2, 1), (3, 0)])


@pytest.mark.parametrize("fill", [0, 3])
def test_icholt_refuses_2049_rows_in_a_column(capfd, fill):
    import ilupp_amd as ilupp
    A = K.spd_arrow_first(2049)
    P, err = _traced(capfd, lambda: ilupp.ICholTPreconditioner(A, add_fill_in=fill, threshold=0.0))
    seen = _route(err, "icholt")
    assert seen == [(0, 1), (1, 1), (2, 1), (3, 1)], seen
    assert isinstance(P, RuntimeError) and "largest capacity class" in str(P), P


@pytest.mark.parametrize("params", [(0, 0.0), (30, 1e-8)])
def test_icholt_dense_rows_route(capfd, params):
    """rand_spd_dense_rows of the seeded test: the triangle has 41 entries per column, so T = 4 (41 + fill) is cut to 128 and classes 0
    and 1 (32 and 64 records) refuse before they launch; a column gathers the tails of some forty stored columns of some forty entries,
    so the pre-drop columns cover most of the 600 rows, a late row is reached by hundreds of them, and class 2 (128 records) stops;
    the largest class has a record for every column"""
    A = _icholt_seeded("rand_spd_dense_rows")
    tri = sp.tril(A).nnz
    assert K.icholt_T(tri, 600, params[0], 0) is None and K.icholt_T(tri, 600, params[0], 1) is None and K.icholt_T(tri, 600, params[0], 2) == 128
    _icholt_run(capfd, A, params[0], params[1], [(0, 1), (1, 1), (2, 1), (3, 0)])


def test_icholt_hop_on_used_blocks(capfd):
    import ilupp_amd as ilupp
    rng = np.random.default_rng(13)
    for _ in range(2):
        R = sp.random(18, 18, density=0.4, random_state=rng, format="csr")
        B = (R + R.T + sp.eye(18) * 40.0).tocsr()
        with _Env(ILUPP_ICHOLT_CLASS=3):
            P = ilupp.ICholTPreconditioner(B, add_fill_in=0, threshold=0.0)
        del P
        _icholt_run(capfd, K.spd_arrow_last(18), 0, 0.0, [(0, 1), (1, 1), (2, 1), (3, 0)])
