"""The CPU model of the CSR sweep family (tests/sweep_ref.py) checked without a GPU, and the figures that put every case of
tests/sweep_cases.py at its edge, stated by hand: a change to a builder cannot silently move a case off its edge.

Tolerances.  Float64 model against the longdouble sweep and against scipy: nothing measured.  The computed x^ of a substitution satisfies,
row by row, |b - T x^|_r <= gamma_k (|T| |x^|)_r with k the entries of row r, u = 2^-53 and gamma_k = k u / (1 - k u) (the standard
backward-error bound), evaluated in longdouble.  Since x - x^ = T^-1 (b - T x^), two computed solutions
x1, x2 that both satisfy that bound differ componentwise by at most |T^-1| (gamma |T| |x1| + gamma |T| |x2|): the bound between the model and
its longdouble twin and between the model and scipy's spsolve_triangular.  It holds for substitution in any order of summation; a solver that
does not divide by the diagonal (scipy 1.15 multiplies a diagonal triangle's right-hand side by reciprocals: its own residual is up to 1.6
gamma_1 there) has no claim on it, and if such a case exceeds it that is a finding, not a reason to widen it."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import golden_util as G
import level_ref
import sweep_cases as C
import sweep_ref as R

FWD = {"lu": {0: True, 1: False, 2: True, 3: False}, "ichol0": {0: True, 3: False}, "icholt": {0: False, 3: True}}
KIND = {"lu": {0: 0, 1: 1, 2: 0, 3: 2}, "ichol0": {0: 0, 3: 2}, "icholt": {0: 1, 3: 0}}


def _orc():
    from oracle import oracle as O
    return O, O.orc()


@functools.lru_cache(maxsize=None)
def _factors(name):
    return C.factors(_orc()[1], name)


def _fac(M):
    return (M.data, M.indices, M.indptr, sp.isspmatrix_csr(M))


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------------
SMALL = ("rows16", "rows17-up", "rows1_16", "dense8", "chain33", "chain100", "chol0-band", "cholt-band", "one")


def _gamma_rows(T):
    ld = np.longdouble
    k = np.diff(T.indptr).astype(ld)
    u = ld(2.0) ** -53
    return k * u / (1 - k * u)


def _difference_bound(T, x1, x2):
    """|T^-1| (gamma |T| |x1| + gamma |T| |x2|) in longdouble (dense: the cases here have n <= 300)"""
    ld = np.longdouble
    A = np.abs(T.toarray().astype(ld))
    n = A.shape[0]
    # |T^-1| by substitution on the identity, in longdouble (numpy's inverse is float64 only)
    Td = T.toarray().astype(ld)
    inv = np.zeros((n, n), dtype=ld)
    lower = sp.tril(T, -1).nnz > 0 or sp.triu(T, 1).nnz == 0
    order = range(n) if lower else range(n - 1, -1, -1)
    for r in order:
        e = np.zeros(n, dtype=ld); e[r] = 1
        inv[r] = (e - Td[r] @ inv + Td[r, r] * inv[r]) / Td[r, r]
    g = _gamma_rows(T)
    rhs = g * (A @ np.abs(x1.astype(ld))) + g * (A @ np.abs(x2.astype(ld)))
    return np.abs(inv) @ rhs


@pytest.mark.parametrize("name", SMALL)
def test_sweep_against_scipy_and_longdouble(name):
    cls, L, U = _factors(name)
    S = R.stored(cls, L, U)
    for slot, T in S.items():
        kind = KIND[cls][slot]
        b = G.rhs(T.shape[0])
        x = R.sweep(T, b, kind)
        ok, worst = R.backward_error_ok(T, x, b, kind)
        assert ok, (name, slot, worst)
        Ts = T.copy(); Ts.sort_indices()
        xs = spla.spsolve_triangular(Ts, b, lower=FWD[cls][slot])
        xl = R.sweep_long(T, b, kind)
        assert xl.dtype == np.longdouble
        ld = np.longdouble
        assert np.all(np.abs(x.astype(ld) - xs.astype(ld)) <= _difference_bound(T, x, xs)), (name, slot, "scipy")
        assert np.all(np.abs(x.astype(ld) - xl) <= _difference_bound(T, x, xl)), (name, slot, "longdouble")
        off = xs * (1 + 2.0 ** -48)                 # (a solution 32 units of roundoff away is told apart)
        assert not np.all(np.abs(x.astype(ld) - off.astype(ld)) <= _difference_bound(T, x, off)), (name, slot, "a perturbed vector passes")


def test_special_values():
    """-0.0, +-inf and NaN go through the model as IEEE says; a NaN result is the one canonical NaN; a row without entries gives NaN"""
    T = sp.csr_matrix(np.array([[2.0, 0, 0], [1.0, -4.0, 0], [0, 1.0, 1.0]]))
    x = R.sweep(T, np.array([-0.0, np.inf, np.nan]), R.FWD_LAST_ASC)
    assert np.signbit(x[0]) and x[0] == 0 and x[1] == -np.inf and x[2:].view(np.uint64)[0] == 0x7FF8000000000000
    x = R.sweep(T, np.array([np.inf, np.inf, 1.0]), R.FWD_LAST_ASC)                # inf - inf inside a row
    assert x[0] == np.inf and np.isnan(x[1]) and x[1:2].view(np.uint64)[0] == 0x7FF8000000000000
    E = sp.csr_matrix((np.array([2.0, 3.0]), np.array([0, 2]), np.array([0, 1, 1, 2])), shape=(3, 3))
    assert np.isnan(R.sweep(E, np.ones(3), R.FWD_LAST_ASC)[1]) and np.isnan(R.sweep(E, np.ones(3), R.BWD_FIRST_ASC)[1])


def test_order_matters():
    """the three kinds differ where they should: BWD_FIRST_DESC takes the entries behind the diagonal last to first"""
    T = sp.csr_matrix((np.array([1.0, 1e16, 1.0, 1.0, 1.0]), np.array([0, 1, 2, 1, 2]), np.array([0, 3, 4, 5])), shape=(3, 3))
    b = np.array([1e16, 1.0, 1.0])
    assert R.sweep(T, b, R.BWD_FIRST_ASC)[0] == -1.0           # (1e16 - 1e16) - 1
    assert R.sweep(T, b, R.BWD_FIRST_DESC)[0] == 0.0           # (1e16 - 1) rounds to 1e16, - 1e16


@pytest.mark.parametrize("name", ["rows16", "rows16-csc", "rows17-up", "cycle16", "handoff5-up", "chol0-band", "cholt-band", "arrow", "one"])
def test_model_against_the_oracle_bit_for_bit(name):
    O, orc = _orc()
    cls, L, U = _factors(name)
    n = L.shape[0]
    b = G.rhs(n)
    for tr, use in ((False, O.ID), (True, O.TRANSPOSE)):
        want = orc.apply_lu(_fac(L), _fac(U), b, use) if cls == "lu" else orc.apply_llt(_fac(L), b, O.ID)
        got = R.apply(cls, L, U, C.info(name)[2] == "csr", tr, b)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, tr)


# ---- the figures of every case, by hand ----------------------------------------------------------------------------------------------------
# the pattern's own sweep (slot 0; its "-up" / "-csc" twin: the transposed matrix in slot 1 resp. the slot the CSC object keeps it in):
# n, nnz, longest row, shortest row, cuts, B, nb, compact, nslots, rows per lane (the longest block), distinct foreign producer lanes of a
# workgroup, unknowns of other workgroups in a row
FIGURES = {
    "rows16": (48, 648, 16, 1, 33, 1, 48, True, 256, 2, 0, 0),
    "rows17": (48, 649, 17, 1, 33, 1, 48, True, 256, 2, 0, 0),
    "rows1_16": (49, 353, 16, 1, 41, 1, 49, True, 256, 2, 0, 0),
    "dense7": (7, 28, 7, 1, 1, 7, 1, True, 256, 7, 0, 0),
    "dense8": (8, 36, 8, 1, 1, 8, 1, True, 256, 8, 0, 0),
    "nnz15": (8, 15, 8, 1, 7, 1, 8, True, 256, 2, 0, 0),
    "nnz16": (8, 16, 8, 1, 7, 1, 8, True, 256, 2, 0, 0),
    "one": (1, 1, 1, 1, 1, 1, 1, True, 256, 1, 0, 0),
    "tail3": (41, 523, 16, 1, 26, 1, 41, True, 256, 2, 0, 0),
    "tail6": (41, 526, 16, 1, 26, 1, 41, True, 256, 2, 0, 0),
    "chain15": (15, 75, 6, 1, 1, 15, 1, True, 256, 15, 0, 0),
    "chain16": (16, 81, 6, 1, 1, 16, 1, True, 256, 16, 0, 0),
    "chain17": (17, 87, 6, 1, 1, 17, 1, True, 256, 17, 0, 0),
    "chain33": (33, 183, 6, 1, 1, 33, 1, True, 256, 33, 0, 0),
    "chain100": (100, 585, 6, 1, 1, 100, 1, True, 256, 100, 0, 0),
    "cycle16": (514, 4355, 16, 1, 33, 16, 33, True, 256, 16, 0, 0),
    "handoff1": (512, 2738, 6, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff1-desc": (512, 2749, 17, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff3": (512, 2682, 6, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff3-desc": (512, 2693, 17, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff4": (512, 2654, 6, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff4-desc": (512, 2665, 17, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff5": (512, 2626, 6, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff5-desc": (512, 2637, 17, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff8": (512, 2542, 6, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff8-desc": (512, 2553, 17, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff9": (512, 2514, 6, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff9-desc": (512, 2525, 17, 1, 8, 64, 8, True, 256, 64, 0, 0),
    "handoff40": (640, 2698, 6, 1, 4, 160, 4, True, 256, 160, 0, 0),
    "handoff40-desc": (640, 2709, 17, 1, 4, 160, 4, True, 256, 160, 0, 0),
    "imports1": (768, 4804, 7, 1, 768, 1, 768, True, 768, 1, 1, 1),
    "imports63": (768, 5572, 10, 1, 768, 1, 768, True, 768, 1, 63, 4),
    "imports64": (768, 5828, 11, 1, 768, 1, 768, True, 768, 1, 64, 5),
    "imports65": (768, 6852, 15, 1, 768, 1, 768, True, 768, 1, 65, 9),
    "imports512": (768, 6852, 15, 1, 768, 1, 768, True, 768, 1, 512, 9),
    "imports65-desc": (768, 6854, 17, 1, 768, 1, 768, True, 768, 1, 67, 11),
    "lanes511": (511, 3046, 6, 1, 511, 1, 511, True, 512, 1, 6, 5),
    "lanes512": (512, 3052, 6, 1, 512, 1, 512, True, 512, 1, 6, 5),
    "lanes513": (513, 3058, 6, 1, 513, 1, 513, True, 768, 1, 6, 5),
    "lines4x192": (768, 4376, 6, 1, 192, 1, 768, True, 768, 2, 12, 4),
    "chol0-band": (300, 2070, 7, 1, 10, 30, 10, True, 256, 30, 0, 0),
    "cholt-band": (300, 2070, 7, 1, 10, 30, 10, True, 256, 30, 0, 0),
    "lines4x192-short": (768, 2108, 3, 1, 192, 1, 768, True, 768, 2, 3, 1),
    "ghost20": (6000, 12580, 3, 1, 300, 20, 300, True, 512, 20, 44, 1),
    "chain32768": (32768, 65535, 2, 1, 1, 32768, 1, True, 256, 32768, 0, 0),
    "chain32769": (32769, 65537, 2, 1, 1, 32769, 1, False, 256, 32769, 0, 0),
    "arrow": (2048, 3063, 1000, 1, 2048, 1, 2048, True, 2048, 1, 875, 875),
    "cholt-indefinite": (300, 1045, 7, 0, 155, 1, 300, True, 512, 2, 6, 6),
}
KEYS = ("n", "nnz", "longest", "shortest", "ncuts", "B", "nb", "compact", "nslots", "rows_per_lane", "foreign_producers", "externals_per_row")


def _figures_of(T, fwd):
    f = R.figures(T, fwd)
    return (T.shape[0], T.nnz, f["longest"], f["shortest"], f["sch"]["ncuts"], f["sch"]["B"], f["sch"]["nb"], f["compact"], f["nslots"],
            f["rows_per_lane"], f["foreign_producers"], f["externals_per_row"])


@pytest.mark.parametrize("name", C.NAMES + (C.DEGENERATE,))
def test_figures(name):
    cls, L, U = _factors(name)
    S = R.stored(cls, L, U)
    base = name[:-3] if name.endswith("-up") else name[:-4] if name.endswith("-csc") else name
    # ("-up": U is the transposed pattern and its transposed copy, slot 2, the pattern itself; the CSC object made of the lower matrix holds
    # the factors of the row-major view, the same two)
    slot = 2 if name != base else 0
    got = _figures_of(S[slot], FWD[cls][slot])
    assert got == FIGURES[base], (name, dict(zip(KEYS, got)), dict(zip(KEYS, FIGURES[base])))
    if cls == "lu":                          # ... and the other factor is the diagonal alone: one row per lane, nothing read
        diag = 0 if name != base else 1
        other = _figures_of(S[diag], FWD[cls][diag])
        if name != base:                     # ... and the backward sweep of "-up" walks what the lower case's transposed apply walks
            lo = C.factors(_orc()[1], base)
            assert _figures_of(S[1], False) == _figures_of(R.stored(*lo)[3], False), name
        n = got[0]
        assert other[:7] == (n, n, 1, 1, n, 1, n) and other[9:] == (1, 0, 0), (name, other)
    if name != C.DEGENERATE:
        assert level_ref.levels(S[slot])[2] >= 1          # (triangular: no cycle)


def test_patterns_survive_the_factorisation():
    """ILUT(fill_in = n, threshold = 0) and ILU(0) of a triangular matrix, IChol(0) and ICholT of P + P^T: the factor has the pattern's entries"""
    for name in C.NAMES:
        cls, L, U = _factors(name)
        P = C.pattern(name)
        S = R.stored(cls, L, U)
        if cls == "lu":                     # (lower, CSR input: L; "-up" and CSC input: the transposed copy of U -- test_figures)
            T = S[0] if C.info(name)[1:3] == ("lower", "csr") else S[2]
        else:
            T = S[0] if cls == "ichol0" else S[3]
        T = T.tocsr(); T.sort_indices()
        assert np.array_equal(T.indptr, P.indptr) and np.array_equal(T.indices, P.indices), name


def test_rows_at_the_array_ends():
    """the window loads are clamped at both ends of the entry arrays: the length of the first and of the last stored row of the swept triangle,
    and the entries between the last row's start and nnz (3 and 6: fewer than 4 and fewer than 8)"""
    want = {"rows16": (1, 16), "rows1_16": (1, 1), "tail3": (1, 3), "tail6": (1, 6), "cycle16": (1, 2)}
    for name, (first, last) in want.items():
        cls, L, U = _factors(name)
        T = R.stored(cls, L, U)[0]
        rows = np.diff(T.indptr)
        assert (rows[0], rows[-1]) == (first, last) and T.nnz - T.indptr[-2] == last, (name, rows[0], rows[-1])
        cls, L, U = _factors(name + "-up")               # (the transposed matrix keeps the pattern in slot 2, swept forward as well ...)
        assert np.array_equal(np.diff(R.stored(cls, L, U)[2].indptr), rows), name
    # (... and its own U, slot 1, begins with a long row: column 0 of the pattern, which every row reads -- n entries)
    for name, first in (("rows16-up", 48), ("tail3-up", 41)):
        cls, L, U = _factors(name)
        rows = np.diff(R.stored(cls, L, U)[1].indptr)
        assert (rows[0], rows[-1]) == (first, 1), (name, rows[0], rows[-1])


@pytest.mark.parametrize("d", [1, 3, 4, 5, 8, 9, 40])
def test_handoff_distances(d):
    """a lane of handoff<d> reads its neighbour d .. d + 3 rows back and its own previous row; the "-desc" twin has these and one long row"""
    for name, exact in (("handoff%d" % d, True), ("handoff%d-desc" % d, False), ("handoff%d-up" % d, True)):
        cls, L, U = _factors(name)
        slot = 1 if name.endswith("-up") else 0
        f = R.figures(R.stored(cls, L, U)[slot], FWD[cls][slot])
        assert f["own_previous_row"] and f["workgroups"] == 1 and f["foreign_producers"] == 0
        assert set(range(d, d + 4)) <= set(f["lane_distances"]), (name, f["lane_distances"])
        assert not exact or f["lane_distances"] == list(range(d, d + 4)), (name, f["lane_distances"])


def test_schedule_rules():
    """make_schedule, k_block_starts and schedule_is_compact on patterns small enough to do by hand"""
    chain = C.chain(10)
    for T, fwd in ((chain, True), (chain.T.tocsr(), False)):
        s = R.schedule(T, fwd)
        assert (s["ncuts"], s["B"], s["nb"], s["start"].tolist()) == (1, 10, 1, [0, 10])
    s = R.schedule(C.band(20, 1, 5), True)                       # chains of 5: B = 5
    assert (s["ncuts"], s["B"], s["nb"], s["start"].tolist()) == (4, 5, 4, [0, 5, 10, 15, 20])
    s = R.schedule(C.band(20, 1, 4), True)                       # chains of 4 are "no chains to speak of": B = 1, and a cell inside a chain is empty
    assert (s["ncuts"], s["B"], s["nb"]) == (5, 1, 20) and s["start"][:6].tolist() == [0, 2, 3, 4, 4, 6]
    s = R.schedule(C.band(21, 1, 7), True)                       # 21 rows, 3 cuts: B = 7
    assert (s["B"], s["nb"]) == (7, 3)
    assert R.is_compact({"B": 32768}, (1 << 17) - 64) and not R.is_compact({"B": 32769}, 256) and not R.is_compact({"B": 1}, (1 << 17) - 63)
    assert R.lc_rule(16, 16, 8) and not R.lc_rule(17, 16, 8) and not R.lc_rule(16, 15, 8) and not R.lc_rule(16, 16, 7) and not R.lc_rule(0, 16, 8)
    assert R.lm_necessary(32, 8, 256) and not R.lm_necessary(33, 8, 256) and not R.lm_necessary(15, 8, 256)
    assert R.long_rows(4097, 1024) and not R.long_rows(4096, 1024) and not R.long_rows(4 * 1023 + 1, 1023)


def test_tiling():
    """lines4x192: 768 blocks of one row with block offsets 1 and 4 (8, 12, 16): patches of 4 x 64; fewer than 512 blocks, or no dominant
    offset beside 1, and the placement is the identity"""
    cls, L, U = _factors("lines4x192")
    T = R.stored(cls, L, U)[0]
    sch = R.schedule(T, True)
    assert R.tiling(T, sch) == (4, 4, 64) and R.tiling(T, sch, tile_tz=2) == (4, 4, 2) and R.tiling(T, sch, no_tiles=True) is None
    assert R.slots(sch, (4, 4, 64))[0] == 768 and R.slots(sch, (4, 4, 2))[0] == 96 * 256
    for name in ("lanes511", "lanes512", "lanes513", "imports65"):
        cls, L, U = _factors(name)
        T = R.stored(cls, L, U)[0]
        assert R.tiling(T, R.schedule(T, True)) is None, name


# ---- the routes ----------------------------------------------------------------------------------------------------------------------------
def test_joint_rule():
    """chain32769: L's B = 32 769 does not fit the descriptors' position field, and U (the diagonal: B = 1, compact by itself) follows it"""
    cls, L, U = _factors("chain32769")
    S = R.stored(cls, L, U)
    assert not R.figures(S[0], True)["compact"] and R.figures(S[1], False)["compact"] and R.figures(S[1], False)["sch"]["B"] == 1
    assert R.expected_routes(cls, L, U) == {s: (R.ROUTE_GENERIC, 0) for s in range(4)}
    cls, L, U = _factors("chain32768")
    assert all(r[1] == (R.ROUTE_DESCRIPTORS, R.KERNEL_LC) for r in R.expected_routes(cls, L, U).values())


def test_records_are_exactly_the_undecided_slots():
    """a slot is RECORDED iff the model answers "level-major or CSR kernel": nnz > 4 n, nnz < 16 or no descriptors are predicted outright;
    under ILUPP_NO_PACKED=1 everything is"""
    for name in C.NAMES:
        cls, L, U = _factors(name)
        S = R.stored(cls, L, U)
        e = R.expected_routes(cls, L, U)
        undecided = {s for s, r in e.items() if r[0] == R.LM_OR_CSR}
        assert undecided == set(C.RECORDED.get(name, {})), name
        for s in undecided:
            assert S[s].nnz <= 4 * S[s].shape[0] and S[s].nnz >= 16, (name, s)
            assert C.RECORDED[name][s] in (R.ROUTE_LEVEL_MAJOR, R.ROUTE_DESCRIPTORS), (name, s)
        assert not any(isinstance(r[0], str) for r in R.expected_routes(cls, L, U, no_packed=True).values()), name


def test_every_kernel_and_kind_has_a_case():
    """by the model and the records: (route, kernel, kind) over all cases, ILUPP_NO_PACKED=1 and the degenerate case included"""
    seen = set()
    for name in C.NAMES + (C.DEGENERATE,):
        cls, L, U = _factors(name)
        for no_packed in (False, True):
            e = R.expected_routes(cls, L, U, degenerate=name == C.DEGENERATE, no_packed=no_packed)
            for s, (route, kernel) in e.items():
                if route == R.LM_OR_CSR:
                    route, kernel = (R.ROUTE_LEVEL_MAJOR, 0) if C.RECORDED[name][s] == R.ROUTE_LEVEL_MAJOR else kernel
                seen.add((route, kernel, KIND[cls][s]))
    for kind in range(3):
        assert (R.ROUTE_DESCRIPTORS, R.KERNEL_LC, kind) in seen and (R.ROUTE_DESCRIPTORS, R.KERNEL_DESC, kind) in seen, kind
        assert (R.ROUTE_GENERIC, 0, kind) in seen and (R.ROUTE_LEVEL_MAJOR, 0, kind) in seen, kind
    assert (R.ROUTE_ROWS_DEGENERATE, 0, R.FWD_LAST_ASC) in seen and (R.ROUTE_ROWS_DEGENERATE, 0, R.BWD_FIRST_ASC) in seen
    # the rule between the two descriptor kernels, case by case
    want = {"rows16": 1, "rows17": 2, "rows1_16": 1, "dense7": 2, "dense8": 1, "nnz15": 2, "nnz16": 1, "one": 2}
    for name, kernel in want.items():
        cls, L, U = _factors(name)
        r = R.expected_routes(cls, L, U, no_packed=True)[0]
        assert r == (R.ROUTE_DESCRIPTORS, kernel), (name, r)
