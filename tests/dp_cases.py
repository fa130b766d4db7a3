"""The cases of tests/test_gpu_dp_chains.py, by name: each is a designed matrix, without preprocessing, that puts ONE step of the chain with
pivoting (ilupp_amd/csrc/pilucdp.hip: k_pilucdp_lds, k_pilucdp) on one side of one boundary: the 2 048th or 2 049th entry of a working
vector at one of the eight places where the LDS kernel abandons a step, a count of 1 024 in the bucket bookkeeping, the 64th or 65th kept
entry, a chunk of bucket moves that clash, a group of 64 or 65 rows, an index stored twice across a 64-entry pass, the ends of the
PERMUTE_ROWS window.  tests/test_dp_ref.py asserts on the CPU, from the records of the model (tests/dp_ref.py), that every case sits where
its name says (CASES[name].pin), that the model and the oracle (and the reference, where it is built) agree on it bit for bit, and that the
cases discriminate the mistakes a hand-over, a resume, a chunk of moves or a doubled index invite.

A case is Case(build, threshold, knobs, pin): build() -> (indptr, indices, data) by rows, knobs by the reference's names on top of
BASE, pin(levels) -> bool on the model's levels.  arrays(name, fmt) gives the same matrix as CSR or CSC.

BASE: MAX_LEVELS 1 (one level, never ended: force_finish), PERMUTE_ROWS 0 (the rows in their order), piv_tol 1, and the one dropping rule
that is a constant weight (USE_STANDARD_DROPPING2, weight 1): an entry stays if |x| >= threshold after scaling.  Diagonals are 4, other
entries mag(j) in [1, 1.1): the diagonal is the pivot, direct entries come out at 0.25 .. 0.275 and stay at threshold 0.2, products of two
of them (fill) go.  Every dense row sits over columns that hold nothing but their diagonal, every dense column beside rows that hold
nothing but theirs, so a case has one large step (two where a level is ended: the next level meets the same row again).

Patterns:
  row(s, m)         row s holds m entries from its diagonal on: row load of m (point row_load)
  two_urows(m)      rows 0 and 1 hold m - 1 columns between them, row 2 has entries in columns 0 and 1: its working row grows to m by
                    subtracting the two rows of U (l_sub) while all those columns are still alive
  nodiag(m)         row 0 holds m entries and no diagonal, the largest in column 1; row 1 holds column 0 alone: the diagonal is inserted as
                    entry m + 1 (diag_touch), the pivot is column 1
  zeros(m)          row 0 is column 1 alone (pivot column 1, so column 1 is dead when row 1 comes), row 1 holds m stored zeros: no entry is
                    larger than zero, perm[1] = column 0 is inserted as entry m + 1 (perm_touch); the pivot is 0, the row NaN and dropped
  col(s, m)         column s holds m entries below its diagonal (col_load_own)
  two_lcols(m)      the transpose of two_urows (u_sub_own)
  offcol(m)         row 0 = {0: 1, 1: 8}: the pivot of step 0 is column 1, which holds m other rows (col_load_other)
  off_two_lcols(m)  two_lcols where the row of the large step has its pivot off the diagonal (u_sub_other)
  schur_*           the same row patterns behind a row with a pivot of 2^-10: MAX_LEVELS 2, SMALL_PIVOT_TERMINATES: the large step runs
                    with eliminate == false
  arrow(n)          row 5 holds every column, PERMUTE_ROWS 3: its count of entries in L walks 1 .. n - 1, one bucket move per step
  arrow2(n)         rows 5 and 7 hold every column: two moves per step into the same bucket
  lcol(rows)        column 0 holds the given rows, PERMUTE_ROWS 3: one step with len(rows) bucket moves, and the group they form

NOT pinned, with the reason:
  * probing that wraps at slot 4 095 of the 4 096-slot table at the sizes this file otherwise keeps to (n <= 2 200): unreachable.  lv_hash
    is injective on 0 .. 2 585 (the first two indices that share a slot are 2 and 2 586), so below that every probe is one slot long; the
    first index set that fills slots 4 091 .. 4 095 and sends one more index there needs index 4 558.  probe_wrap is that case, at
    n = 4 559: the one case larger than 2 200.
  * which lane's index gets which slot when several lanes enter the table in one pass (atomicCAS): the order is the hardware's; the model
    enters them in entry order.  Slot numbers are not results; only the set of occupied slots matters, and that is the same.
  * a hand-over at perm_touch that is not a zero pivot: cannot happen.  The touch is reached only if no entry of the row is larger than
    zero, so the pivot it inserts is 0.
  * more than 2 048 entries in the Schur phase at any point but row_load and l_sub: the other six points belong to an eliminating step.
  * a status-3 stop (the Schur store) between a hand-over and the level's end is pinned by the predicted launch sequence of the schur_*
    cases under small stores; a status-3 stop that a hand-over FOLLOWS in the same level is not: the Schur phase is entered once, and the
    schur_* cases hand over in its first large row.
  * FINAL_ROW_CRIT other than by small pivot as what ends the level: the criteria read numb[k] or the row's norm once per step, none of
    the boundaries above; tests/test_gpu_mlp.py runs every family.
  * inverse-based and weighted dropping: the model refuses them (dp_ref.refuses); the memory flavour runs them in the breadth tests of
    tests/test_gpu_dp_chains.py against the oracle."""
import collections
import functools

import numpy as np

import dp_ref as R
from pivot_cases import mag, slices

Case = collections.namedtuple("Case", "build threshold knobs pin")
BASE = dict(piv_tol=1.0, PERMUTE_ROWS=0, TOTAL_PIV=1, BEGIN_TOTAL_PIV=True, SMALL_PIVOT_TERMINATES=False, MIN_ELIM_FACTOR=1.0, MAX_LEVELS=1,
            USE_STANDARD_DROPPING2=True, USE_ERR_PROP_DROPPING=False, WEIGHT_STANDARD_DROP2=1.0)
SCHUR = dict(MAX_LEVELS=2, SMALL_PIVOT_TERMINATES=True, MIN_PIVOT=0.01, MIN_ELIM_FACTOR=0.0, THRESHOLD_SHIFT_SCHUR=0.01)
D, TAU = 4.0, 0.2
CAP = R.LV_CAP


def knobs(**kw):
    d = dict(BASE)
    d.update(kw)
    return d


# ---- patterns ------------------------------------------------------------------------------------------------------------------------------
def row(n, s, m, last_largest=False):
    r = [(s, D)] + [(s + j, mag(j)) for j in range(1, m)]
    if last_largest:
        r[-1] = (s + m - 1, 8.0)
        return lambda: slices(n, {s: r, s + m - 1: [(s, D)]}, D)            # (the pivot column's own row takes column s instead)
    return lambda: slices(n, {s: r}, D)


def two_urows(n, m, schur=False):
    """working row of row s (2; 3 behind the small pivot): its diagonal + na + nb columns = m, all of them still to come"""
    s_ = 3 if schur else 2
    o = s_ + 1
    na = (m - 1) // 2
    nb = m - 1 - na
    sp = {0: [(0, D)] + [(o + j, mag(j)) for j in range(na)], 1: [(1, D)] + [(o + na + j, mag(j + 1)) for j in range(nb)], s_: [(0, 1.0), (1, 1.0), (s_, D)]}
    if schur:
        sp[2] = [(2, 2.0 ** -10)]
    assert o + na + nb <= n
    return lambda: slices(n, sp, D)


def nodiag(n, m):
    return lambda: slices(n, {0: [(1, 3.0)] + [(1 + j, mag(j)) for j in range(1, m)], 1: [(0, D)]}, D)


def zeros(n, m):
    return lambda: slices(n, {0: [(1, D)], 1: [(2 + j, 0.0) for j in range(m)]}, D)


def col(n, s, m):
    sp = {s + j: [(s, mag(j)), (s + j, D)] for j in range(1, m + 1)}
    return lambda: slices(n, sp, D)


def two_lcols(n, m, off=False):
    """working column of step 2: na + nb rows = m, all of them still to come.  off: that step's pivot is column 3, not the row's own"""
    na = m // 2
    nb = m - na
    c, o = (3, 4) if off else (2, 3)
    sp = {0: [(0, D), (c, 1.0)], 1: [(1, D), (c, 1.0)]}
    for j in range(na):
        sp[o + j] = [(0, mag(j)), (o + j, D)]
    for j in range(nb):
        sp[o + na + j] = [(1, mag(j + 1)), (o + na + j, D)]
    assert o + na + nb <= n
    if off:
        sp[2] = [(2, 1.0), (3, 8.0)]
        sp[3] = [(2, D)]
    return lambda: slices(n, sp, D)


def offcol(n, m):
    sp = {0: [(0, 1.0), (1, 8.0)], 1: [(0, D)]}
    for j in range(m):
        sp[2 + j] = [(1, 2.0 * mag(j)), (2 + j, D)]
    return lambda: slices(n, sp, D)


def schur_row(n, s, m):
    r = [(s, D)] + [(s + j, mag(j)) for j in range(1, m)]
    return lambda: slices(n, {2: [(2, 2.0 ** -10)], s: r}, D)


def arrow(n, r0=5):
    return lambda: slices(n, {r0: [(c, D if c == r0 else mag(c)) for c in range(n)]}, D)


def arrow2(n, r0=5, r1=7):
    """two rows that hold every column: two bucket moves per step into one bucket (the second lane's rank is 1, the cached boundary is
    lowered twice), their counts walking up to n - 1"""
    sp = {r: [(c, D if c == r else mag(c + r)) for c in range(n)] for r in (r0, r1)}
    return lambda: slices(n, sp, D)


def lcol(n, rows_):
    sp = {r: [(0, mag(r)), (r, D)] for r in rows_}
    return lambda: slices(n, sp, D)


def marks(n):
    """row 0 = {0, 1, 3, 5} and row 1 = {0, 1} are eliminated in the LDS flavour: column 1 and row 1 die there.  Row 2 holds 2 049 entries
    (the hand-over).  Row 3 = {0, 3} subtracts row 0 of U -- column 1 is dead, column 5 is new though row 2 held it --, and column 3
    subtracts column 0 of L, where row 1 is dead"""
    sp = {0: [(0, D), (1, 2.0), (3, 3.0), (5, 1.0)], 1: [(0, 2.0), (1, D)], 2: [(2, D)] + [(2 + j, mag(j)) for j in range(1, CAP + 1)], 3: [(0, 3.0), (3, D)]}
    return lambda: slices(n, sp, D)


def kept_row(n, m, big):
    """row 0: m entries behind the diagonal, the first `big` of them 2 (0.5 after scaling), the others 1 (0.25): threshold 0.3 keeps `big`"""
    return lambda: slices(n, {0: [(0, D)] + [(1 + j, (2.0 if j < big else 1.0) * (1.0 if j % 2 else -1.0)) for j in range(m)]}, D)


def kept_col(n, m, big):
    sp = {1 + j: [(0, (2.0 if j < big else 1.0) * (1.0 if j % 2 else -1.0)), (1 + j, D)] for j in range(m)}
    return lambda: slices(n, sp, D)


def twice_row(n, m):
    """row 0: entries 63 and 64 are both column 64 (entry 0 is the diagonal), values 1.5 and then 1.25: the last one stands"""
    r = [(0, D)] + [(j, mag(j)) for j in range(1, 63)] + [(64, 1.5), (64, 1.25)] + [(j, mag(j)) for j in range(65, m)]
    return lambda: slices(n, {0: r}, D)


def twice_col(n, m):
    """column 0: entry 0 is the diagonal, rows 1 .. 62 are its entries 1 .. 62, row 70 holds column 0 twice: entries 63 and 64, values 1.5
    and then 1.25"""
    sp = {r: [(0, mag(r)), (r, D)] for r in range(1, 63)}
    sp[70] = [(0, 1.5), (0, 1.25), (70, D)]
    for r in range(71, m):
        sp[r] = [(0, mag(r)), (r, D)]
    return lambda: slices(n, sp, D)


def probe_wrap(n=4559):
    """row 0: the five indices that fill slots 4 091 .. 4 095, then 4 558 (slot 4 091 again: its probe wraps), then the diagonal and
    columns up to 2 048 entries"""
    first = [377, 1974, 3571, 987, 2584, 4558]
    assert [R.lv_hash(c) for c in first] == [4091, 4092, 4093, 4094, 4095, 4091]
    rest = [c for c in range(0, CAP) if c not in first][:CAP - len(first)]
    r = sorted([(c, D if c == 0 else mag(c)) for c in first + rest])
    return lambda: slices(n, {0: r}, D)


# ---- what a pin reads ----------------------------------------------------------------------------------------------------------------------
def stops(levels):
    return [(q, r["step"], r["stop"], r["eliminate"]) for q, lev in enumerate(levels) for r in lev.records if r["stop"]]


def at_point(levels, point, q=0):
    """the largest count a vector reaches at the point, over the steps of level q (z for the first four points, w for the others)"""
    side = 1 if R.POINTS.index(point) < 4 else 2
    return max([c[side] for r in levels[q].records for c in r["checks"] if c[0] == point], default=0)


def largest(levels):
    return max(max(r["znnz"], r["wnnz"]) for lev in levels for r in lev.records)


def fits(point):
    return lambda lv: at_point(lv, point) == CAP and not stops(lv) and largest(lv) == CAP


def hands_over(point, step, eliminate=True):
    return lambda lv: at_point(lv, point) == CAP + 1 and [s for s in stops(lv) if s[0] == 0] == [(0, step, point, eliminate)]


def rec0(lv, k=0):
    return lv[0].records[k]


CASES = collections.OrderedDict()
N = 2060
STORE = 50                    # the ILUPP_DP_STORE of the small-store modes: stores of n + 52 entries that grow by as much
# the eight places where a step is abandoned: 2 048 entries fit, the 2 049th hands over
CASES["row_load/2048_step0"] = Case(row(N, 0, CAP), TAU, knobs(), lambda lv: fits("row_load")(lv) and rec0(lv)["takeU"] == (CAP - 1, N - 1, CAP - 1))
CASES["row_load/2049_step0"] = Case(row(N, 0, CAP + 1), TAU, knobs(), hands_over("row_load", 0))
CASES["row_load/2048_mid"] = Case(row(2160, 100, CAP), TAU, knobs(), fits("row_load"))
CASES["row_load/2049_mid"] = Case(row(2160, 100, CAP + 1), TAU, knobs(), hands_over("row_load", 100))
CASES["l_sub/2048"] = Case(two_urows(N, CAP), TAU, knobs(), fits("l_sub"))
CASES["l_sub/2049"] = Case(two_urows(N, CAP + 1), TAU, knobs(), hands_over("l_sub", 2))
CASES["diag_touch/2048"] = Case(nodiag(N, CAP - 1), TAU, knobs(), lambda lv: fits("diag_touch")(lv) and rec0(lv)["pivot_col"] == 1)
CASES["diag_touch/2049_missing_diagonal"] = Case(nodiag(N, CAP), TAU, knobs(), lambda lv: hands_over("diag_touch", 0)(lv) and rec0(lv)["checks"][0][1] == CAP)
CASES["perm_touch/2048"] = Case(zeros(N, CAP - 1), TAU, knobs(), lambda lv: fits("perm_touch")(lv) and lv[0].zero_pivots == 1)
CASES["perm_touch/2049"] = Case(zeros(N, CAP), TAU, knobs(), lambda lv: hands_over("perm_touch", 1)(lv) and lv[0].zero_pivots == 1)
CASES["col_load_own/2048"] = Case(col(2160, 100, CAP), TAU, knobs(), lambda lv: fits("col_load_own")(lv) and rec0(lv, 100)["takeL"] == (CAP, 2160, CAP))
CASES["col_load_own/2049"] = Case(col(2160, 100, CAP + 1), TAU, knobs(), hands_over("col_load_own", 100))
CASES["u_sub_own/2048"] = Case(two_lcols(N, CAP), TAU, knobs(), fits("u_sub_own"))
CASES["u_sub_own/2049"] = Case(two_lcols(N, CAP + 1), TAU, knobs(), hands_over("u_sub_own", 2))
CASES["col_load_other/2048"] = Case(offcol(N, CAP), TAU, knobs(), fits("col_load_other"))
CASES["col_load_other/2049"] = Case(offcol(N, CAP + 1), TAU, knobs(), hands_over("col_load_other", 0))
CASES["u_sub_other/2048"] = Case(two_lcols(N, CAP, off=True), TAU, knobs(), fits("u_sub_other"))
CASES["u_sub_other/2049"] = Case(two_lcols(N, CAP + 1, off=True), TAU, knobs(), hands_over("u_sub_other", 2))
# ... with eliminate == false: the level ends at row 2 (a pivot of 2^-10), the large row is a row of the Schur complement
CASES["schur/row_load_2048"] = Case(schur_row(N, 5, CAP), TAU, knobs(**SCHUR), lambda lv: at_point(lv, "row_load") == CAP and not stops(lv) and not rec0(lv, 5)["eliminate"])
CASES["schur/row_load_2049"] = Case(schur_row(N, 5, CAP + 1), TAU, knobs(**SCHUR), hands_over("row_load", 5, eliminate=False))
CASES["schur/l_sub_2049"] = Case(two_urows(N, CAP + 1, schur=True), TAU, knobs(**SCHUR), hands_over("l_sub", 3, eliminate=False))
# the pivot search: the largest entry in the last of 2 048 slots, piv_tol 1
CASES["pivot/last_slot_2048"] = Case(row(N, 0, CAP, last_largest=True), TAU, knobs(), lambda lv: fits("row_load")(lv) and rec0(lv)["pivot_col"] == CAP - 1)
CASES["probe_wrap"] = Case(probe_wrap(), TAU, knobs(), lambda lv: fits("row_load")(lv) and rec0(lv)["zprobe"][1] and rec0(lv)["zprobe"][0] >= 6)
# the selection: kept 64 / 65 of 200 (dp_sort_n against wave_sort_u64), and a bounded fill against 300 candidates
for big in (64, 65):
    CASES["kept/U_%d" % big] = Case(kept_row(220, 200, big), 0.3, knobs(), lambda lv, b=big: rec0(lv)["takeU"] == (b, 219, b))
    CASES["kept/L_%d" % big] = Case(kept_col(220, 200, big), 0.3, knobs(), lambda lv, b=big: rec0(lv)["takeL"] == (b, 220, b))
for f in (1, 64, 65):
    CASES["fill/U_%d" % f] = Case(row(320, 0, 301), TAU, knobs(fill_in=f), lambda lv, f=f: rec0(lv)["takeU"] == (300, f - 1, f - 1))
    CASES["fill/L_%d" % f] = Case(col(320, 0, 300), TAU, knobs(fill_in=f), lambda lv, f=f: rec0(lv)["takeL"] == (300, f, f))
# the bucket bookkeeping: a count that walks up to n - 1 around kPnL = 1 024 (npn = min(n + 2, 1024))
for n_ in (1021, 1022, 1023, 1024, 1025, 1026, 1027, 1100):
    CASES["arrow/%d" % n_] = Case(arrow(n_), TAU, knobs(PERMUTE_ROWS=3),
                                   lambda lv, n_=n_: max(r["pnum_seen"] for r in lv[0].records if r["takeL"]) == n_ - 1
                                   and sum(1 for r in lv[0].records if r["far"]) == max(0, n_ - 1 - (R.PNL - 1)) and all(len(r["moves"]) <= 1 for r in lv[0].records))
CASES["arrow2/1030"] = Case(arrow2(1030), TAU, knobs(PERMUTE_ROWS=3),
                            lambda lv: max(r["pnum_seen"] for r in lv[0].records if r["takeL"]) == 1029 and sum(1 for r in lv[0].records if r["far"]) == 1029 - (R.PNL - 1)
                            and sum(1 for r in lv[0].records if r["moves"] == ["once"] and r["takeL"][2] == 2) >= 1000)
CASES["moves/once_2chunks"] = Case(lcol(200, range(1, 101)), TAU, knobs(PERMUTE_ROWS=3), lambda lv: rec0(lv)["moves"] == ["once", "once"])
CASES["moves/clash"] = Case(lcol(200, range(130, 200)), TAU, knobs(PERMUTE_ROWS=3), lambda lv: rec0(lv)["moves"] == ["clash", "once"])
CASES["group/64"] = Case(lcol(200, range(1, 65)), TAU, knobs(PERMUTE_ROWS=3), lambda lv: [r["group"] for r in lv[0].records if r["group"] > 1] == [64])
CASES["group/65"] = Case(lcol(200, range(1, 66)), TAU, knobs(PERMUTE_ROWS=3), lambda lv: [r["group"] for r in lv[0].records if r["group"] > 1] == [65])
# an index stored twice, the copies on both sides of a 64-entry pass
CASES["twice/row_63_64"] = Case(twice_row(120, 100), TAU, knobs(), lambda lv: rec0(lv)["dupz"] == [1] and rec0(lv)["znnz"] == 99)
CASES["twice/col_63_64"] = Case(twice_col(120, 100), TAU, knobs(), lambda lv: rec0(lv)["dupw"] == [1] and rec0(lv)["wnnz"] == 92)
# the window of the row reordering: PERMUTE_ROWS 2 in a level of the loop is [0, (n - 1) / 2]; PERMUTE_ROWS 1 without preprocessing [n - 1, n - 1]
CASES["window/rows2_epr"] = Case(lcol(101, (5, 50, 51)), TAU, knobs(PERMUTE_ROWS=2, MAX_LEVELS=2),
                                 lambda lv: list(lv[0].perm_rows[[5, 49, 50, 51]]) == [49, 5, 50, 51] and len(lv) == 1 and rec0(lv)["moves"] == ["clash"])
CASES["window/rows1_bpr"] = Case(lcol(101, (99, 100)), TAU, knobs(PERMUTE_ROWS=1), lambda lv: list(lv[0].perm_rows) == list(range(101)))
# what crosses a hand-over and a resume: columns and rows that died in the LDS flavour, met again by the subtractions of the memory flavour;
# a step of the memory flavour that begins a launch (the stores are full behind the large row) and meets indices of the step before it
CASES["handover/marks"] = Case(marks(N), TAU, knobs(), lambda lv: stops(lv) == [(0, 2, "row_load", True)]
                               and R.launches(lv, store=STORE)[:2] == [(N, "LDS", 4, 2), (N, "memory", 1, 3)])
NAMES = list(CASES)
# the cases every mode of the GPU test runs with small stores, and the one whose launch sequence must show a store stop in the LDS flavour,
# the hand-over, and a store stop in the memory flavour
STOP_HANDOVER_STOP = "row_load/2049_mid"


def params(name, O):
    import ml_cases
    c = CASES[name]
    return ml_cases.oracle_params(O, c.threshold, (), c.knobs)


@functools.lru_cache(maxsize=None)
def rows(name):
    return CASES[name].build()


@functools.lru_cache(maxsize=None)
def arrays(name, fmt):
    """(indptr, indices, data) of the case as "csr" or "csc": the same matrix"""
    ptr, idx, val = rows(name)
    if fmt == "csr":
        return ptr, idx, val
    p, i, v = R.other_orientation([int(x) for x in ptr], [int(x) for x in idx], [float(x) for x in val])
    return np.array(p, dtype=np.int32), np.array(i, dtype=np.int32), np.array(v, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def model(name):
    from oracle import oracle as O
    ptr, idx, val = rows(name)
    return R.multilevel(ptr, idx, val, True, params(name, O))
