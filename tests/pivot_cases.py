"""The cases of tests/test_gpu_pivot_chains.py, by name: each is a designed pattern that puts ONE row of the ILUTP chain (ilutp.hip: tp_chain,
tp_select) or ONE step of the ILUCP chain (ilucp.hip: cp_chain, with dp_subtract, dp_seq_sum, dp_sort_n of dp_dev.h and select_largest,
wave_sort_u64 of piluc_dev.h) on one side of one boundary: a 64-entry pass edge of one of the loops, a tie rule, a selection branch, a
store's last entry.  tests/test_pivot_ref.py asserts on the CPU, from the records of the model (tests/pivot_ref.py), that every case sits
where its name says (CASES[name].pin), that the model and the oracle and the reference agree on it bit for bit, and -- for the ordered
sums and the duplicates -- that the case is discriminating: another order of the same terms, or the copies swapped, gives other bits.

A case is Case(kind, build, params, pin): kind "tp" (ILUTP: the arrays are rows) or "cp" (ILUCP: the arrays are the reference's columns),
build() -> (indptr, indices, data), params the five constructor arguments, pin(result, figures, records) -> bool.

Patterns (all values exactly representable unless the case is about rounding):
  tp_left(m)        rows 0 .. m-1 their diagonal alone, row m has m entries left of its diagonal: a stored row of m + 1, m left norm terms,
                    m eliminations with U rows of length 1, an L row of m + 1
  tp_min(ns)        the last row loads ns slots; eliminating column 0 appends column 1 BEHIND them: the next smallest waiting position sits
                    in slot ns, a later pass than lane 0's first slot
  tp_urow(len)      row 0 has len entries behind its pivot, row 1 = {0, 1}: one subtraction of len entries, all new (or every second: mixed)
  tp_top(w, slots)  row 0 has w entries, the largest magnitude at the given slots (different signs): the first of equal maxima
  bidiag(n)         rows {r: 1, r + 1: 3}: the diagonal is kept or the 3 is the pivot, by piv_tol and the switch row
  cp_top(w)         row 0 of the matrix has w entries (the slices' first entries): nrow = w, a U row of w, subtracted from the rows slice 0 names
  cp_leftcol(m)     slice 0 has m entries: the pivot column of step 0, an L column of m
Empty rows and slices, rows without a diagonal, stored zeros, columns stored twice are written out where they are used.

NOT pinned, with the reason:
  * `encountered zero pivot in row n - 1`: unreachable.  The error needs the pivot 0.0 to be SELECTED; a candidate must be > norm * tau, so
    a stored 0.0 gets there only as the kept diagonal (magnitude := norm of the U part), which needs larg * piv_tol < 0, i.e. another
    nonzero entry in the U part -- and the U part of the last row is one position wide.  zperr_last raises it in row n - 2, the last
    row that can.
  * status 12 of k_ilutp ("the working row outgrows its slots"): unreachable for rows with sorted indices once a column stored twice
    takes one slot.  A subtracted U row k only holds columns of positions > k (later swaps exchange positions > k), so a dropped
    column never comes back and every column has at most one slot: ns <= n + 1 < cap = 4 * ((n + 64) & ~15).  test_pivot_ref.py
    reports the largest ns / cap over all cases and the fuzz sample (135 / 768 at n = 135; (n + 1) / cap stays below 0.25).  The checks stay in the kernel as
    bounds for rows whose indices are NOT sorted (copies of a column apart from each other take a slot each): undefined input, not built.
  * ILUCP's "pivot kept" branch in the SECOND pass: cannot happen.  The kept branch always returns the pivot (nU >= 1), so a second pass
    follows only a "pivoting" pass without candidates (cp/second) or a "neither" pass (cp/nrow0) and, the row being the same, takes the same
    branch again.
  * the order of tp_select's accL sum on its own: accL and accU are added in one loop, term by term, by one branch on the slot's class;
    unorm65 / unorm129 put a threshold on the edge between the orders of accU.  For accL the left arrow of norm65 / norm129 gives the
    multipliers v / 2, so nrmL is exactly half the load loop's norm and sits on the same edge, but no case separates the two sums.
  * the switch row at n - 1 (bp7, rp7) on the GPU: the last row's U part / the last step's row has one entry, which is taken whatever
    piv_tol says -- the same bits as without a switch (bp_none, rp_none).  bp6 / rp6 switch at n - 2, the last place that shows.
  * unsorted indices within a row or slice: the kernel's "stored twice" test looks at the neighbouring entry.  The reference sorts nothing
    and the oracle follows it; the Python classes hand over sorted arrays.
  * a NaN among the KEYS of a selection (wv_argmax_first's shuffle form): a NaN never is a candidate (NaN > norm * tau is false, and a NaN
    in the row makes the norm a NaN), so no input reaches it from these two kernels.  The nonfinite cases show inf keys and NaN values.
  * select_largest on more than a few hundred candidates, n beyond 300, the 2^31 reservation refusal: sizes, not boundaries of the chain.
  * pilucdp.hip: not here.  Its two chain kernels and their hand-over have a model, cases and tests of their own: tests/dp_ref.py,
    tests/dp_cases.py, tests/test_dp_ref.py, tests/test_gpu_dp_chains.py.  Of the helpers it shares, these cases run dp_subtract (both the prefetched first pass and the later ones),
    dp_seq_sum (mode 1), dp_sort_n, dp_touch, wv_argmax_first (integer form), wv_max_f64, wv_min_i32, select_largest and
    wave_sort_u64<true>; not dp_sort64, dp_node / dp_row / dp_ent, dp_seq_sum mode 0."""
import collections
import functools
import math

import numpy as np

import pivot_ref as R

Case = collections.namedtuple("Case", "kind build params pin")
DEFAULT = dict(fill_in=1000, threshold=0.0, piv_tol=0.0, rp=-1, mem_factor=10.0)


def par(**kw):
    d = dict(DEFAULT)
    d.update(kw)
    return d


def mag(j):
    """distinct magnitudes, exactly representable, alternating sign"""
    return (1.0 + (j % 100000) * 2.0 ** -20) * (1.0 if j % 2 == 0 else -1.0)


def irr(seed):
    """values whose squares are rounded: a sum of them depends on its order"""
    return lambda j: (1.0 + 1.0 / (j + 3.0 + seed)) * (-1.0 if j % 2 else 1.0) * 2.0 ** ((j % 5) - 2)


def slices(n, special, diag=2.0):
    """(indptr, indices, data): slice r is special[r] = [(index, value), ...] as written (sorted by the caller, copies allowed, [] = empty),
    every other slice its diagonal alone"""
    ptr, idx, val = [0], [], []
    for r in range(n):
        for c, v in (special[r] if r in special else [(r, diag)]):
            idx.append(c); val.append(v)
        ptr.append(len(idx))
    return np.array(ptr, dtype=np.int32), np.array(idx, dtype=np.int32), np.array(val, dtype=np.float64)


# ---- the order of a sum -------------------------------------------------------------------------------------------------------------------
def sums(terms):
    """the same terms added one after the other (what the kernels do, 64 per pass), in reverse, and pairwise"""
    seq = 0.0
    for t in terms:
        seq = seq + t
    rev = 0.0
    for t in reversed(terms):
        rev = rev + t
    p = list(terms)
    while len(p) > 1:
        p = [p[i] + p[i + 1] if i + 1 < len(p) else p[i] for i in range(0, len(p), 2)]
    return seq, rev, (p[0] if p else 0.0)


def edge_tau(a, terms, dec):
    """a threshold at which dec(a, tau * norm) with the norm of the ordered sum differs from both other orders, or None"""
    nr = [math.sqrt(x) for x in sums(terms)]
    if nr[0] in nr[1:]:
        return None
    t0 = a / nr[0]
    cand, up, dn = [t0], t0, t0
    for _ in range(64):
        up, dn = math.nextafter(up, math.inf), math.nextafter(dn, -math.inf)
        cand += [up, dn]
    for t in cand:
        d = [dec(a, t * x) for x in nr]
        if d[1] != d[0] and d[2] != d[0]:
            return t
    return None


def dropped(a, prod):       # tp_chain's drop test / its complement in the selections
    return a < prod


def selected(a, prod):
    return a > prod


@functools.lru_cache(maxsize=None)
def _edge(kind, m):
    """(seed of the values, threshold): the first seed for which the smallest-position entry sits on the edge between the orders"""
    for seed in range(200):
        v = irr(seed)
        if kind == "tp_left":       # the norm of the m original left entries, in column order; the entry of column 0 is tested first, as stored
            t = edge_tau(abs(v(0)), [v(c) * v(c) for c in range(m)], dropped)
        elif kind == "tp_top":      # tp_select's own sum over the U part of row 0, in slot = column order; the entry of column 1 is selected or not
            t = edge_tau(abs(v(1)), [v(c) * v(c) for c in range(m)], selected)
        elif kind == "cp_top":      # row 0: slots in DECREASING slice number (the list is pushed at its front); the entry of slice m - 1 leads
            vals = [4.0 if h == 0 else v(h) for h in range(m)]
            t = edge_tau(abs(vals[1]), [vals[h] * vals[h] for h in range(m - 1, -1, -1)], selected)
        else:                       # cp_leftcol: the m - 1 entries below the diagonal, in stored order, divided by nothing before the norm
            t = edge_tau(abs(v(1)), [v(r) * v(r) for r in range(1, m)], selected)
        if t is not None and 0.0 < t < 0.5:
            return seed, t
    raise AssertionError("no discriminating values for %s(%d)" % (kind, m))


# ---- ILUTP patterns -------------------------------------------------------------------------------------------------------------------------
def tp_left(m, vals=mag, extra=0):
    return lambda: slices(m + 1 + extra, {m: [(c, vals(c)) for c in range(m)] + [(m, 4.0)]})


def tp_min(ns):
    n = ns + 1
    last = [(0, 1.5)] + [(c, mag(c)) for c in range(2, ns)] + [(n - 1, 4.0)]
    return lambda: slices(n, {0: [(0, 2.0), (1, 1.0)], n - 1: last})


def tp_urow(ln, mixed=False, vals=mag):
    n = ln + 2
    row1 = [(0, 1.0), (1, 4.0)] + ([(c, 0.5) for c in range(2, ln + 2, 2)] if mixed else [])
    return lambda: slices(n, {0: [(0, 2.0)] + [(c, vals(c)) for c in range(2, ln + 2)], 1: row1})


def tp_top(w, slots, big=7.0):
    row = [(c, (big if slots.index(c) % 2 == 0 else -big) if c in slots else mag(c)) for c in range(w)]
    return lambda: slices(w, {0: row})


def bidiag(n):
    return lambda: slices(n, {r: [(r, 1.0), (r + 1, 3.0)] for r in range(n - 1)}, diag=1.0)


def raw(n, special, diag=2.0):
    return lambda: slices(n, special, diag)


def _tp_norm(m):
    seed, t = _edge("tp_left", m)
    return Case("tp", tp_left(m, irr(seed)), par(threshold=t), lambda res, f, rc: len(rc[-1]["norm_terms"]) == m and rc[-1]["stored"] == m + 1)


def _tp_unorm(m):
    seed, t = _edge("tp_top", m)
    v = irr(seed)
    return Case("tp", raw(m, {0: [(c, v(c)) for c in range(m)]}), par(threshold=t),
                lambda res, f, rc: len(rc[0]["selects"][0]["termsU"]) == m and rc[0]["selects"][0]["keep_diag"] and not rc[0]["selects"][0]["cutU"])


def _over(store):
    def pin(res, f, rc):
        r = rc[-1]
        need = (r["pL0"] + r["nL"] + 1) if store == "L" else (r["pU0"] + r["nU"])
        return res.err == R.ERR_MEMORY and res.err_store == store and need == r["reserved"] + 1
    return pin


def _fits(store):
    return lambda res, f, rc: res.err == R.OK and rc[-1]["p%s1" % store] == rc[-1]["reserved"]


def _tp_load(s):
    return Case("tp", tp_left(s - 1), par(),
                lambda res, f, rc: rc[-1]["stored"] == s == rc[-1]["distinct"] and len(rc[-1]["norm_terms"]) == s - 1 and rc[-1]["nL"] == s - 1)


def _tp_min(ns):
    return Case("tp", tp_min(ns), par(),
                lambda res, f, rc: rc[-1]["ns_load"] == ns and [e["ns"] for e in rc[-1]["elims"][:2]] == [ns, ns + 1]
                and rc[-1]["elims"][0]["slot"] == 0 and rc[-1]["elims"][1]["slot"] == ns >= R.PASS)


def _tp_usub(ln):
    return Case("tp", tp_urow(ln), par(),
                lambda res, f, rc: [(e["ulen"], e["new"], e["ns"]) for e in rc[1]["elims"]] == [(ln, ln, 2)] and rc[1]["selects"][0]["cU"] == ln + 1
                and f["append_across_pass"] == (ln + 2 > R.PASS))


def _tp_cut(n_L):
    return Case("tp", tp_left(70), par(fill_in=n_L + 1), lambda res, f, rc: rc[-1]["selects"][0]["cL"] == 70 and f["cutL"] == [n_L] and rc[-1]["nL"] == n_L)


def _tp_max(w, a, b, **kw):
    return Case("tp", tp_top(w, (a, b)), par(piv_tol=1.0, **kw),
                lambda res, f, rc: rc[0]["selects"][0]["max_slots"] == [a, b] and rc[0]["pivot_col"] == a and res.perm[0] == a)


def _tp_bp(n, rp, kept):
    return Case("tp", bidiag(n), par(rp=rp), lambda res, f, rc: [r["selects"][0]["keep_diag"] for r in rc] == [True] * kept + [False] * (n - kept))


_LONG = R.tp_cap(2)          # 256: the slots of the working row at n = 2


def tp_long(stored):
    """n = 2: row 1 stores column 0 128 times (1.0, the last copy 1.5) and column 1 stored - 128 times (the last copy 4.0).  The left norm
    sums ALL copies (sqrt(127 + 2.25) = 11.4), so with threshold 0.2 the kept value 1.5 < 2.27 is dropped; the last copy alone would not be"""
    row = [(0, 1.0)] * 127 + [(0, 1.5)] + [(1, 3.0)] * (stored - 129) + [(1, 4.0)]
    return lambda: slices(2, {0: [(0, 2.0), (1, 1.0)], 1: row})


TP = collections.OrderedDict()
# -- row load and left norm: a stored row of 1 .. 129 (the load loop's passes, the ordered left norm) --
for _s in (1, 63, 64, 65, 128, 129):
    TP["load%d" % _s] = _tp_load(_s)
TP["norm65"] = _tp_norm(65)          # the threshold sits between the norm of the ordered sum and those of the reversed and the pairwise sum:
TP["norm129"] = _tp_norm(129)        # the entry of column 0 is dropped or not by the ORDER of 65 / 129 terms (two / three passes)
TP["unorm65"] = _tp_unorm(65)        # the same for tp_select's norm of the U part (accU) over 65 / 129 slots: the entry of column 1 is a candidate or not
TP["unorm129"] = _tp_unorm(129)
# -- the smallest waiting position: found in slot ns, behind the slots loaded (ns = 64, 65, 129 at the first search, one more at the second) --
for _s in (64, 65, 129):
    TP["minsearch%d" % _s] = _tp_min(_s)
# -- subtraction of a U row of 0 .. 129 entries behind its pivot, all new: ns goes 2 -> 2 + len, across the pass edge from len = 63 on --
for _s in (0, 1, 63, 64, 65, 129):
    TP["usub%d" % _s] = _tp_usub(_s)          # (usub63 / usub64: cU = 64 / 65 as well)
TP["usub_mixed"] = Case("tp", tp_urow(100, mixed=True), par(), lambda res, f, rc: rc[1]["elims"][0]["new"] == 50 and rc[1]["elims"][0]["ulen"] == 100 and f["mixed_pass"])
# -- the drop test at equality: one left entry, threshold 1.0: |cur| = threshold * norm is NOT dropped (<); a dropped entry leaves a dead slot --
TP["drop_eq"] = Case("tp", raw(2, {1: [(0, 3.0), (1, 4.0)]}), par(threshold=1.0),
                     lambda res, f, rc: rc[1]["drops"] == 0 and rc[1]["kept_at_eq"] == [True] and len(rc[1]["elims"]) == 1 and rc[1]["second"])
TP["drop_dead"] = Case("tp", raw(3, {2: [(0, 2.0 ** -10), (1, 1.0), (2, 4.0)]}), par(threshold=0.1),
                       lambda res, f, rc: rc[2]["drops"] == 1 and rc[2]["dead"] == 1 and rc[2]["nL"] == 1 and rc[2]["ns"] == 3)
# -- selection counts and cuts --
TP["cl65"] = Case("tp", tp_left(65), par(), lambda res, f, rc: rc[-1]["selects"][0]["cL"] == 65)          # (cL = 64: load65; cL = 0: load1)
for _s in (0, 1, 63, 64):
    TP["cutL%d" % _s] = _tp_cut(_s)          # (n_L = 0: fill_in = 1, the `n_L > 0` guard)
TP["cutL_tie"] = Case("tp", tp_left(70, lambda c: 1.5 if c % 2 else -1.5), par(fill_in=6), lambda res, f, rc: f["tie_at_cut"] and f["cutL"] == [5])
TP["cutU"] = Case("tp", tp_top(12, ()), par(fill_in=3), lambda res, f, rc: rc[0]["selects"][0]["cU"] == 12 and rc[0]["selects"][0]["cutU"] and rc[0]["nU"] == 3)
TP["cutU_tie"] = Case("tp", raw(12, {0: [(c, 1.25 if c % 2 else -1.25) for c in range(12)]}), par(fill_in=4),
                      lambda res, f, rc: rc[0]["selects"][0]["tie_at_cutU"] and rc[0]["nU"] == 4 and rc[0]["selects"][0]["keep_diag"])
# -- the first of equal maxima: two lanes of one pass, one lane of two passes, different passes, and after a cut --
TP["max_3_9"] = _tp_max(20, 3, 9)
TP["max_6_70"] = _tp_max(80, 6, 70)
TP["max_3_70"] = _tp_max(80, 3, 70)
TP["max_70_130"] = _tp_max(135, 70, 130)
# three equal maxima, two kept: select_largest leaves one of them in FRONT of the cut (key[offU - 1] = the maximum), and the first of the
# two behind it is the pivot -- a search from 0 instead of offU, or a pivot taken from the dropped part, gives another column
TP["max_across_cut"] = Case("tp", tp_top(20, (3, 9, 12)), par(piv_tol=1.0, fill_in=2),
                            lambda res, f, rc: (lambda s: s["cU"] == 20 and s["offU"] == 18 and s["key_before_cut"] == s["max_key"] == 7.0
                                                and s["max_ties"] == [18, 19] and s["max_pos"] == 18)(rc[0]["selects"][0])
                            and rc[0]["pivot_col"] == 3 == res.perm[0] and sorted(res.U[1][res.U[2][0]:res.U[2][1]]) == [3, 9])      # (column 12 is the one left out)
TP["max_cut"] = Case("tp", tp_top(20, (3, 9)), par(piv_tol=1.0, fill_in=5),
                     lambda res, f, rc: rc[0]["selects"][0]["offU"] == 15 and len(rc[0]["selects"][0]["max_ties"]) == 2 and rc[0]["nU"] == 5)
# -- the diagonal against the largest: larg * piv_tol >= |diagonal| pivots (at equality too) --
TP["tol_eq"] = Case("tp", raw(2, {0: [(0, 2.0), (1, 4.0)], 1: [(0, 1.0), (1, 3.0)]}), par(piv_tol=0.5),
                    lambda res, f, rc: rc[0]["selects"][0]["at_tol"] and not rc[0]["selects"][0]["keep_diag"] and rc[0]["pivot_col"] == 1)
TP["tol_above"] = Case("tp", raw(2, {0: [(0, math.nextafter(2.0, 3.0)), (1, 4.0)], 1: [(0, 1.0), (1, 3.0)]}), par(piv_tol=0.5),
                       lambda res, f, rc: rc[0]["selects"][0]["keep_diag"] and rc[0]["pivot_col"] == 0)
TP["nodiag"] = Case("tp", raw(3, {0: [(1, 3.0), (2, -5.0)]}), par(), lambda res, f, rc: rc[0]["selects"][0]["diag_slot"] == -1 and rc[0]["pivot_col"] == 2)
TP["tol_neg"] = Case("tp", bidiag(6), par(piv_tol=-1.0), lambda res, f, rc: f["keep_diag"] == 6 and list(res.perm) == list(range(6)))
TP["bp0"] = _tp_bp(8, 0, 0)          # piv_tol = 0 keeps every diagonal, from the switch row on piv_tol = 1 takes the 3
TP["bp4"] = _tp_bp(8, 4, 4)
TP["bp6"] = _tp_bp(8, 6, 6)          # row n - 2 is the last whose U part has two positions: the last switch row that changes the factors
# (the switch at n - 1 only changes how the one-entry U part of the last row is selected -- not kept as the diagonal, taken as the largest --,
#  the same entry either way: bp7 has the bits of bp_none, the difference is in the model's record alone)
TP["bp7"] = Case("tp", bidiag(8), par(rp=7), lambda res, f, rc: f["keep_diag"] == 7 and not rc[7]["selects"][0]["keep_diag"])
TP["bp_none"] = _tp_bp(8, -1, 8)
# -- the second selection: threshold 0.8, a U part of two equal entries keeps none at first; a U part of one entry does --
TP["second"] = Case("tp", raw(3, {0: [(0, 1.0), (1, -1.0)], 1: [(1, 3.0)]}), par(threshold=0.8, piv_tol=1.0),
                    lambda res, f, rc: [r["second"] for r in rc] == [True, False, False] and rc[0]["nU"] == 2 and f["zp_new"] == f["zp_reuse"] == 0)
TP["second_skipped"] = Case("tp", raw(3, {1: [(0, 1.0)]}), par(threshold=0.0),          # threshold 0: no second selection, the pivot is inserted
                            lambda res, f, rc: not rc[1]["second"] and rc[1]["zp"] == "new" and res.zero_pivots == 1)
# -- the inserted pivot: a new slot (no U part), the slot of a stored 0.0, an empty row, n = 1 and 2 --
TP["zp_new"] = Case("tp", raw(3, {1: [(0, 1.0)]}), par(threshold=0.1), lambda res, f, rc: rc[1]["second"] and rc[1]["zp"] == "new" and rc[1]["ns"] == 2)
TP["zp_reuse"] = Case("tp", raw(3, {1: [(1, 0.0), (2, 0.0)]}), par(threshold=0.1, piv_tol=1.0),
                      lambda res, f, rc: rc[1]["zp"] == "reuse" and rc[1]["ns"] == 2 and res.zero_pivots == 1)
TP["empty_row"] = Case("tp", raw(3, {1: []}), par(threshold=0.1), lambda res, f, rc: rc[1]["stored"] == 0 and rc[1]["zp"] == "new" and rc[1]["ns"] == 1)
TP["all_empty"] = Case("tp", raw(3, {0: [], 1: [], 2: []}), par(), lambda res, f, rc: res.err == R.ERR_MEMORY and res.err_at == 0 and res.err_store == "L")
TP["n1"] = Case("tp", raw(1, {0: [(0, 5.0)]}), par(), lambda res, f, rc: res.err == R.OK and len(rc) == 1)
TP["n1_empty"] = Case("tp", raw(1, {0: []}), par(), lambda res, f, rc: res.err == R.ERR_MEMORY and res.err_at == 0)
TP["n2"] = Case("tp", raw(2, {0: [(0, 1.0), (1, 2.0)], 1: [(0, 3.0), (1, 4.0)]}), par(piv_tol=1.0), lambda res, f, rc: list(res.perm) == [1, 0])
# -- the stores: ILUTP checks L, then U.  mem_factor 1.0: as many entries as the matrix has --
TP["fitL"] = Case("tp", tp_left(5), par(mem_factor=1.0), _fits("L"))                              # 11 = nnz entries of L
TP["fitU"] = Case("tp", raw(6, {0: [(c, mag(c) + (3.0 if c == 0 else 0.0)) for c in range(6)]}), par(mem_factor=1.0), _fits("U"))
TP["overL"] = Case("tp", raw(8, {0: [], 1: [], 2: [], 5: [(3, 1.0), (4, 1.0), (5, 4.0)]}), par(mem_factor=1.0),      # three inserted pivots: L is 1 past nnz in row 5
                   lambda res, f, rc: _over("L")(res, f, rc) and res.err_at == 5)
TP["overU"] = Case("tp", raw(6, {0: [(0, 2.0), (4, 1.0), (5, 1.0)], 3: [(0, 1.0), (3, 4.0)], 4: [], 5: []}), par(mem_factor=1.0),
                   lambda res, f, rc: _over("U")(res, f, rc) and res.err_at == 3)
TP["mem05"] = Case("tp", tp_left(3), par(mem_factor=0.5), lambda res, f, rc: res.err == R.ERR_MEMORY and res.err_at == 0 and rc[0]["reserved"] == 0)
TP["mem19"] = Case("tp", raw(8, {0: [], 1: [], 2: [], 5: [(3, 1.0), (4, 1.0), (5, 4.0)]}), par(mem_factor=1.9),      # 1.9 is 1: overL again (2 x nnz would hold it)
                   lambda res, f, rc: _over("L")(res, f, rc) and res.err_at == 5 and rc[0]["reserved"] == 7)
TP["fill0"] = Case("tp", tp_left(5), par(fill_in=0), lambda res, f, rc: rc[0]["reserved"] == 6 and f["max_nL"] == 0 and f["cutL"] == [0] and res.err == R.OK)
TP["fill_big"] = Case("tp", tp_left(5), par(fill_in=10 ** 6, mem_factor=100.0), lambda res, f, rc: rc[0]["reserved"] == 36 and res.err == R.OK)
# -- "encountered zero pivot in row r": a stored 0.0 on the diagonal that a negative piv_tol keeps (its magnitude becomes the norm) --
TP["zperr0"] = Case("tp", raw(3, {0: [(0, 0.0), (1, 1.0)]}), par(threshold=0.1, piv_tol=-0.5), lambda res, f, rc: res.err == R.ERR_ZERO_PIVOT and res.err_at == 0)
TP["zperr_last"] = Case("tp", raw(4, {2: [(2, 0.0), (3, 1.0)]}), par(threshold=0.1, piv_tol=-0.5), lambda res, f, rc: res.err == R.ERR_ZERO_PIVOT and res.err_at == 2)
# -- a column stored twice: one slot, the LAST value, every copy in the left norm --
TP["dup_pass"] = Case("tp", raw(3, {2: [(0, 1.0), (0, 3.0), (1, 0.5), (2, 4.0)]}), par(threshold=0.1), lambda res, f, rc: rc[2]["stored"] == 4 and rc[2]["distinct"] == 3)
TP["dup_6364"] = Case("tp", raw(70, {69: [(c, mag(c)) for c in range(63)] + [(63, 1.0), (63, -3.0), (69, 4.0)]}), par(threshold=0.01),
                      lambda res, f, rc: rc[-1]["stored"] == 66 and rc[-1]["distinct"] == 65)
TP["dup3"] = Case("tp", raw(3, {2: [(0, 1.0), (1, 0.5), (1, -2.0), (1, 0.25), (2, 4.0)]}), par(threshold=0.1), lambda res, f, rc: rc[2]["stored"] == 5 and rc[2]["distinct"] == 3)
TP["dup_long256"] = Case("tp", tp_long(_LONG), par(threshold=0.2),            # stored = cap: the kernel of before refused cap + 1 (status 12)
                         lambda res, f, rc: rc[1]["stored"] == _LONG == 256 and rc[1]["distinct"] == 2 and rc[1]["drops"] == 1 and res.err == R.OK)
TP["dup_long257"] = Case("tp", tp_long(_LONG + 1), par(threshold=0.2),
                         lambda res, f, rc: rc[1]["stored"] == _LONG + 1 and rc[1]["distinct"] == 2 and rc[1]["drops"] == 1 and res.err == R.OK)
TP["dup_long300"] = Case("tp", raw(2, {1: [(0, mag(q)) for q in range(150)] + [(1, mag(q) + 2.0) for q in range(150)]}), par(threshold=0.1),
                         lambda res, f, rc: rc[1]["stored"] == 300 and rc[1]["distinct"] == 2 and res.err == R.OK)
# -- values that overflow: inf multipliers, inf - inf in the working row --
TP["nonfinite"] = Case("tp", raw(3, {0: [(0, 1e-150), (2, 1e150)], 1: [(1, 1e-150), (2, -1e150)], 2: [(0, 1e150), (1, 1e150), (2, 1.0)]}), par(),
                       lambda res, f, rc: f["nonfinite"] and res.err == R.OK and rc[2]["zp"] == "reuse")       # column 2 of row 2: 1 - inf + inf

# the copies of these cases swapped (name -> the two entries of `data` to exchange): other bits from the oracle
TP_SWAPS = {"dup_pass": (0, 1), "dup_6364": (63, 64), "dup3": (2, 3), "dup_long257": (256, 255), "dup_long300": (150 + 149, 150 + 148)}


# ---- ILUCP patterns -------------------------------------------------------------------------------------------------------------------------
def cp_top(w, down=(), vals=mag, n=None, d0=4.0):
    """slice h (0 < h < w) = {0: vals(h), h: 2}; slice 0 = {0: d0} and the rows `down`: row 0 has w entries, its U row is subtracted from
    the rows `down`"""
    n = max(w, max(down, default=0) + 1) if n is None else n
    sp_ = {h: [(0, vals(h)), (h, 2.0)] for h in range(1, w)}
    sp_[0] = [(0, d0)] + [(r, 1.0 + 0.25 * q) for q, r in enumerate(sorted(down))]
    return lambda: slices(n, sp_)


def cp_leftcol(m, vals=mag, n=None, dups=()):
    """slice 0 = rows 0 .. m - 1 (the copies `dups` = [(position in the slice, row, value)] put in), every other slice its diagonal"""
    ent = [(0, 4.0)] + [(r, vals(r)) for r in range(1, m)]
    for pos, r, v in sorted(dups, reverse=True):
        ent.insert(pos, (r, v))
    return lambda: slices(m if n is None else n, {0: ent})


def cp_bidiag(n):
    """the matrix {r: 1, r + 1: 3} by its columns: slice h = {h - 1: 3, h: 1}"""
    return lambda: slices(n, {h: [(h - 1, 3.0), (h, 1.0)] for h in range(1, n)}, diag=1.0)


def cp_chains(n):
    """slices sharing first rows (h % 3 for h >= 3), every 50th slice from 10 on empty"""
    sp_ = {h: [(h % 3, mag(h)), (h, 4.0)] for h in range(3, n)}
    for h in range(10, n, 50):
        sp_[h] = []
    return lambda: slices(n, sp_)


def cp_bottom():
    """slices 0 .. 69 = {h, 100}, slices 100 .. 104 = {100, ...}: the list of row 100 holds 70 columns that have been pivots and 5 that have not"""
    sp_ = {h: [(h, 2.0), (100, mag(h))] for h in range(70)}
    sp_.update({h: [(100, mag(h))] + ([(h, 2.0)] if h > 100 else []) for h in range(100, 105)})
    sp_[100] = [(100, 4.0)]
    return lambda: slices(105, sp_)


def cp_filtcol():
    """slice 70 = rows 0 .. 140: at step 70 its 71 entries of rows <= 70 are filtered, the 70 below make the L column"""
    return lambda: slices(141, {70: [(r, 4.0 if r == 70 else mag(r) * 0.5) for r in range(141)]})


def _sel(rc, k, q=0):
    return rc[k]["selects"][q]


def _cp_nrow(w):
    return Case("cp", cp_top(w, down=(1, 2, 3), n=max(w, 4)), par(),
                lambda res, f, rc: rc[0]["nrow"] == w == rc[0]["znnz"] and rc[1]["zsubs"] == [dict(len=w, dead=1, new=max(w - 2, 0), ns=1)]
                and (w < 4 or f["zsub_dead"] >= 2) and f["append_across_pass"] == (w > R.PASS + 1))


def _cp_nl(nl):
    return Case("cp", cp_leftcol(nl + 1, n=max(nl + 1, 2)), par(), lambda res, f, rc: rc[0]["nL"] == nl == rc[0]["cntL"] and rc[0]["col_len"] == nl + 1)


def _cp_max(w, a, b):
    """equal maxima at the slots a < b of row 0: slot s holds slice w - 1 - s"""
    cols = (w - 1 - a, w - 1 - b)
    return Case("cp", cp_top(w, vals=lambda h: (7.0 if h == cols[0] else -7.0) if h in cols else mag(h)), par(piv_tol=1.0),
                lambda res, f, rc: _sel(rc, 0)["branch"] == "pivoting" and _sel(rc, 0)["max_ties"] == [a, b] and rc[0]["pivot_col"] == cols[0])


def _cp_norm(kind, m):
    seed, t = _edge(kind, m)
    if kind == "cp_top":
        return Case("cp", cp_top(m, vals=irr(seed)), par(threshold=t), lambda res, f, rc: len(_sel(rc, 0)["terms"]) == m and _sel(rc, 0)["branch"] == "kept")
    return Case("cp", cp_leftcol(m, vals=irr(seed)), par(threshold=t), lambda res, f, rc: len(rc[0]["wterms"]) == m - 1)


def _cp_rp(n, rp, kept):
    return Case("cp", cp_bidiag(n), par(rp=rp), lambda res, f, rc: [_sel(rc, k)["branch"] for k in range(n)] == ["kept"] * kept + ["pivoting"] * (n - 1 - kept) + ["kept"])


CP = collections.OrderedDict()
# -- the list of row k: nrow = 1, 64, 65 (129: three passes) and the U row of that length subtracted from a later row: the first pass of
#    dp_subtract is fetched ahead, later passes are read in the loop; the pivot of step 0 is dead (-2) in it and must stay so after the reset --
for _s in (1, 64, 65, 129):
    CP["nrow%d" % _s] = _cp_nrow(_s)
CP["nrow0"] = Case("cp", raw(3, {1: []}), par(threshold=0.1), lambda res, f, rc: rc[1]["nrow"] == 0 and rc[1]["zp"] and rc[1]["col_len"] == 0
                   and [s["branch"] for s in rc[1]["selects"]] == ["neither", "neither"])
CP["filtered"] = Case("cp", cp_bottom(), par(), lambda res, f, rc: rc[100]["nrow"] == 75 and rc[100]["nonpiv"] == 5)
for _s in (255, 256, 257):
    CP["chains%d" % _s] = Case("cp", cp_chains(_s), par(threshold=0.01), lambda res, f, rc, n=_s: rc[0]["nrow"] == len(range(3, n, 3)) + 1 - len([h for h in range(10, n, 50) if h % 3 == 0]))
CP["norm65"] = _cp_norm("cp_top", 65)
CP["norm129"] = _cp_norm("cp_top", 129)
# -- the three branches of the selection --
CP["tol_eq"] = Case("cp", raw(2, {0: [(0, 2.0)], 1: [(0, 4.0), (1, 3.0)]}), par(piv_tol=0.5),       # best * piv_tol = |at_pivot|: not >, the pivot is kept
                    lambda res, f, rc: _sel(rc, 0)["at_tol"] and _sel(rc, 0)["branch"] == "kept" and rc[0]["pivot_col"] == 0)
CP["tol_below"] = Case("cp", raw(2, {0: [(0, math.nextafter(2.0, 1.0))], 1: [(0, 4.0), (1, 3.0)]}), par(piv_tol=0.5),
                       lambda res, f, rc: _sel(rc, 0)["branch"] == "pivoting" and rc[0]["pivot_col"] == 1)
CP["piv_lim"] = Case("cp", cp_top(6, d0=0.5), par(piv_tol=1.0, fill_in=6), lambda res, f, rc: (_sel(rc, 0)["branch"], _sel(rc, 0)["cnt"], _sel(rc, 0)["cut"]) == ("pivoting", 6, False))
CP["piv_lim1"] = Case("cp", cp_top(6, n=8, d0=0.5), par(piv_tol=1.0, fill_in=5), lambda res, f, rc: (_sel(rc, 0)["branch"], _sel(rc, 0)["cnt"], _sel(rc, 0)["cut"]) == ("pivoting", 6, True))
CP["kept_lim_1"] = Case("cp", cp_top(6), par(fill_in=6), lambda res, f, rc: (_sel(rc, 0)["branch"], _sel(rc, 0)["cnt"], _sel(rc, 0)["cut"]) == ("kept", 5, False))
CP["kept_lim"] = Case("cp", cp_top(6, n=8), par(fill_in=5), lambda res, f, rc: (_sel(rc, 0)["branch"], _sel(rc, 0)["cnt"], _sel(rc, 0)["cut"]) == ("kept", 5, True))
CP["piv_fill1"] = Case("cp", cp_top(6, d0=0.5), par(piv_tol=1.0, fill_in=1), lambda res, f, rc: ("pivoting", 6, 1) in f["cuts"] and rc[0]["nU"] == 1)
CP["kept_fill1"] = Case("cp", cp_top(6), par(fill_in=1), lambda res, f, rc: ("kept", 5, 1) in f["cuts"] and rc[0]["nU"] == 1 and rc[0]["pivot_col"] == 0)
CP["cut_tie"] = Case("cp", cp_top(12, vals=lambda h: 1.5 if h % 2 else -1.5, d0=0.5), par(piv_tol=1.0, fill_in=4),
                     lambda res, f, rc: _sel(rc, 0)["tie_at_cut"] and _sel(rc, 0)["branch"] == "pivoting")
CP["kept_cut_tie"] = Case("cp", cp_top(12, vals=lambda h: 1.5 if h % 2 else -1.5), par(fill_in=4), lambda res, f, rc: _sel(rc, 0)["tie_at_cut"] and _sel(rc, 0)["branch"] == "kept")
CP["max_3_9"] = _cp_max(20, 3, 9)
CP["max_6_70"] = _cp_max(80, 6, 70)
CP["max_3_70"] = _cp_max(80, 3, 70)
CP["max_70_130"] = _cp_max(135, 70, 130)
CP["second"] = Case("cp", raw(3, {0: [(0, 1.0)], 1: [(0, -2.0), (1, 3.0)], 2: [(0, 2.0), (2, 3.0)]}), par(threshold=0.8, piv_tol=1.0),      # row 0 = {1, -2, 2}: nothing above 0.8 * 3; tau = 0 takes all
                    lambda res, f, rc: [s["branch"] for s in rc[0]["selects"]] == ["pivoting", "pivoting"] and rc[0]["nU"] == 3 and not rc[0]["zp"] and rc[0]["pivot_col"] == 2)
CP["rp0"] = _cp_rp(8, 0, 0)
CP["rp4"] = _cp_rp(8, 4, 4)
CP["rp6"] = _cp_rp(8, 6, 6)          # step n - 2 is the last with two columns that have not been pivots: the last switch step that changes the factors
# (at step n - 1 one column is left, best = |at_pivot| and best * 1 > |at_pivot| is false: rp7 takes the branches and has the bits of rp_none)
CP["rp7"] = _cp_rp(8, 7, 7)
CP["rp_none"] = _cp_rp(8, -1, 7)
# -- the L column: the pivot's stored column of 0 (nrow0), 64, 65 entries; nL = 0 .. 129 (dp_sort_n up to 64, wave_sort_u64 on 128 and 256 above) --
for _s in (0, 1, 63, 64, 65, 128, 129):
    CP["nL%d" % _s] = _cp_nl(_s)
CP["wnorm65"] = _cp_norm("cp_leftcol", 66)
CP["wnorm129"] = _cp_norm("cp_leftcol", 130)
CP["filtcol"] = Case("cp", cp_filtcol(), par(), lambda res, f, rc: rc[70]["col_len"] == 141 and rc[70]["col_below"] == 70 == rc[70]["nL"])
CP["wsub"] = Case("cp", cp_top(3, down=tuple(range(1, 131)), n=131), par(),      # the L column of step 0 (131 entries) is subtracted from the columns 1 and 2
                  lambda res, f, rc: rc[1]["wsubs"] == [dict(len=131, new=131, ns=0)] and 131 in f["wsub_lens"] and f["append_across_pass"])
CP["dup_pass"] = Case("cp", cp_leftcol(6, dups=[(2, 1, 3.0)]), par(threshold=0.1), lambda res, f, rc: rc[0]["col_dups"] == 1 and rc[0]["col_len"] == 7 and rc[0]["wnnz"] == 5)
CP["dup_6364"] = Case("cp", cp_leftcol(70, dups=[(64, 63, -3.0)]), par(threshold=0.01), lambda res, f, rc: rc[0]["col_dups"] == 1 and rc[0]["col_len"] == 71)
CP["dup3"] = Case("cp", cp_leftcol(6, dups=[(3, 2, -2.0), (3, 2, 0.25)]), par(threshold=0.1), lambda res, f, rc: rc[0]["col_dups"] == 2 and rc[0]["wnnz"] == 5)
CP["cutL0"] = Case("cp", cp_leftcol(6), par(fill_in=1), lambda res, f, rc: rc[0]["cntL"] == 5 and rc[0]["limL"] == 0 and rc[0]["nL"] == 0)
CP["cutL_tie"] = Case("cp", cp_leftcol(70, vals=lambda r: 1.5 if r % 2 else -1.5), par(fill_in=6), lambda res, f, rc: rc[0]["tie_at_cutL"] and rc[0]["nL"] == 5)
CP["cutL65"] = Case("cp", cp_leftcol(100), par(fill_in=66), lambda res, f, rc: rc[0]["cntL"] == 99 and rc[0]["nL"] == 65)
# -- the stores: ILUCP checks U, then L --
CP["fit_both"] = Case("cp", cp_leftcol(6), par(fill_in=1), lambda res, f, rc: rc[-1]["pU1"] == rc[-1]["pL1"] == rc[-1]["reserved"] == 6)
CP["fitL"] = Case("cp", cp_leftcol(5, n=6), par(mem_factor=1.0), _fits("L"))
CP["overU"] = Case("cp", raw(4, {2: []}), par(mem_factor=1.0), lambda res, f, rc: _over("U")(res, f, rc) and res.err_at == 3)
CP["overL"] = Case("cp", raw(5, {0: [(0, 4.0), (1, 1.0), (2, 1.25), (3, 1.5)], 3: []}), par(mem_factor=1.0),
                   lambda res, f, rc: _over("L")(res, f, rc) and res.err_at == 4)
CP["mem05"] = Case("cp", cp_leftcol(4), par(mem_factor=0.5), lambda res, f, rc: res.err == R.ERR_MEMORY and res.err_at == 0 and res.err_store == "U")
CP["all_empty"] = Case("cp", raw(3, {0: [], 1: [], 2: []}), par(), lambda res, f, rc: res.err == R.ERR_MEMORY and res.err_at == 0 and res.err_store == "U")
CP["n1"] = Case("cp", raw(1, {0: [(0, 5.0)]}), par(), lambda res, f, rc: res.err == R.OK)
CP["n2"] = Case("cp", raw(2, {0: [(0, 1.0), (1, 3.0)], 1: [(0, 2.0), (1, 4.0)]}), par(piv_tol=1.0), lambda res, f, rc: list(res.perm) == [1, 0])
CP["nonfinite"] = Case("cp", raw(4, {0: [(0, 1e-150), (2, 1e150)], 1: [(1, 1e-150), (2, 1e150)], 2: [(2, 1.0)], 3: [(0, 1e150), (1, -1e150), (3, 1.0)]}), par(),
                       lambda res, f, rc: rc[2]["nonfinite"] and res.err == R.OK and rc[2]["nU"] == 1 and not rc[2]["zp"])      # row 2, column 3: 0 - inf + inf; the pivot 1.0 is kept

CP_SWAPS = {"dup_pass": (1, 2), "dup_6364": (63, 64), "dup3": (3, 4)}
SWAPS = dict([("tp/" + k, v) for k, v in TP_SWAPS.items()] + [("cp/" + k, v) for k, v in CP_SWAPS.items()])


def _order(kind, m, terms, first, dec):
    return (m, terms, abs(irr(_edge(kind, m)[0])(first)), dec)


# the ordered sums: name -> (number of terms, the record's terms, the magnitude on the edge, the test it is put to); test_pivot_ref.py
# shows that the reversed and the pairwise sum of the same terms have other bits AND decide the other way
ORDERS = {"tp/unorm65": _order("tp_top", 65, lambda rc: rc[0]["selects"][0]["termsU"], 1, selected),
          "tp/unorm129": _order("tp_top", 129, lambda rc: rc[0]["selects"][0]["termsU"], 1, selected),
          "tp/norm65": _order("tp_left", 65, lambda rc: rc[-1]["norm_terms"], 0, dropped),
          "tp/norm129": _order("tp_left", 129, lambda rc: rc[-1]["norm_terms"], 0, dropped),
          "cp/norm65": _order("cp_top", 65, lambda rc: rc[0]["selects"][0]["terms"], 1, selected),
          "cp/norm129": _order("cp_top", 129, lambda rc: rc[0]["selects"][0]["terms"], 1, selected),
          "cp/wnorm65": (65,) + _order("cp_leftcol", 66, lambda rc: rc[0]["wterms"], 1, selected)[1:],
          "cp/wnorm129": (129,) + _order("cp_leftcol", 130, lambda rc: rc[0]["wterms"], 1, selected)[1:]}

CASES = collections.OrderedDict([("tp/" + k, v) for k, v in TP.items()] + [("cp/" + k, v) for k, v in CP.items()])
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def arrays(name):
    ptr, idx, val = CASES[name].build()
    for a in (ptr, idx, val):
        a.setflags(write=False)
    return ptr, idx, val


@functools.lru_cache(maxsize=None)
def model(name):
    """the CPU model's result for a case (computed once, shared by the tests)"""
    c = CASES[name]
    ptr, idx, val = arrays(name)
    return (R.ilutp if c.kind == "tp" else R.ilucp)(ptr, idx, val, **c.params)
