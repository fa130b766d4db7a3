"""The cases of tests/test_gpu_ilut_tiers.py, by name: every one is a designed pattern that puts ONE row of the wave-parallel ILUT kernel
(ilupp_amd/csrc/ilut_wp.hip) on one side of one boundary, so that every figure is exact and the model of tests/ilut_ref.py stays fast.
tests/test_ilut_ref.py asserts, on the CPU, the figures that put each case there (CASES[name].pin) and the route written beside it.

  arrow(left, right)   every row is its diagonal alone but one, which has `left` entries left and `right` entries right of its diagonal:
                       no fill, the demands are the counts, every left entry is one elimination with a U row of length 1
  chain(e)             rows k = {k: 1, k + 1: -1} and a last row {0: 1, e: 4}: e eliminations, each makes exactly one fill entry of
                       magnitude 1 -- the pool holds one or two entries, the kept list grows to e (all multipliers equal: the L row's cut
                       falls between equal magnitudes and the sort decides); distinct=True gives the multipliers distinct magnitudes
  midrow(), forget(m), shape(ul, cntL), hashmove(R), collide(), reuse(), band()   see there

A route is (outgrew, pool, uslots, kept, left_tier2, status, big) as ilut_ref.route returns it.

NOT pinned, with the reason:
  * the overflow of the 16-bit sequence numbers (`seq + popc(mL) > 65535`): a column enters a row's left part at most once (fill only
    lands right of the column just eliminated), so it takes a row with more than 65 535 left insertions of which at most 32 768 are
    in the pool at a time and at most 32 768 are kept -- tens of thousands of entries that are inserted and forgotten again.  No
    small pattern reaches it; the model refuses to predict a route through it (ilut_ref.route).
  * `nU + p` = 2 048 / 2 049 in tier 3: the same code as in tier 2 (wp_row<true>), reached here only in the process with
    ILUPP_ILUT_NO_TIER2=1 (hashmove2048 / hashmove2049 are on its list).
  * a row that follows a row whose hash MOVED to the whole table (`nU + p > 2048`) on the same wave: `reuse` makes rows follow rows that
    START on the whole table (a row of A above 1 024 entries); the move itself is run by hashmove2049, alone on its wave.
  * the hash move and the walk past a collision have no counter: the model says where they happen (ilut_ref.hash_moves, walks), the
    GPU test can only show the bits.
  * the timeout, values with the sentinel's bit pattern, anything that makes a wave wait: out of scope, no case builds such an input."""
import collections
import functools

import numpy as np
import scipy.sparse as sp

import ilut_ref as R

Case = collections.namedtuple("Case", "build p tau route pin")
OK = (0, 0, 0, 0, 0, 0, False)


def mag(j):
    """distinct magnitudes, exactly representable, alternating sign"""
    return (1.0 + (j % 100000) * 2.0 ** -20) * (1.0 if j % 2 == 0 else -1.0)


def _csr(n, special, diag=2.0):
    """rows of `special` = {row: {column: value}}, every other row its diagonal alone"""
    lens = np.ones(n, dtype=np.int64)
    for r, d in special.items():
        lens[r] = len(d)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    idx = np.empty(ptr[-1], dtype=np.int32)
    val = np.empty(ptr[-1], dtype=np.float64)
    plain = np.ones(n, dtype=bool)
    plain[list(special)] = False
    idx[ptr[:-1][plain]] = np.nonzero(plain)[0]
    val[ptr[:-1][plain]] = diag
    for r, d in special.items():
        c = np.array(sorted(d), dtype=np.int32)
        idx[ptr[r]:ptr[r + 1]] = c
        val[ptr[r]:ptr[r + 1]] = [d[int(x)] for x in c]
    return sp.csr_matrix((val, idx, ptr.astype(np.int32)), shape=(n, n))


def arrow(left, right, lvals=None, rvals=None, n=None):
    i = left
    n = i + right + 9 if n is None else n
    row = {i: 4.0}
    for c in range(left):
        row[c] = mag(c) if lvals is None else lvals(c)
    for t in range(right):
        row[i + 1 + t] = mag(t + 1) if rvals is None else rvals(t)
    return _csr(n, {i: row})


def tiny_left(c):
    """four live entries, the rest below the stage-1 threshold (tau = 1e-3): forgotten, never eliminated -- the boundary is the scatter's"""
    return mag(c) if c < 4 else 1e-9


def chain(e, distinct=False):
    r = (lambda k: 1.0 + k * 2.0 ** -20) if distinct else (lambda k: 1.0)
    ptr = np.arange(0, 2 * (e + 1) + 1, 2, dtype=np.int32)
    idx = np.empty(2 * (e + 1), dtype=np.int32)
    val = np.empty(2 * (e + 1), dtype=np.float64)
    k = np.arange(e)
    idx[0:2 * e:2] = k; idx[1:2 * e:2] = k + 1
    val[0:2 * e:2] = 1.0
    val[1:2 * e:2] = -np.array([r(q + 1) / r(q) for q in range(e)])
    idx[2 * e:] = (0, e); val[2 * e:] = (1.0, 4.0)
    return sp.csr_matrix((val, idx, ptr), shape=(e + 1, e + 1))


def midrow():
    """p = 10: row 600 has 490 left entries (tier 2: 490 + 10 <= 512); rows 0, 1, 2 have nine entries each at columns 490 ... 516 that the
    pool does not hold, so after two eliminations it holds 506 and `nL + p > 512` moves it, with two multipliers kept"""
    sp_ = {600: dict([(c, mag(c)) for c in range(490)] + [(600, 4.0), (601, 1.5)])}
    for k in range(3):
        sp_[k] = dict([(k, 2.0)] + [(490 + 9 * k + t, mag(t + 3)) for t in range(9)])
    return _csr(604, sp_)


def forget(m):
    """tau = 0.1: row i has live entries at columns 0, m + 1, m + 2 and five more behind them, and m entries of 1e-6 at columns 1 .. m.
    Column 0 is eliminated, then m + 1 -- the m small ones lie left of it and are forgotten --, and the pass of the THIRD elimination
    finds them: nd = m"""
    i = m + 8
    row = {0: 1.0, i: 4.0, i + 1: 1.25, i + 2: -1.5, i + 3: 1.75}
    for c in range(1, m + 1):
        row[c] = 1e-6
    for c in range(m + 1, m + 8):
        row[c] = mag(c)
    return _csr(i + 6, {i: row})


def shape(ul, cntL):
    """row 0 of U has ul entries, cntL of them (its diagonal included) left of the diagonal of row i; row i holds every second of those
    columns on either side (hits) and not the others (misses); the rows between are their diagonals (U rows of length 1: cntL = 1)"""
    i = max(cntL, 2) + 3
    nright = ul - cntL
    row0 = {0: 2.0}
    rowi = {0: 1.5, i: 4.0}
    for t in range(1, cntL):
        row0[t] = mag(t)
        if t % 2 == 0:
            rowi[t] = mag(t + 7)
    for t in range(nright):
        row0[i + 1 + t] = mag(t + 5)
        if t % 2 == 0:
            rowi[i + 1 + t] = mag(t + 11)
    return _csr(i + nright + 4, {0: row0, i: rowi})


SHAPES = [(4, 1), (5, 2), (7, 4), (8, 5), (11, 8), (12, 9), (16, 16), (17, 9), (64, 30), (65, 30), (130, 70)]


def hashmove(Rn):
    """p = 256: rows 0 .. 6 have 255 entries right of the diagonal in seven disjoint blocks, rows 7, 8, 9 the blocks of rows 0, 1, 2 again;
    row 10 has all ten to its left and Rn entries of its own to its right: after seven eliminations it has Rn + 1 785 U slots, and the
    last three eliminations find every column in the hash"""
    sp_ = {}
    for k in range(10):
        sp_[k] = dict([(k, 2.0)] + [(20 + 255 * (k % 7) + t, mag(t + k)) for t in range(255)])
    sp_[10] = dict([(k, mag(k)) for k in range(10)] + [(10, 4.0)] + [(11 + t, mag(t + 2)) for t in range(Rn)])
    return _csr(20 + 255 * 7 + 5, sp_)


def colliding(count=4, first=200, mask=R.HASH_SMALL - 1):
    """the first `count` columns >= first that share a home cell in a table of mask + 1 cells (consecutive columns never do: the hash is
    multiplicative)"""
    by = {}
    for c in range(first, first + 200000):
        s = by.setdefault(R.wp_hash(c, mask), [])
        s.append(c)
        if len(s) == count:
            return s
    raise AssertionError("no collision")


def collide():
    """p = 10: row 5 has 130 consecutive columns and three of four columns S that share a home cell of the small global table to its right
    (tier 2: 133 U slots), and column 0 to its left; U's row 0 holds S[1] (a hit found behind S[0]'s cell) and S[3] (a miss: the walk passes
    three taken cells and the column goes into the fourth)"""
    S = colliding()
    row5 = dict([(0, 1.5), (5, 4.0)] + [(6 + t, mag(t)) for t in range(130)] + [(S[0], 1.25), (S[1], -1.75), (S[2], 2.25)])
    return _csr(S[3] + 4, {0: {0: 2.0, S[1]: 0.5, S[3]: -0.75}, 5: row5})


REUSE_PIVOTS, REUSE_ROWS, REUSE_X = 4, 300, 400


def reuse_len(j):
    """entries right of the diagonal of the j-th table row: fewer in every later row, all above 1 024"""
    return 1400 - j


def reuse_pivot_columns(k):
    """the 31 columns of pivot row k: ten inside every table row's block (hits), ten in the range where the blocks end (a hit in the longer
    rows, a miss in the shorter), eleven beyond every block (misses; pivot 3 repeats those of pivot 0: hits on fill)"""
    X = REUSE_X
    return ([X + 100 * t + 7 * k for t in range(10)] + [X + 1105 + 29 * t + 3 * k for t in range(10)] +
            [X + 1400 + 10 * t + k % 3 for t in range(11)])


def reuse():
    """p = 32.  Rows 0 .. 3 are pivot rows with 31 entries right of the diagonal.  The 300 TABLE rows 4 .. 303 each have columns 0 .. 3 to
    their left and the block of columns X .. X + 1 399 - j to their right (j = 0 .. 299): a row of A above 1 024 entries, so its U-slot hash
    starts on the WHOLE table of its wave (tier 2: 128 U slots do not hold it), and four eliminations whose 124 lookups hit and miss.
    Every table row is both a whole-table row and a row that looks columns up, so a launch with fewer than 300 waves makes some wave take
    one after another, whatever the assignment.  What a cell left behind does to the later row B (fewer slots than the earlier row A, rows
    are handed out in ascending order): the cell of a column c that B misses names a slot t of A with t >= nU of B at that moment -- t - nU
    is the difference of the block lengths less the columns of the pivots between the two block ends, which are distinct integers in that
    gap --, the slot still holds A's column c, the lookup takes it for a hit and the fill entry (magnitude 8: among the 31 kept) is lost"""
    X = REUSE_X
    sp_ = {}
    for k in range(REUSE_PIVOTS):
        sp_[k] = dict([(k, 2.0)] + [(c, 16.0 * (1.0 if q % 2 else -1.0)) for q, c in enumerate(reuse_pivot_columns(k))])
    for j in range(REUSE_ROWS):
        i = REUSE_PIVOTS + j
        sp_[i] = dict([(k, mag(k + j)) for k in range(REUSE_PIVOTS)] + [(i, 4.0)] + [(X + t, mag(t + j)) for t in range(reuse_len(j))])
    return _csr(X + 1520, sp_)


def band(n=300):
    """five diagonals (-2, -1, 0, 1, 3) with a dominant main one: fill inside the band"""
    rng = np.random.default_rng(300)
    M = sp.diags([rng.uniform(0.2, 1.0, n - 2), -rng.uniform(0.2, 1.0, n - 1), rng.uniform(4.0, 5.0, n), rng.uniform(0.2, 1.0, n - 1),
                  -rng.uniform(0.2, 1.0, n - 3)], [-2, -1, 0, 1, 3], format="csr")
    M.sort_indices()
    return M


# ---- the pins: what the model's records must show for the case to be where its name says ----------------------------------------------
def _the_row(rows, i):
    assert rows[i] is not None, i
    return rows[i]


def _long_row(rows):
    """the one row of an arrow or a chain with a record of more than a diagonal's worth"""
    c = [r for r in rows if r is not None and (r["elims"] or r["alen"] > 2)]
    return max(c, key=lambda r: (len(r["elims"]), r["alen"]))


def pin_counts(left=None, right=None, nK=None):
    def f(rows, ev, p):
        r = _long_row(rows)
        if left is not None: assert sum(a for a, _ in r["scatter"]) == left and r["tops"][0][0] == left
        if right is not None: assert r["nU"] == right and sum(b for _, b in r["scatter"]) == right
        if nK is not None: assert r["nK"] == nK and len(r["elims"]) == nK
    return f


def pin_event(tier2, tier3=None, nK_at_move=None):
    def f(rows, ev, p):
        r = _long_row(rows)
        e = ev[r["i"]]
        assert e[1] == tier2 and (tier3 is None or e[2] == tier3), e
        if nK_at_move is not None:
            a = R._attempt(r, R.clip_p(p, len(rows)), R.CAP2_SMALL if p <= 32 else R.CAP2_LARGE, R.G_CAPU, R.G_CAPK, alt_capL=R.G_CAPL)
            assert a[0] == "move" and nK_at_move(a[2][3]) and a[1] >= 1, a
    return f


def pin_all(*fs):
    def f(rows, ev, p):
        for g in fs:
            g(rows, ev, p)
    return f


def pin_forget(m):
    def f(rows, ev, p):
        r = _long_row(rows)
        assert [el["nd"] for el in r["elims"][:3]] == [0, 0, m] and (m < R.FREE_LIST) == (m <= 62)
        assert len(r["elims"]) == 8 and r["tops"][3][0] == 5           # (five entries behind: the movers / what the rewrite keeps)
    return f


def pin_shape(ul, cntL):
    def f(rows, ev, p):
        r = _long_row(rows)
        el = r["elims"][0]
        assert el["k"] == 0 and el["ul"] == ul and sum(c[2] for c in el["chunks"]) == cntL, el
        want = ("skip" if cntL <= 1 else "scalar4" if cntL <= 4 else "scalar8" if cntL <= 8 else "scalar16") if ul <= 16 else "search"
        assert el["chunks"][0][3] == want and len(el["chunks"]) == (ul + 63) // 64, el
        assert all(c[3] == "search" for c in el["chunks"][1:])
        hitsL = sum(1 for t in range(1, cntL) if t % 2 == 0)
        assert sum(c[0] for c in el["chunks"]) == cntL - 1 - hitsL                  # misses left of the diagonal ...
        assert sum(c[1] for c in el["chunks"]) == (ul - cntL) // 2                  # ... and right of it; the rest are hits
        assert all(e2["ul"] == 1 and e2["chunks"][0][2:] == (1, "skip") for e2 in r["elims"][1:])
    return f


def pin_sel(which, **kw):
    def f(rows, ev, p):
        s = _long_row(rows)[which]
        for k, v in kw.items():
            assert s[k] == v, (which, k, s)
    return f


def pin_hash(moves, walks_mask=None, alen=None):
    def f(rows, ev, p):
        r = _long_row(rows)
        hm = R.hash_moves(r, R.clip_p(p, len(rows)))
        assert (len(hm) == 1 and hm[0] < len(r["elims"])) if moves else hm == [], hm      # (a move with eliminations still to come)
        if alen is not None: assert r["alen"] == alen
        if walks_mask is not None: assert R.walks(r["ucols"], walks_mask) > 0
    return f


def pin_reuse(rows, ev, p):
    assert p == 32 and sorted(ev) == list(range(REUSE_PIVOTS, REUSE_PIVOTS + REUSE_ROWS)) and all(e == ["uslots", "ok", None] for e in ev.values())
    assert all(rows[k]["nU"] == 31 == rows[k]["selU"]["nsel"] for k in range(REUSE_PIVOTS))
    for j in range(REUSE_ROWS):
        r, n0 = rows[REUSE_PIVOTS + j], reuse_len(j)
        assert r["alen"] == REUSE_PIVOTS + 1 + n0 > R.HASH_SMALL // 4 and R.hash_moves(r, p) == []       # on the whole table from the start
        assert [el["k"] for el in r["elims"]] == list(range(REUSE_PIVOTS)) and all(el["ul"] == 32 for el in r["elims"])
        misses = [sum(c[1] for c in el["chunks"]) for el in r["elims"]]
        # (every elimination hits, and the first three miss too; pivot 3 misses only where the block has ended before its middle columns)
        assert all(0 < m < 31 for m in misses[:3]) and 0 <= misses[3] < 31 and r["nU"] == n0 + sum(misses)
        assert r["ucols"][n0:].min() >= REUSE_X + n0 and sum(c[0] for el in r["elims"] for c in el["chunks"]) == 0
        assert np.all(np.diff(r["ucols"][:n0]) == 1) and r["selU"]["long"] and r["selU"]["nsel"] == 31


def pin_collide(rows, ev, p):
    S = colliding()
    r = rows[5]
    assert len(set(R.wp_hash(c, R.HASH_SMALL - 1) for c in S)) == 1 and list(r["ucols"][-4:]) == S[:3] + [S[3]] and r["nU"] == 134
    assert r["elims"][0]["chunks"] == [(0, 1, 1, "skip")] and R.walks(r["ucols"], R.HASH_SMALL - 1) >= 3 and R.hash_moves(r, p) == []


def pin_none(rows, ev, p):
    pass


def _eq(v):
    return lambda t: v


def _is(got, want):
    assert got == want, (got, want)


CASES = collections.OrderedDict()


def _add(name, build, p, tau, route, pin=pin_none):
    assert name not in CASES
    CASES[name] = Case(build, p, tau, route, pin)


# tier 1, the pool (capL = 128 for p <= 32, 256 beyond)
_add("pool128", lambda: arrow(128, 3), 10, 0.0, OK, pin_counts(left=128))
_add("pool129", lambda: arrow(129, 3), 10, 0.0, (1, 1, 0, 0, 0, 0, False), pin_all(pin_counts(left=129), pin_event("ok")))
_add("pool128_p32", lambda: arrow(128, 3), 32, 0.0, OK, pin_counts(left=128))
_add("pool129_p32", lambda: arrow(129, 3), 32, 0.0, (1, 1, 0, 0, 0, 0, False), pin_counts(left=129))
_add("pool128_p33", lambda: arrow(128, 3), 33, 0.0, OK, pin_counts(left=128))
_add("pool129_p33", lambda: arrow(129, 3), 33, 0.0, OK, pin_counts(left=129))
_add("pool256_p33", lambda: arrow(256, 3), 33, 0.0, OK, pin_counts(left=256))
_add("pool257_p33", lambda: arrow(257, 3), 33, 0.0, (1, 1, 0, 0, 0, 0, False), pin_counts(left=257))
# tier 1, the U slots
_add("uslots128", lambda: arrow(3, 128), 10, 0.0, OK, pin_counts(right=128))
_add("uslots129", lambda: arrow(3, 129), 10, 0.0, (1, 0, 1, 0, 0, 0, False), pin_all(pin_counts(right=129), pin_event("ok")))
_add("uslots256_p33", lambda: arrow(3, 256), 33, 0.0, OK, pin_counts(right=256))
_add("uslots257_p33", lambda: arrow(3, 257), 33, 0.0, (1, 0, 1, 0, 0, 0, False), pin_counts(right=257))
# tier 1, the kept list (`nK > capL` at the row's end)
_add("chain128", lambda: chain(128), 10, 0.0, OK, pin_all(pin_counts(nK=128), pin_sel("selL", cnt=128, tie=True, sorted=True)))
_add("chain129", lambda: chain(129), 10, 0.0, (1, 0, 0, 1, 0, 0, False), pin_all(pin_counts(nK=129), pin_event("ok")))
# tier 2, the pool (512 entries) and its move
_add("left502", lambda: arrow(502, 3), 10, 0.0, (1, 1, 0, 0, 0, 0, False), pin_all(pin_counts(left=502), pin_event("ok")))
_add("left503", lambda: arrow(503, 3), 10, 0.0, (1, 1, 0, 0, 1, 0, False), pin_all(pin_counts(left=503), pin_event("move", "ok")))
_add("left513", lambda: arrow(513, 3), 10, 0.0, (1, 1, 0, 0, 1, 0, False), pin_all(pin_counts(left=513), pin_event("restart:pool", "ok")))
_add("midrow", midrow, 10, 0.0, (1, 1, 0, 0, 1, 0, False), pin_event("move", "ok", nK_at_move=lambda nK: nK == 2))
# tier 2, the move at the row's end (`nK > 512`)
_add("chain512", lambda: chain(512), 10, 0.0, (1, 0, 0, 1, 0, 0, False), pin_all(pin_counts(nK=512), pin_event("ok")))
_add("chain513", lambda: chain(513), 10, 0.0, (1, 0, 0, 1, 1, 0, False), pin_all(pin_counts(nK=513), pin_event("endmove", "ok")))
# the 64 K class and the natural fall-back to the largest one
_add("uarrow65534", lambda: arrow(0, 65534, n=65600), 4, 0.0, (1, 0, 1, 0, 0, 0, False),
     pin_all(pin_counts(right=65534), pin_event("ok")))
_add("uarrow65535", lambda: arrow(0, 65535, n=65600), 4, 0.0, (1, 0, 1, 0, 1, 3, True),
     pin_all(pin_counts(right=65535), pin_event("restart:uslots", "uslots")))
_add("larrow32768", lambda: arrow(32768, 3, lvals=tiny_left, n=32800), 10, 1e-3, (1, 1, 0, 0, 1, 0, False),
     pin_all(pin_counts(left=32768, nK=4), pin_event("restart:pool", "ok")))
_add("larrow32769", lambda: arrow(32769, 3, lvals=tiny_left, n=32800), 10, 1e-3, (1, 1, 0, 0, 1, 3, True),
     pin_all(pin_counts(left=32769, nK=4), pin_event("restart:pool", "pool")))
_add("chain32768", lambda: chain(32768, True), 10, 0.0, (1, 0, 0, 1, 1, 0, False),
     pin_all(pin_counts(nK=32768), pin_event("endmove", "ok"), pin_sel("selL", cnt=32768, tie=False, long=True)))
_add("chain32769", lambda: chain(32769, True), 10, 0.0, (1, 0, 0, 1, 1, 3, True),
     pin_all(pin_counts(nK=32769), pin_event("restart:kept", "kept"), pin_sel("selL", tie=False)))
# budgets
BIG_AT_ONCE = (None, None, None, None, None, None, True)
_add("band_p256", band, 256, 0.0, OK)
_add("band_p257", band, 257, 0.0, BIG_AT_ONCE)
_add("band_p0", band, 0, 0.0, OK, lambda rows, ev, p: [pin_sel("selU", nkeep=0, nsel=0)(rows, ev, p), pin_sel("selL", nkeep=0, nsel=0)(rows, ev, p)])
_add("band_p1", band, 1, 0.0, OK, pin_sel("selU", nkeep=0, nsel=0))
_add("band_p1000", band, 1000, 0.0, BIG_AT_ONCE)
# (n = 200: clipped to 200 the budget stays below the selection queue; unclipped it would go to the largest class at once)
_add("band200_p1000", lambda: band(200), 1000, 0.0, OK, pin_sel("selU", nkeep=199))
# the list of freed places (`nd < 63`)
for _m in (61, 62, 63, 64):
    _add("forget%d" % _m, lambda m=_m: forget(m), 10, 0.1, OK, pin_forget(_m))
# the shapes of the update with a U row
for _ul, _c in SHAPES:
    _add("shape_ul%d_c%d" % (_ul, _c), lambda a=_ul, b=_c: shape(a, b), max(_ul, 4), 0.0, OK, pin_shape(_ul, _c))
# wp_select
_add("uarrow1023", lambda: arrow(0, 1023), 10, 0.0, (1, 0, 1, 0, 0, 0, False),
     pin_all(pin_sel("selU", cnt=1023, long=False), pin_hash(False, alen=1024)))
_add("uarrow1024", lambda: arrow(0, 1024), 10, 0.0, (1, 0, 1, 0, 0, 0, False),
     pin_all(pin_sel("selU", cnt=1024, long=False, ncand=1024, nsel=9), pin_hash(False, alen=1025)))
_add("uarrow1025", lambda: arrow(0, 1025), 10, 0.0, (1, 0, 1, 0, 0, 0, False), pin_sel("selU", cnt=1025, long=True, ncand=1025, nsel=9))
_add("tie16", lambda: arrow(2, 16, rvals=_eq(1.5)), 5, 0.0, OK, pin_sel("selU", ncand=16, tie=True, sorted=False, nsel=4))
_add("tie17", lambda: arrow(2, 17, rvals=_eq(1.5)), 5, 0.0, OK, pin_sel("selU", ncand=17, tie=True, sorted=True, nsel=4))
_add("nsel64", lambda: arrow(2, 100), 65, 0.0, OK, pin_sel("selU", nkeep=64, nsel=64, ncand=100))
_add("nsel65", lambda: arrow(2, 100), 66, 0.0, OK, pin_sel("selU", nkeep=65, nsel=65, ncand=100))
_add("allkept", lambda: arrow(2, 20), 30, 0.0, OK, pin_sel("selU", ncand=20, nkeep=29, nsel=20, tie=False))
_add("chain1025", lambda: chain(1025), 10, 0.0, (1, 0, 0, 1, 1, 0, False),
     pin_all(pin_event("endmove", "ok"), pin_sel("selL", cnt=1025, long=True, tie=True, sorted=True, nsel=9)))
# the U-slot hash of a row in a global table
_add("hashmove2048", lambda: hashmove(7), 256, 0.0, (1, 0, 1, 0, 0, 0, False),
     pin_all(pin_hash(False), lambda rows, ev, p: _is(max(t[1] for t in rows[10]["tops"]) + p, 2048)))
_add("hashmove2049", lambda: hashmove(8), 256, 0.0, (1, 0, 1, 0, 0, 0, False), pin_hash(True))
_add("collide", collide, 10, 0.0, (1, 0, 1, 0, 0, 0, False), pin_collide)
# a wave that takes several rows that use its global table
_add("reuse", reuse, 32, 0.0, (REUSE_ROWS, 0, REUSE_ROWS, 0, 0, 0, False), pin_reuse)

NAMES = list(CASES)
# the cases of the child processes (each switch is read once per process)
TIER_CASES = ["pool129", "uslots129", "chain129", "left502", "left503", "left513", "midrow", "chain512", "chain513", "chain1025",
              "hashmove2048", "hashmove2049"]
CAP256_CASES = ["pool128", "pool129", "uslots128", "uslots129", "chain128", "chain129", "left502", "left513"]
REUSE_CASES = ["reuse", "hashmove2049", "midrow", "chain513"]


@functools.lru_cache(maxsize=None)
def model(name):
    """(L, U, rows) of a case's row view from ilut_ref.ilut, computed once and left unchanged"""
    from oracle import oracle as O
    A = matrix(name)
    c = CASES[name]
    return R.ilut(A.indptr, A.indices, A.data, c.p, c.tau, O.orc().sort_slots_by_abs_desc)


def matrix(name):
    A = sp.csr_matrix(CASES[name].build())
    A.sort_indices()
    return A
