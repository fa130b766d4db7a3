"""The cases of tests/test_gpu_sweep_kernels.py: every one is built for ONE edge of the CSR sweep kernels (sptrsv.hip, sptrsv_lm.hip) and is
the smallest size that reaches it.  tests/test_sweep_ref.py asserts, on the CPU, the figures that put each case at its edge.

A case is a lower triangular PATTERN (rows ascending, the diagonal last) with perturbed values, and a way to make an object of it:
  "ilut"    ILUTPreconditioner(fill_in = n, threshold = 0): a triangular matrix has no fill, L keeps the pattern and U is the diagonal
            (orientation "upper": the transposed matrix, U keeps the pattern).  Such an object has neither static records nor a factor
            order, so its routes follow from sweep_ref's rules alone.
  "ilu0"    ILU0Preconditioner of the same matrix: the short-row cases (every object with n >= 1024 is one: more than 4 n entries sweep in
            level order there).
  "ichol0", "icholt"   of the symmetric matrix P + P^T with a dominant diagonal: the factor has P's pattern.
With apply and apply_trans, "lower" and "upper", CSR and CSC input, and the two LL^T classes the cases reach all three sweep kinds:
  FWD_LAST_ASC     slot 0 of lower / slot 2 of upper (ilut, ilu0), slot 0 of ichol0, slot 3 of icholt
  BWD_FIRST_ASC    slot 1 of upper (ilut, ilu0), slot 0 of icholt
  BWD_FIRST_DESC   slot 3 of lower (ilut, ilu0), slot 3 of ichol0
RECORDED: where sweep_ref answers "level-major or CSR kernel" (short rows: whether the records accept a factor depends on skews the model
does not restate) the table carries what an MI355X did, observed once; every such entry is marked.  Everything else is predicted."""
import functools

import numpy as np
import scipy.sparse as sp

LANE = 256          # lanes of a workgroup


def _lower(cols_of_row, n, seed):
    """lower triangular CSR from {row: iterable of columns < row}; the diagonal last, off-diagonal values small enough that no solve grows"""
    rng = np.random.default_rng(seed)
    ptr = np.zeros(n + 1, dtype=np.int32)
    cols, vals = [], []
    percol = np.zeros(n, dtype=np.int64)
    rows = [np.array(sorted(set(int(c) for c in cols_of_row(r))), dtype=np.int32) for r in range(n)]
    for c in rows:
        percol[c] += 1
    for r, c in enumerate(rows):
        assert c.shape[0] == 0 or (0 <= c[0] and c[-1] < r), r
        k = c.shape[0]
        scale = 1.0 / np.maximum(np.maximum(percol[c], k), 1)            # (row sums and column sums of |off-diagonal| stay below 0.75)
        cols.append(c); cols.append(np.array([r], dtype=np.int32))
        vals.append(-(0.25 + 0.5 * rng.random(k)) * scale); vals.append(np.array([1.0 + rng.random()]))
        ptr[r + 1] = ptr[r] + k + 1
    return sp.csr_matrix((np.concatenate(vals), np.concatenate(cols), ptr), shape=(n, n))


def _spread(r, k):
    """k distinct columns < r, spread over [0, r) (none of them r - 1 unless k == r)"""
    k = min(k, r)
    if k == 0:
        return []
    if k == r:
        return range(r)
    return sorted(set(int(x) for x in np.linspace(0, r - 2, k).round()))          # (k <= r - 1 places among r - 1: a step of at least 1)


# ---- row lengths: the rule between k_sptrsv_lc and k_sptrsv_desc ------------------------------------------------------------------------
def rows_of(lengths):
    """row r has lengths[r] entries (fewer where r is smaller), no (r, r - 1) link where it can be avoided: one row per lane"""
    n = len(lengths)
    return _lower(lambda r: _spread(r, lengths[r] - 1), n, 100 + n)


def dense(n):
    return _lower(lambda r: range(r), n, 200 + n)


def few(n, nnz):
    """n rows and exactly nnz entries: the diagonal, and nnz - n entries that fill the rows from the last one up"""
    take, left = [0] * n, nnz - n
    for q in range(n - 1, -1, -1):
        take[q] = min(q, left)
        left -= take[q]
    return _lower(lambda r: _spread(r, take[r]), n, 300 + nnz)


# ---- chains: one lane owns many rows (entry and right-hand-side rings) ---------------------------------------------------------------------
def band(n, width, chain, lengths=None):
    """rows r - 1 ... r - width and the diagonal, the (r, r - 1) link missing at every multiple of `chain`: lanes of `chain` rows.
    lengths: the entries of row r (cycling), 1 = the diagonal alone (which also ends a chain)"""
    def cols(r):
        w = width if lengths is None else lengths[r % len(lengths)] - 1
        c = [r - d for d in range(1, w + 1) if r - d >= 0]
        if r % chain == 0 and r - 1 in c:
            c.remove(r - 1)
        return c
    return _lower(cols, n, 400 + n + width)


# ---- hand-off between lanes of one workgroup ---------------------------------------------------------------------------------------------
def handoff(d, lanes=8, rows=64, extra=3, long_row=0):
    """`lanes` chains of `rows` rows; row k of lane j reads its own previous row and rows k - d, k - d - 1 ... k - d - extra of lane j - 1:
    the producer has run at least d rows past the row that is read.  long_row: one row of that many entries (the kernel rule)"""
    lanes, rows = (lanes, rows) if 4 * d <= rows else (4, 4 * d)          # (d = 40: longer lanes, fewer of them, so that n stays below 1 024)
    n = lanes * rows
    def cols(r):
        j, k = divmod(r, rows)
        c = [r - 1] if k else []
        if j:
            c += [(j - 1) * rows + k - d - e for e in range(extra + 1) if k - d - e >= 0]
        if long_row and r == n - 1:
            c += _spread((lanes - 2) * rows, long_row - 1 - len(c))
        return c
    return _lower(cols, n, 500 + d + long_row)


# ---- imports: unknowns of other workgroups -------------------------------------------------------------------------------------------------
def imports(producers, per_row, n=768, long_row=0):
    """one row per lane (no (r, r - 1) link), three workgroups; every row reads rows r - 2 ... r - 6 of its own workgroup, and the rows of the
    LAST workgroup read `per_row` unknowns each out of the first `producers` rows: that workgroup imports from `producers` foreign lanes"""
    def cols(r):
        base = (r // LANE) * LANE
        c = [r - d for d in range(2, 7) if r - d >= base]
        if r >= n - LANE:
            c += [((r - (n - LANE)) * per_row + t) % producers for t in range(per_row)]
        if long_row and r == n - 1:
            c += range(300, 300 + long_row - 1 - len(c))
        return c
    return _lower(cols, n, 600 + producers + per_row + long_row)


def ghost_chain(rows=20, lanes=300):
    """lanes of `rows` rows; the lanes of the second workgroup read, row for row, the lane 256 places before them: every ghost lane of that
    workgroup stands for a producer that owns a chain of `rows` rows"""
    n = rows * lanes
    def cols(r):
        j, k = divmod(r, rows)
        return ([r - 1] if k else []) + ([r - LANE * rows] if j >= LANE else [])
    return _lower(cols, n, 700)


# ---- placement -------------------------------------------------------------------------------------------------------------------------------
def one_per_lane(n):
    """n lanes of one row (rows r - 2 ... r - 6): nb = n blocks"""
    return _lower(lambda r: [r - d for d in range(2, 7) if r - d >= 0], n, 800 + n)


def lines(nx, ny, far=(2, 3, 4)):
    """lines of nx rows (chains of nx <= 4 rows: one row per lane), every row reads its place in the line before and in the lines `far`
    before: block offsets 1 and nx ... -- the shape the tiling takes"""
    n = nx * ny
    def cols(r):
        return ([r - 1] if r % nx else []) + [r - nx * f for f in (1,) + tuple(far) if r - nx * f >= 0]
    return _lower(cols, n, 900 + n + len(far))


# ---- n >= 1024 ---------------------------------------------------------------------------------------------------------------------------------
def chain(n):
    return _lower(lambda r: [r - 1] if r else [], n, 1000 + n)


def arrow(n=2048, long_row=1000, mid_row=17):
    def cols(r):
        if r == n - 1:
            return _spread(r, long_row - 1)
        if r == n // 2:
            return _spread(r, mid_row - 1)
        return []
    return _lower(cols, n, 1100)


C16 = tuple(range(1, 17))

# name -> (builder, class, orientation, input format, what the case is for)
_T = {}


def _case(name, build, cls="ilut", orient="lower", fmt="csr", aim=""):
    _T[name] = (build, cls, orient, fmt, aim)


def _both(name, build, aim, cls="ilut"):
    _case(name, build, cls, "lower", "csr", aim)
    _case(name + "-up", build, cls, "upper", "csr", aim)


_both("rows16", lambda: rows_of([16] * 48), "longest row 16: k_sptrsv_lc; first rows short, last row long")
_both("rows17", lambda: rows_of([16] * 47 + [17]), "longest row 17: k_sptrsv_desc")
_both("rows1_16", lambda: rows_of([1, 16] * 24 + [1]), "rows of 1 mixed with rows of 16; the last row short")
_case("rows16-csc", lambda: rows_of([16] * 48), "ilut", "lower", "csc", "CSC input: the plans of apply and apply_trans change places")
_case("dense7", lambda: dense(7), aim="n = 7, nnz = 28: below n >= 8, k_sptrsv_desc")
_both("dense8", lambda: dense(8), "n = 8, nnz = 36: k_sptrsv_lc")
_case("nnz15", lambda: few(8, 15), aim="nnz = 15: k_sptrsv_desc")
_case("nnz16", lambda: few(8, 16), aim="nnz = 16: k_sptrsv_lc (or the records)")
_case("one", lambda: dense(1), aim="n = 1")
_both("tail3", lambda: rows_of([16] * 40 + [3]), "the last row starts 3 entries before nnz: window loads clamped at the array's end")
_both("tail6", lambda: rows_of([16] * 40 + [6]), "the last row starts 6 entries before nnz")
for _k in (15, 16, 17, 33, 100):
    _both("chain%d" % _k, functools.partial(band, _k, 5, 1 << 20), "one lane owns a chain of %d rows of 6 entries" % _k)
_both("cycle16", lambda: band(16 * 32 + 2, 0, 16, C16), "row lengths cycling 1 .. 16 in lanes of 16 rows; the last lane owns 2 rows")
for _d in (1, 3, 4, 5, 8, 9, 40):
    _both("handoff%d" % _d, functools.partial(handoff, _d), "k_sptrsv_lc (ring of 4): a lane reads its neighbour %d rows back" % _d)
    _both("handoff%d-desc" % _d, functools.partial(handoff, _d, long_row=17), "k_sptrsv_desc (ring of 8): the same with one row of 17")
for _p, _e in ((1, 1), (63, 4), (64, 5), (65, 9), (512, 9)):
    _both("imports%d" % _p, functools.partial(imports, _p, _e), "a workgroup imports from %d foreign lanes, %d foreign unknowns per row" % (_p, _e))
_both("imports65-desc", lambda: imports(65, 9, long_row=17), "k_sptrsv_desc: 67 foreign lanes (the 65 and two of the middle workgroup, read by the row of 17), 11 foreign unknowns in that row")
for _n in (511, 512, 513):
    _case("lanes%d" % _n, functools.partial(one_per_lane, _n), aim="nb = %d blocks (tiling_wanted at 512)" % _n)
_both("lines4x192", lambda: lines(4, 192), "768 lanes in patches: the tiled placement (and ILUPP_TILE_TZ)")
_case("chol0-band", lambda: band(300, 6, 30), "ichol0", aim="IChol(0): FWD_LAST_ASC and BWD_FIRST_DESC")
_case("cholt-band", lambda: band(300, 6, 30), "icholt", aim="ICholT: FWD_LAST_ASC and BWD_FIRST_ASC")
# (not in NAMES: made only in a process that runs with ILUPP_REFERENCE_NANS=1)
DEGENERATE = "cholt-indefinite"
# short rows (at n >= 1024 nothing else reaches these kernels: more than 4 n entries sweep in level order), hence level-major candidates: recorded
_both("lines4x192-short", lambda: lines(4, 192, ()), "short rows of a tiled object: the level-major records", cls="ilu0")
_both("ghost20", ghost_chain, "a ghost producer that owns a chain of 20 rows", cls="ilu0")
_both("chain32768", lambda: chain(32768), "positions up to 0x7fff in the descriptors", cls="ilu0")
_both("chain32769", lambda: chain(32769), "B = 32 769: not compact, the generic kernel; the other factor (B = 1) by the joint rule too", cls="ilu0")
_both("arrow", arrow, "n >= 1024, one row of 17 and one of 1 000: k_sptrsv_desc", cls="ilu0")

NAMES = tuple(_T)
_T[DEGENERATE] = (lambda: band(300, 6, 30), "icholt", "lower", "csr", "a negative pivot: columns of NaN are stored empty, the object is degenerate, "
                  "k_sptrsv_rows (route 5) FWD_LAST_ASC and BWD_FIRST_ASC")


@functools.lru_cache(maxsize=None)
def pattern(name):
    """the lower triangular matrix of the case (shared: nobody writes into it)"""
    P = _T[name][0]()
    for a in (P.data, P.indices, P.indptr):
        a.setflags(write=False)
    return P


def info(name):
    """(class, orientation, input format, aim)"""
    return _T[name][1:]


@functools.lru_cache(maxsize=None)
def matrix(name):
    """the matrix the object is made of, in its input format"""
    P = pattern(name)
    _, cls, orient, fmt, _ = _T[name]
    if cls in ("ichol0", "icholt"):
        S = (P + P.T).tocsr()                             # (the diagonal doubled: dominant)
        S.sort_indices()
        if name == DEGENERATE:
            S[150, 150] = -1.0
        M = S
    else:
        M = P if orient == "lower" else P.T.tocsr()
        M.sort_indices()
    M = M.tocsr() if fmt == "csr" else M.tocsc()
    M = type(M)((M.data.astype(np.float64), M.indices.astype(np.int32), M.indptr.astype(np.int32)), shape=M.shape)
    for a in (M.data, M.indices, M.indptr):
        a.setflags(write=False)
    return M


# ---- RECORDED on an MI355X --------------------------------------------------------------------------------------------------------------------
# (slot: route) where sweep_ref answers LM_OR_CSR: 2 = the level-major records took the sweep, 6 = they declined and the descriptor kernel the
# model names ran.  Observed once on the device, not predicted.  Under ILUPP_NO_PACKED=1 none of this applies: every such slot is predicted.
RECORDED = {}
for _n in ("rows16", "rows17", "rows1_16", "tail3", "tail6", "chain16", "chain17", "chain33", "chain100", "cycle16", "handoff1",
           "handoff1-desc", "handoff3", "handoff3-desc", "handoff4", "handoff4-desc", "handoff5", "handoff5-desc", "handoff8",
           "handoff8-desc", "handoff9", "handoff9-desc", "handoff40", "handoff40-desc", "imports1", "imports63", "imports64", "imports65",
           "imports512", "imports65-desc", "lanes511", "lanes512", "lanes513", "lines4x192"):
    RECORDED[_n] = {1: 2, 2: 2}
for _n in ("rows16-up", "rows17-up", "rows1_16-up", "rows16-csc", "tail3-up", "tail6-up", "chain16-up", "chain17-up", "chain33-up",
           "chain100-up", "cycle16-up", "handoff1-up", "handoff1-desc-up", "handoff3-up", "handoff3-desc-up", "handoff4-up",
           "handoff4-desc-up", "handoff5-up", "handoff5-desc-up", "handoff8-up", "handoff8-desc-up", "handoff9-up", "handoff9-desc-up",
           "handoff40-up", "handoff40-desc-up", "imports1-up", "imports63-up", "imports64-up", "imports65-up", "imports512-up",
           "imports65-desc-up", "lines4x192-up"):
    RECORDED[_n] = {0: 2, 3: 2}
for _n in ("dense7",):
    RECORDED[_n] = {0: 6, 3: 6}
for _n in ("nnz16",):
    RECORDED[_n] = {0: 6, 3: 2}
for _n in ("lines4x192-short", "chain32768"):
    RECORDED[_n] = {0: 6, 1: 2, 2: 2, 3: 6}
for _n in ("lines4x192-short-up", "chain32768-up"):
    RECORDED[_n] = {0: 2, 1: 6, 2: 6, 3: 2}
for _n in ("ghost20", "ghost20-up"):
    RECORDED[_n] = {0: 2, 1: 2, 2: 2, 3: 2}
for _n in ("arrow",):
    RECORDED[_n] = {0: 6, 1: 2, 2: 2, 3: 2}
for _n in ("arrow-up",):
    RECORDED[_n] = {0: 2, 1: 2, 2: 6, 3: 2}
# ... and the ILU(0) / IChol(0) objects that the static analysis (st.hip, which the model does not restate) takes whole, route 1 on every slot: none
RECORDED_STATIC = ()


def factors(O, name):
    """the factors by the oracle O (oracle.orc() or oracle.ref()), as P.factors() returns them: (class for sweep_ref, L, U or None)"""
    M = matrix(name)
    cls = info(name)[0]
    A = (M.data, M.indices, M.indptr, sp.isspmatrix_csr(M))
    n = M.shape[0]
    mat = lambda F: (sp.csr_matrix if F[3] else sp.csc_matrix)((F[0], F[1], F[2]), shape=(n, n))
    if cls == "ilut":
        L, U = O.ilut(A, n, 0.0)
        return "lu", mat(L), mat(U)
    if cls == "ilu0":
        L, U = O.ilu0(A)
        return "lu", mat(L), mat(U)
    if cls == "ichol0":
        return "ichol0", mat(O.ichol0(A)), None
    return "icholt", mat(O.icholt(A, 0, 0.0)), None


def make(ilupp, name):
    """the object of the case"""
    M = matrix(name)
    cls = info(name)[0]
    if cls == "ilut":
        return ilupp.ILUTPreconditioner(M, fill_in=M.shape[0], threshold=0.0)
    if cls == "ilu0":
        return ilupp.ILU0Preconditioner(M)
    if cls == "ichol0":
        return ilupp.IChol0Preconditioner(M)
    return ilupp.ICholTPreconditioner(M, add_fill_in=0, threshold=0.0)
