"""A plain CPU model of the CSR sweep family (ilupp_amd/csrc/sptrsv.hip, sptrsv_lm.hip) and of the rules that send a sweep there (api.hip:
sweep(), sweep_tables(), long_rows(); symbolic.hip: k_row_cuts, make_schedule, k_block_starts; schedule.hip: build_slot_tables,
tiling_decide; sptrsv.hip: sptrsv(); sptrsv_lm.hip: lm_prepare).  numpy / scipy only; it never calls the library.

The arithmetic (sptrsv.hip's header): three gather sweeps over row-major storage,
  FWD_LAST_ASC     rows ascending,  x_r = (b_r - sum over the entries before the last, first to last) / the last entry
  BWD_FIRST_ASC    rows descending, x_r = (b_r - sum over the entries behind the first, first to last) / the first entry
  BWD_FIRST_DESC   the same with the entries behind the first taken last to first
Entries in STORED order, product and subtraction two separate operations, the diagonal found by POSITION and always divided by; a NaN
result is stored as the one canonical NaN.  `sweep` does it in float64, `sweep_long` in np.longdouble.

The routing is RESTATED from the code's own statements (not imported), so that a threshold that drifts in the code fails a test.  What the
model cannot decide -- whether the level-major records accept a short-row factor depends on skews -- it answers with LM_OR_CSR."""
import numpy as np
import scipy.sparse as sp

FWD_LAST_ASC, BWD_FIRST_ASC, BWD_FIRST_DESC = 0, 1, 2
KIND_NAMES = ("FWD_LAST_ASC", "BWD_FIRST_ASC", "BWD_FIRST_DESC")
# ilupp_hip_debug_level_order's info[6] and info[7]
ROUTE_STATIC, ROUTE_LEVEL_MAJOR, ROUTE_LEVEL_ORDER, ROUTE_ROWS, ROUTE_ROWS_DEGENERATE, ROUTE_DESCRIPTORS, ROUTE_GENERIC = 1, 2, 3, 4, 5, 6, 7
KERNEL_LC, KERNEL_DESC = 1, 2
LM_OR_CSR = "level-major or CSR kernel"          # the model's answer where lm_prepare's necessary conditions hold
LEVEL_OR_ROWS = "level order or natural order"   # ... and where long_rows() holds (level_ref.py models that family)

# constants of the code, restated
THREADS, GHOSTS = 256, 64
GHOST_BASE = (1 << 17) - GHOSTS
MAX_LANES = 1 << 24
EW, EQ = 32, 8                                   # k_sptrsv_lc's entry ring and its refill quantum
CANON_NAN = np.uint64(0x7FF8000000000000).view(np.float64)


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------------
def _arrays(T):
    """(indptr, indices, data) of T as stored (CSR; nothing sorted, nothing summed)"""
    assert sp.isspmatrix_csr(T)
    return T.indptr, T.indices, T.data


def _sweep(T, b, kind, ftype, canon):
    ptr, idx, val = _arrays(T)
    n = T.shape[0]
    val = val.astype(ftype)
    x = np.array(b, dtype=ftype)
    out = np.empty(n, dtype=ftype)
    with np.errstate(all="ignore"):
        for r in (range(n) if kind == FWD_LAST_ASC else range(n - 1, -1, -1)):
            lo, hi = int(ptr[r]), int(ptr[r + 1])
            if hi == lo:                           # a row without entries (factors with NaN columns): divided by NaN
                out[r] = canon
                continue
            if kind == FWD_LAST_ASC:
                js, d = range(lo, hi - 1), hi - 1
            elif kind == BWD_FIRST_ASC:
                js, d = range(lo + 1, hi), lo
            else:
                js, d = range(hi - 1, lo, -1), lo
            acc = x[r]
            for j in js:
                prod = val[j] * out[idx[j]]
                acc = acc - prod
            acc = acc / val[d]
            out[r] = canon if acc != acc else acc
    return out


def sweep(T, b, kind):
    """the float64 sweep: what the device must give bit for bit (NaNs: by position)"""
    return _sweep(T, b, kind, np.float64, CANON_NAN)


def sweep_long(T, b, kind):
    """the same sweep in np.longdouble"""
    return _sweep(T, b, kind, np.longdouble, np.longdouble("nan"))


def backward_error_ok(T, x, b, kind):
    """the backward-error bound of substitution, row by row and in longdouble: |b - T x|_r <= gamma_k (|T| |x|)_r with k the entries of
    row r, u = 2^-53, gamma_k = k u / (1 - k u).  Returns (ok, worst ratio residual / bound)"""
    ptr, idx, val = _arrays(T)
    ld = np.longdouble
    u = ld(2.0) ** -53
    xl, worst = np.asarray(x).astype(ld), ld(0)
    for r in range(T.shape[0]):
        lo, hi = int(ptr[r]), int(ptr[r + 1])
        v, xc = val[lo:hi].astype(ld), xl[idx[lo:hi]]
        k = hi - lo
        res = abs(ld(b[r]) - np.sum(v * xc))
        bound = (k * u / (1 - k * u)) * np.sum(np.abs(v) * np.abs(xc))
        if res > bound:
            worst = max(worst, res / bound if bound > 0 else ld(np.inf))
        elif bound > 0:
            worst = max(worst, res / bound)
    return bool(worst <= 1), float(worst)


# ---- which triangle a slot holds and how it is swept ----------------------------------------------------------------------------------
# slots: 0 = Lc, 1 = Uc, 2 = UcT, 3 = LcT (sweep_parts in api.hip).  The two sweeps of an apply (apply_plan) as (slot, the matrix the sweep
# walks in CSR as stored, kind), the forward sweep first.  L and U are what P.factors() returns.
def _stored_rows(M):
    """the row-major matrix whose arrays are M's own (a CSC matrix read as CSR is its transpose)"""
    return M if sp.isspmatrix_csr(M) else sp.csr_matrix((M.data, M.indices, M.indptr), shape=M.shape)


def _transposed_storage(S):
    """transpose_storage: a counting transposition, the entries of a new row in the order of the old rows"""
    S = S.tocsr()
    n = S.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(S.indptr))
    order = np.argsort(S.indices, kind="stable")
    ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(S.indices, minlength=n), out=ptr[1:])
    return sp.csr_matrix((S.data[order], rows[order], ptr), shape=S.shape)


def stored(cls, L, U):
    """{slot: CSR matrix as the object stores it} for "lu" (ILU(0), ILUT), "ichol0", "icholt" """
    Lc = _stored_rows(L)
    if cls == "lu":
        Uc = _stored_rows(U)
        if not sp.isspmatrix_csr(L):                      # CSC input: the object holds the factors of the row-major view A^T = U^T L^T
            Lc, Uc = Uc, Lc
        return {0: Lc, 1: Uc, 2: _transposed_storage(Uc), 3: _transposed_storage(Lc)}
    return {0: Lc, 3: _transposed_storage(Lc)}


def plan(cls, csr_input, transpose):
    """[(slot, kind), (slot, kind)] of apply (transpose False) or apply_trans"""
    if cls == "lu":
        if transpose == (not csr_input):
            return [(0, FWD_LAST_ASC), (1, BWD_FIRST_ASC)]
        return [(2, FWD_LAST_ASC), (3, BWD_FIRST_DESC)]
    if cls == "ichol0":
        return [(0, FWD_LAST_ASC), (3, BWD_FIRST_DESC)]
    if cls == "icholt":
        return [(3, FWD_LAST_ASC), (0, BWD_FIRST_ASC)]
    raise ValueError(cls)


def apply(cls, L, U, csr_input, transpose, b):
    """what apply / apply_trans must leave in place of b, by the float64 model"""
    S = stored(cls, L, U)
    x = np.array(b, dtype=np.float64)
    for slot, kind in plan(cls, csr_input, transpose):
        x = sweep(S[slot], x, kind)
    return x


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------
def cuts(T, fwd):
    """k_row_cuts: forward, a block may start at row r iff r == 0 or row r has no entry in column r - 1; backward, a cut lies between r - 1
    and r iff r == 0 or row r - 1 has no entry in column r"""
    ptr, idx, _ = _arrays(T)
    n = T.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    cut = np.ones(n, dtype=np.uint8)
    if fwd:
        cut[rows[idx == rows - 1]] = 0
        cut[0] = 1
    else:
        linked = rows[idx == rows + 1]
        cut[linked + 1] = 0
    return cut


def schedule(T, fwd):
    """make_schedule + k_block_starts: {"ncuts", "B", "nb", "start"}"""
    n = T.shape[0]
    cut = cuts(T, fwd)
    ncuts = int(cut.sum())
    B = (n + MAX_LANES - 1) // MAX_LANES
    chain = (n + ncuts - 1) // ncuts if ncuts > 0 else n
    B = max(B, chain)
    if chain <= 4:
        B = 1
    B = max(B, 1)
    nb = (n + B - 1) // B
    start = np.empty(nb + 1, dtype=np.int64)
    start[0], start[nb] = 0, n
    for b in range(1, nb):
        lo, hi = b * B, min((b + 1) * B, n)
        at = np.flatnonzero(cut[lo:hi])
        start[b] = lo + at[0] if at.shape[0] else hi
    return {"ncuts": ncuts, "B": B, "nb": nb, "start": start, "fwd": fwd}


def block_of(c, sch):
    return np.searchsorted(sch["start"], c, side="right") - 1      # (blocks may be empty: the last block that starts at or before c)


def _patch_shape(s2, nbz, max_wgs):
    ty, tz = 16, 16
    while ty > s2 and ty > 1:
        ty >>= 1; tz <<= 1
    while tz > nbz and tz > 1:
        tz >>= 1; ty <<= 1
    if ty > s2 or ty * tz != THREADS or ((s2 + ty - 1) // ty) * ((nbz + tz - 1) // tz) > max_wgs:
        return None
    return ty, tz


def tiling(T, sch, no_tiles=False, tile_tz=None):
    """tiling_wanted + k_sample_block_offsets + tiling_decide: None, or (s2, ty, tz) of the patches"""
    nb = sch["nb"]
    if no_tiles or nb < 2 * THREADS:
        return None
    ptr, idx, _ = _arrays(T)
    fwd, start = sch["fwd"], sch["start"]
    nsamp = min(nb, 2048)
    stride = max(nb // nsamp, 1)
    cnt, has1, nonempty = {}, 0, 0
    for s in range(nsamp):
        b = (s * stride) % nb
        if start[b + 1] <= start[b]:
            continue
        r = int(start[b] + (start[b + 1] - start[b]) // 2)
        offs = []
        for q in range(ptr[r], ptr[r + 1]):
            c = int(idx[q])
            if len(offs) == 8:
                break
            if (c >= r) if fwd else (c <= r):
                continue
            d = int(b - block_of(c, sch)) if fwd else int(block_of(c, sch) - b)
            if d > 0:
                offs.append(d)
        for d in offs:
            if d == 1:
                has1 += 1
            elif d in cnt or len(cnt) < 64:
                cnt[d] = cnt.get(d, 0) + 1
        nonempty += bool(offs)
    s2, best = 0, 0
    for d, c in cnt.items():                       # (insertion order, the first of equal counts: as the code's vector)
        if c > best:
            best, s2 = c, d
    max_wgs = MAX_LANES // THREADS
    if nonempty == 0 or s2 < 4 or best * 2 < nonempty or has1 * 2 < nonempty:
        return None
    nbz = (nb + s2 - 1) // s2
    shape = _patch_shape(s2, nbz, max_wgs)
    if shape is None:
        return None
    ty, tz = shape
    if tile_tz is not None and 1 <= tile_tz <= tz:
        tz = tile_tz
    if ((s2 + ty - 1) // ty) * ((nbz + tz - 1) // tz) > max_wgs:
        return None
    return s2, ty, tz


def slots(sch, til):
    """build_slot_tables + k_slot_tables: (nslots, slot of every block)"""
    nb = sch["nb"]
    order = np.arange(nb) if sch["fwd"] else nb - 1 - np.arange(nb)      # block in sweep order -> block
    if til is None:
        nslots = ((nb + THREADS - 1) // THREADS) * THREADS
        blk2slot = np.empty(nb, dtype=np.int64)
        blk2slot[order] = np.arange(nb)
        return nslots, blk2slot
    s2, ty, tz = til
    NY = (s2 + ty - 1) // ty
    nbz = (nb + s2 - 1) // s2
    NZ = (nbz + tz - 1) // tz
    nslots = NY * NZ * THREADS
    blk2slot = np.full(nb, -1, dtype=np.int64)
    for s in range(nslots):
        Tn, lane = divmod(s, THREADS)
        by, bz = (Tn % NY) * ty + lane % ty, (Tn // NY) * tz + lane // ty
        if by >= s2 or lane // ty >= tz:
            continue
        bs = bz * s2 + by
        if bs < nb:
            blk2slot[order[bs]] = s
    assert (blk2slot >= 0).all()
    return nslots, blk2slot


def is_compact(sch, nslots):
    """schedule_is_compact: the 15-bit position field and the slot field below the ghost lanes"""
    return sch["B"] <= 32768 and nslots <= GHOST_BASE


def figures(T, fwd, no_tiles=False, tile_tz=None):
    """the schedule of one sweep and the figures that put a case at an edge of the kernels: longest row, rows per lane (the longest block),
    per workgroup the distinct foreign producer lanes it reads from (the largest count), per row the unknowns of other workgroups (the
    largest count), and the distances, in rows of the producer, at which a row reads another lane of its own workgroup"""
    ptr, idx, _ = _arrays(T)
    n = T.shape[0]
    sch = schedule(T, fwd)
    til = tiling(T, sch, no_tiles, tile_tz)
    nslots, blk2slot = slots(sch, til)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    off = idx != rows
    rblk, cblk = block_of(rows[off], sch), block_of(idx[off].astype(np.int64), sch)
    rs, cs = blk2slot[rblk], blk2slot[cblk]
    foreign = (rs >> 8) != (cs >> 8)
    per_wg = {}
    for w, s in zip((rs >> 8)[foreign], cs[foreign]):
        per_wg.setdefault(int(w), set()).add(int(s))
    ext = np.bincount(rows[off][foreign], minlength=n) if n else np.zeros(0, dtype=np.int64)
    start = sch["start"]
    return {"sch": sch, "tiling": til, "nslots": nslots, "compact": is_compact(sch, nslots), "longest": int(np.diff(ptr).max()) if n else 0,
            "shortest": int(np.diff(ptr).min()) if n else 0, "rows_per_lane": int(np.diff(start).max()),
            "foreign_producers": max((len(v) for v in per_wg.values()), default=0), "externals_per_row": int(ext.max()) if n else 0,
            "lane_distances": _lane_distances(rows[off], idx[off].astype(np.int64), rblk, cblk, rs, cs, sch),
            "workgroups": nslots // THREADS, "own_previous_row": bool(np.any((rblk == cblk) & (np.abs(rows[off] - idx[off]) == 1)))}


def _lane_distances(r, c, rblk, cblk, rs, cs, sch):
    """where a row reads ANOTHER lane of its own workgroup: (place of the reading row in its lane) - (place of the row read in its lane),
    places in processing order; the set of these differences"""
    start, fwd = sch["start"], sch["fwd"]
    sel = ((rs >> 8) == (cs >> 8)) & (rblk != cblk)
    place = lambda x, b: (x - start[b]) if fwd else (start[b + 1] - 1 - x)
    return sorted(set((place(r[sel], rblk[sel]) - place(c[sel], cblk[sel])).tolist()))


# ---- the route and the kernel of every slot --------------------------------------------------------------------------------------------
def lc_rule(longest, nnz, n):
    """sptrsv(): rows fit the entry ring with room for the refill quantum; tiny systems keep the simple kernel"""
    return 0 < longest <= EW - 2 * EQ and nnz >= 16 and n >= 8


def lm_necessary(nnz, n, nslots):
    """lm_prepare's cheap conditions (descriptors and the import table exist wherever this is asked)"""
    return nnz <= 4 * n and nslots >= THREADS and nnz >= 16


def long_rows(nnz, n):
    return nnz > 4 * n and n >= 1024


def expected_routes(cls, L, U, degenerate=False, no_packed=False, no_tiles=False, tile_tz=None):
    """{slot: (route, kernel)} as ilupp_hip_debug_level_order must report them after an apply and an apply_trans of an object that has
    neither static records nor a factor order (an ILUT object; an ILU(0) or IChol(0) object where st.hip declines, which the model does
    not restate: such cases are recorded).  route is a number, or LM_OR_CSR / LEVEL_OR_ROWS with the CSR answer as second element"""
    S = stored(cls, L, U)
    if cls == "lu":
        pairs = [((0, True), (1, False), True), ((2, True), (3, False), True)]
    elif cls == "ichol0":
        pairs = [((0, True), None, True), ((3, False), None, True)]
    else:
        pairs = [((0, False), None, True), ((3, True), None, True)]
    out = {}
    for a, b, joint in pairs:
        group = [g for g in (a, b) if g]
        fig = {slot: figures(S[slot], fwd, no_tiles, tile_tz) for slot, fwd in group}
        maxlen = max(f["longest"] for f in fig.values())              # (*max_len of sweep_tables: the longer of the two)
        allc = all(f["compact"] for f in fig.values())
        for slot, fwd in group:
            T, f = S[slot], fig[slot]
            n, nnz = T.shape[0], T.nnz
            desc = allc if joint else f["compact"]
            csr = (ROUTE_DESCRIPTORS, KERNEL_LC if lc_rule(maxlen, nnz, n) else KERNEL_DESC) if desc else (ROUTE_GENERIC, 0)
            if degenerate:
                out[slot] = (ROUTE_ROWS_DEGENERATE, 0)
            elif desc and not no_packed and lm_necessary(nnz, n, f["nslots"]):
                out[slot] = (LM_OR_CSR, csr)
            elif long_rows(nnz, n):
                out[slot] = (LEVEL_OR_ROWS, csr)
            else:
                out[slot] = csr
    return out
