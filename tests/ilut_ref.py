"""CPU model of the wave-parallel ILUT kernel (ilupp_amd/csrc/ilut_wp.hip): plain Python + numpy, float64, no FMA anywhere.

ilut() restates ILUT_heap the way wp_row computes it (the header comment of ilut_wp.hip is the specification): a row is three
insertion-ordered pieces -- POOL (left of the diagonal, not eliminated yet), KEPT (the multipliers) and U SLOTS --, the stage-1 threshold
is tau * sqrt(z) over the scattered left part summed in insertion order, the row eliminates its smallest LIVE column (neither zero nor
below that threshold; what lies left of it is forgotten), the dropping step takes candidates by strict > and the p - 1 largest by
(magnitude desc, position asc) unless the cut falls between equal magnitudes among more than 16 candidates (then `sort`, the oracle's
sort_slots_by_abs_desc, decides), exact zeros are stripped from the result (compact_slab).  It returns L and U of the row view as CSR
triples (data, indices, indptr) and, per row, the DEMANDS the kernel's capacity tests see, in the kernel's own bookkeeping:

  rec["scatter"]   [(mL, mU)] per 64-chunk of A's row (ilut_wp.hip:473-488: `nL + popc(mL) > capL`, `nU + popc(mU) > capU`)
  rec["tops"]      [(nL, nU, nK, seq)] at the top of every pass of the elimination loop, the last pass -- the one that finds nothing
                   live and leaves -- included: what the hash move (:542) and the pool move (:553) read.  nL counts the pool as the
                   kernel does: the entries that went with the previous elimination (column <= klast) are still in it, and so is the
                   entry about to be popped
  rec["elims"]     per elimination: k, nd (the entries with column <= klast that the pass found: `nd < 63` chooses between filling
                   holes from the tail and rewriting the pool, :589), ul (length of U's row k, the diagonal included), and per
                   64-chunk of that row (mL, mU, cntL, shape): the misses appended left and right (:751), the columns left of this
                   row's diagonal (the popped one included, :710) and the update's shape (:704-726): "skip" (cntL <= 1), "scalar4",
                   "scalar8", "scalar16", or "search" (more than 16 entries, or a later chunk)
  rec["nK"], rec["nU"], rec["alen"]   the pieces at the row's end, the entries of A's row (:427: above 1 024 the hash starts on the whole table)
  rec["selU"], rec["selL"]   the two selections (:776, :815): cnt, nkeep, ncand, tie (what the extra round found), sorted (the cut was
                   decided by the sort), nsel, long (cnt > 1 024: the path that reads the piece again per round, :257)
  rec["ucols"]     the columns of the U slots in slot order (for the hash: walks())
A row that is its diagonal alone has no record (rows[i] is None): it fits every class.

route() walks the kernel's three attempts per row over those demands with the capacities restated from the source, and returns what the
two ILUPP_DEBUG lines of ilut_rows_wp (:1211, :1037) must show."""
import heapq
import math

import numpy as np

# ---- capacities, restated from ilut_wp.hip ---------------------------------------------------------------------------------------------
CAP1_SMALL, CAP1_LARGE = 128, 256            # k_ilut_rows_wp<128, 512> for p <= 32, <256, 1024> else (:1051, :1100-1105): capL = capU (:841)
CAP2_SMALL, CAP2_LARGE = 7168 // 14, 14336 // 14      # tier 2: the whole LDS block is the pool, ILUT_RAW / 14 (:846-850) = 512 / 1 024
G_CAPU, G_CAPL, G_CAPK = 65534, 1 << 15, 1 << 15      # the wave's global arrays (:57); capK is gw.capK in every tier (:870-871)
SEL_QUEUE = 256                               # kWpSel (:56): budgets with p - 1 >= 256 go to the largest class at once (:1050)
SMALL_P = 32                                  # :1051
ID_MAX = 65535                                # WpIdMax<unsigned short> (:99): sequence numbers of the left-part insertions
HASH_SMALL = 4096                             # kWpHashSmall (:62); a row of A above HASH_SMALL / 4 entries starts on the whole table (:427)
HASH_G = 1 << 17                              # kWpHashG (:58)
FREE_LIST = 63                                # `nd < 63` (:589)
SEL_REGS = 1024                               # 64 * kRC (:173)


def clip_p(p, n):
    """ilut.hip:77-79"""
    return max(1, min(int(p), n))


def wp_hash(c, mask):
    """:345"""
    return (((int(c) * 0x9E3779B1) & 0xffffffff) >> 12) & mask


def walks(ucols, mask):
    """the number of U slots whose insertion walked past an occupied cell of a table of mask + 1 cells (open addressing, :351-374)"""
    taken, n = set(), 0
    for c in ucols:
        h = wp_hash(c, mask)
        if h in taken:
            n += 1
            while h in taken:
                h = (h + 1) & mask
        taken.add(h)
    return n


def _ordered_sum_sq(v):
    """z = z + v * v over v in order (np.add.accumulate adds strictly left to right)"""
    v = np.asarray(v, dtype=np.float64)
    return float(np.add.accumulate(v * v)[-1]) if v.shape[0] else 0.0


def select(cols, vals, nkeep, tau, sort):
    """threshold_and_drop over one piece in insertion order (wp_select, :161-342): (kept positions by increasing column, record)"""
    cols = np.asarray(cols, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    cnt = cols.shape[0]
    rec = {"cnt": cnt, "nkeep": nkeep, "ncand": 0, "tie": False, "sorted": False, "nsel": 0, "long": cnt > SEL_REGS}
    if nkeep <= 0:                                                      # :169
        return np.zeros(0, dtype=np.int64), rec
    thr = math.sqrt(_ordered_sum_sq(vals)) * tau
    mag = np.abs(vals)
    cand = np.nonzero(mag > thr)[0]
    rec["ncand"] = int(cand.shape[0])
    if cand.shape[0] <= nkeep:
        sel = cand
    else:
        order = cand[np.lexsort((cand, -mag[cand]))]                    # magnitude desc, position asc
        sel = order[:nkeep]
        rec["tie"] = bool(mag[order[nkeep]] == mag[order[nkeep - 1]])   # the extra round (:222-237)
        if rec["tie"] and cand.shape[0] > 16:                           # :239
            lst = np.asarray(sort(vals[cand]), dtype=np.int64)
            sel = cand[lst[:nkeep]]
            rec["sorted"] = True
    rec["nsel"] = int(sel.shape[0])
    return sel[np.argsort(cols[sel], kind="stable")], rec


def _shape(base, cnt, cntL):
    if cnt <= 16 and base == 0:                                         # :704
        return "skip" if cntL <= 1 else ("scalar4" if cntL <= 4 else ("scalar8" if cntL <= 8 else "scalar16"))      # :711-714
    return "search"


def ilut(indptr, indices, data, fill_in, tau, sort):
    """ILUT(p, tau) of the row view (indptr, indices, data): (L, U, rows) -- L, U CSR triples (data, indices, indptr), rows the records"""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    data = np.asarray(data, dtype=np.float64)
    n = indptr.shape[0] - 1
    p = clip_p(fill_in, n)
    Uc, Uv = [None] * n, [None] * n            # U's rows as the kernel publishes them: the diagonal, then the kept entries by column
    Lc, Lv = [None] * n, [None] * n
    rows = [None] * n
    for i in range(n):
        a0, a1 = int(indptr[i]), int(indptr[i + 1])
        cols, vals = indices[a0:a1], data[a0:a1]
        if a1 - a0 == 1 and cols[0] == i:
            Uc[i], Uv[i] = (i,), (float(vals[0]),)
            Lc[i], Lv[i] = (), ()
            continue
        left, right = cols < i, cols > i
        rec = {"i": i, "alen": a1 - a0, "scatter": [], "tops": [], "elims": []}
        starts = np.arange(0, max(a1 - a0, 1), 64)
        if a1 > a0:
            rec["scatter"] = list(zip(np.add.reduceat(left.astype(np.int64), starts).tolist(),
                                      np.add.reduceat(right.astype(np.int64), starts).tolist()))
        dg = vals[cols == i]
        wdiag = float(dg[0]) if dg.shape[0] else 0.0
        lcols, lvals = cols[left].tolist(), vals[left].tolist()
        pool = {c: [v, s] for s, (c, v) in enumerate(zip(lcols, lvals))}        # column -> [value, seq]
        heap = list(lcols)
        heapq.heapify(heap)
        seq = nL = len(lcols)
        thr1 = tau * math.sqrt(_ordered_sum_sq(lvals))                          # :490-494
        ucol, uval = cols[right].tolist(), vals[right].tolist()
        uslot = {c: q for q, c in enumerate(ucol)} if nL else None               # (rows without a left part never look a column up)
        kept = []                                                                # (column, multiplier, seq)
        pending = 0                 # entries forgotten left of the last eliminated column: in the pool until the next pass (nd)
        while True:
            rec["tops"].append((nL, len(ucol), len(kept), seq))
            forgotten, k = 0, -1
            while heap:
                c = heapq.heappop(heap)
                v = pool[c][0]
                if v != 0.0 and not (abs(v) < thr1):                             # live (:532)
                    k = c
                    break
                forgotten += 1
                del pool[c]
            if k < 0:
                break
            wkv, sk = pool.pop(k)
            nd = pending
            nL -= nd + 1                                                         # :590, :612 / :632
            pending = forgotten
            ukc, ukv = Uc[k], Uv[k]
            ul = len(ukc)
            m = wkv / ukv[0]                                                     # :670
            kept.append((k, m, sk))
            el = {"k": k, "nd": nd, "ul": ul, "chunks": []}
            for base in range(0, ul, 64):
                cnt = min(64, ul - base)
                mL = mU = cntL = 0
                for j in range(base, base + cnt):
                    c = ukc[j]
                    if c < i:
                        cntL += 1
                    if j == 0:
                        continue
                    pr = m * ukv[j]
                    if c < i:
                        e = pool.get(c)
                        if e is not None:
                            e[0] = e[0] - pr
                        else:
                            pool[c] = [0.0 - pr, seq + mL]                       # :754-755
                            heapq.heappush(heap, c)
                            mL += 1
                    elif c == i:
                        wdiag = wdiag - pr                                       # :742
                    else:
                        q = uslot.get(c)
                        if q is not None:
                            uval[q] = uval[q] - pr
                        else:
                            uslot[c] = len(ucol)
                            ucol.append(c); uval.append(0.0 - pr)                # :758
                            mU += 1
                nL += mL; seq += mL
                el["chunks"].append((mL, mU, cntL, _shape(base, cnt, cntL)))
            rec["elims"].append(el)
        rec["nK"], rec["nU"] = len(kept), len(ucol)
        rec["ucols"] = np.asarray(ucol, dtype=np.int64)
        su, rec["selU"] = select(ucol, uval, p - 1, tau, sort)
        Uc[i] = (i,) + tuple(int(ucol[q]) for q in su)
        Uv[i] = (wdiag,) + tuple(uval[q] for q in su)
        kept.sort(key=lambda t: t[2])                                            # back in insertion order (:794-811)
        kc, kv = [t[0] for t in kept], [t[1] for t in kept]
        sl, rec["selL"] = select(kc, kv, p - 1, tau, sort)
        Lc[i], Lv[i] = tuple(kc[q] for q in sl), tuple(kv[q] for q in sl)
        rows[i] = rec

    def csr(C, V, suffix_one):
        ptr = np.zeros(n + 1, dtype=np.int32)
        cc, vv = [], []
        for r in range(n):
            c, v = list(C[r]), list(V[r])
            if suffix_one:
                c.append(r); v.append(1.0)
            keep = [t for t in range(len(c)) if v[t] != 0.0]                     # compact_slab strips exact zeros
            cc.extend(c[t] for t in keep); vv.extend(v[t] for t in keep)
            ptr[r + 1] = len(cc)
        return np.asarray(vv, dtype=np.float64), np.asarray(cc, dtype=np.int32), ptr

    return csr(Lc, Lv, True), csr(Uc, Uv, False), rows


# ---- the route ----------------------------------------------------------------------------------------------------------------------------
def _attempt(rec, p, capL, capU, capK, alt_capL=None, resume=None):
    """one call of wp_row over a row's demands: ("ok",), ("pool" | "uslots" | "kept" | "seq",) = it returned 1 for that cause, or
    ("move", e, state) / ("endmove", state) = it returned 3 at the top of pass e / after the last pass.  resume: the state a move left"""
    if resume is None:
        nL = nU = nK = seq = 0
        for mL, mU in rec["scatter"]:
            if seq + mL > ID_MAX: return ("seq",)                                # :480
            if nL + mL > capL: return ("pool",)                                  # :481
            if nU + mU > capU: return ("uslots",)
            nL += mL; seq += mL; nU += mU
        e0 = 0
    else:
        e0, nL, nU, nK, seq = resume
    elims = rec["elims"]
    for e in range(e0, len(elims) + 1):
        assert resume is not None or (nL, nU, nK, seq) == rec["tops"][e], (rec["i"], e)      # (the two bookkeepings agree)
        if alt_capL is not None and nL + p > capL and nL + p <= alt_capL:        # :553
            return ("move", e, (e, nL, nU, nK, seq))
        if e == len(elims):
            break
        el = elims[e]
        nL -= el["nd"] + 1
        if nK >= capK: return ("kept",)                                          # :671
        nK += 1
        for mL, mU, _, _ in el["chunks"]:
            if seq + mL > ID_MAX: return ("seq",)                                # :750
            if nL + mL > capL: return ("pool",)                                  # :751
            if nU + mU > capU: return ("uslots",)
            nL += mL; seq += mL; nU += mU
    if alt_capL is not None and nK > capL and nK <= alt_capL:                    # :769 (nL = 0: only the pool's home changes)
        return ("endmove", (len(elims), 0, nU, nK, seq))
    if nK > capL: return ("kept",)                                               # :770
    return ("ok",)


def route(rows, n, p, cap256=False, tier2=True, force_big=False):
    """what a factorisation shows under ILUPP_DEBUG: (outgrew, pool, uslots, kept, left_tier2, status, big) -- ctrl[3], [4], [5], [6],
    [24], [1] of the first line and whether the line of the largest class is printed -- and, per row that left tier 1, what became of it:
    events[i] = [tier-1 cause, tier-2 outcome ("ok", "move", "endmove", "restart:<cause>" or None without tier 2), tier-3 outcome or None].
    Budgets with p - 1 >= 256 (and ILUPP_ILUT_BIG) go to the largest class at once: the first line is absent, its figures are None.
    cap256: ILUPP_ILUT_CAP=256; tier2=False: ILUPP_ILUT_NO_TIER2=1"""
    p = clip_p(p, n)
    if p - 1 >= SEL_QUEUE or force_big:                                          # :1050
        return (None, None, None, None, None, None, True), {}
    large = p > SMALL_P or cap256                                                # :1100
    cap1, cap2 = (CAP1_LARGE, CAP2_LARGE) if large else (CAP1_SMALL, CAP2_SMALL)
    count = {"pool": 0, "uslots": 0, "kept": 0, "seq": 0}
    outgrew = left2 = status = 0
    events = {}
    failed = []
    for rec in rows:
        if rec is None:
            continue
        r = _attempt(rec, p, cap1, cap1, G_CAPK)                                 # :886 (lw)
        if r[0] == "ok":
            continue
        outgrew += 1; count[r[0]] += 1                                           # ctrl[3] (:890, :896) and ctrl[4..6] (tier 1 only: `!G`)
        ev = [r[0], None, None]
        resume = None
        if tier2:
            r = _attempt(rec, p, cap2, G_CAPU, G_CAPK, alt_capL=G_CAPL)          # :891 (hw, the global arrays as the pool's second home)
            if r[0] in ("move", "endmove"):
                left2 += 1; resume = r[-1]; ev[1] = r[0]                         # :894
            elif r[0] != "ok":
                left2 += 1; ev[1] = "restart:" + r[0]
            else:
                ev[1] = "ok"
        if not tier2 or ev[1] != "ok":
            r = _attempt(rec, p, G_CAPL, G_CAPU, G_CAPK, resume=resume)          # :901 (g)
            ev[2] = r[0]
            if r[0] != "ok":
                status = 3; failed.append(rec["i"])                              # :908
        events[rec["i"]] = ev
    # (a row that gives up is published as its diagonal alone: the counters of the first line are those of the model only while no later
    # row eliminates that column -- every case with status 3 is built that way)
    for rec in rows:
        if rec is not None and failed:
            assert not any(el["k"] in failed for el in rec["elims"]), "a later row depends on a row that gave up"
    assert count["seq"] == 0, "sequence numbers past 16 bits: no counter of the debug line shows this cause"
    return (outgrew, count["pool"], count["uslots"], count["kept"], left2, status, status == 3), events


def hash_moves(rec, p):
    """the passes at whose top the U-slot hash of a row in a wave's global table moves from its first 4 096 cells to the whole table
    (:542: `nU + p > 2048`); [] for a row that starts on the whole table (:427) or never moves"""
    if rec["alen"] > HASH_SMALL // 4:
        return []
    for e, (_, nU, _, _) in enumerate(rec["tops"]):
        if nU + p > HASH_SMALL // 2:
            return [e]
    return []
