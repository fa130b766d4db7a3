"""A stepwise CPU model of the multilevel factorisation WITH pivoting (ilupp_amd/csrc/pilucdp.hip: k_pilucdp_lds, k_pilucdp and the host loop
of pilucdp_level), in plain Python floats.  It restates partialILUCDP (ILUCDP.hpp:268-1404, as oracle/ilupp_oracle.c::partial_ilucdp states it)
in the reference's order of operations -- the insertion order of both working vectors, norms summed in slot order, the FIRST of equal
maxima, the reference's partial sort (select_largest of tests/pivot_ref.py) exactly as written, the bucket bookkeeping of the rows by their
number of entries in L, the level's end -- so that every level's L, U, D, permutations and zero-pivot count have the oracle's bits
(tests/test_dp_ref.py).  The Schur complement is the next level's matrix; the model runs every level (orc_ml_create's loop, without
preprocessing), and the oracle, which does not hand the Schur complement out, is compared through the level that is computed from it.

It keeps one record per step with what the two kernels branch on:
  checks      [(point, znnz, wnnz)] after each of the eight places where k_pilucdp_lds may abandon a step (POINTS: the source lines of
              the DPL_STOP(4) they stand for are LINES), `stop`: the first point at which a vector holds more than 2 048 entries, or None
  takeU/takeL (candidates, limit, kept) of the two lv_take / dp_take calls
  moves       per 64-entry chunk of bucket moves its class: "once" (no two moves touch one position: applied by all lanes), "clash",
              "far" (a count reaches kPnL = 1024: boundaries beyond the LDS cache)
  group       the length of the group of rows that is sorted behind the step (0: none begins there)
  pU pL pS    the store positions at the step's start; eliminate: whether the step starts while eliminating
  dupz/dupw   the 64-entry passes of the row / column load in which a doubly stored index was met
  zprobe/wprobe  (longest probe, wrapped past slot 4 095) of the vector's index set in the 4 096-slot table, entered in insertion order

launches(levels, ...) predicts from the records what the host loop goes through: (n, flavour, status, step) per launch, for a given store
size (ILUPP_DP_STORE = k: stores of n + 2 + k entries that grow by as much) and start flavour, with the stop rule p + row_max > cap and
the hand-over rule entries > 2 048.

REFUSED parameter families (NotImplementedError): any preprocessing, inverse-based dropping, weighted dropping (both forms).  Everything
else of orc_ml_params is followed: all local dropping rules and combinations, bounded fill, every FINAL_ROW_CRIT, the windows of
PERMUTE_ROWS and TOTAL_PIV, small pivots, the threshold shifts.

Variants for the tests that show that a case discriminates (never the default): see level()."""
import collections
import math

import numpy as np

from pivot_ref import select_largest, _Vec

LV_CAP, LV_HASH, PNL, PASS = 2048, 4096, 1024, 64
POINTS = ("row_load", "l_sub", "diag_touch", "perm_touch", "col_load_own", "u_sub_own", "col_load_other", "u_sub_other")
LINES = dict(zip(POINTS, (785, 788, 802, 809, 822, 824, 827, 829)))
DROP_STANDARD, DROP_STANDARD2, DROP_ERR_PROP, DROP_ERR_PROP2, DROP_PIVOT, DROP_INVERSE, DROP_WEIGHTED, DROP_WEIGHTED2 = 1, 2, 4, 8, 16, 32, 64, 128

Level = collections.namedtuple("Level", "n L U D perm_rows perm_cols inv_perm_rows inv_perm_cols zero_pivots Anew records to_the_end last max_fill nnz")


# ---- the table of k_pilucdp_lds ------------------------------------------------------------------------------------------------------------
def lv_hash(c):
    """lv_hash<LvLds>: Fibonacci hashing to 12 bits"""
    return ((c * 0x9E3779B1) & 0xFFFFFFFF) >> 20


def probe_stats(indices):
    """the indices entered one after the other by linear probing: (the longest probe in slots visited, whether a probe went from slot
    4 095 on to slot 0)"""
    table, longest, wrapped = set(), 0, False
    for c in indices:
        h, steps = lv_hash(c), 1
        while h in table:
            if h == LV_HASH - 1:
                wrapped = True
            h = (h + 1) & (LV_HASH - 1)
            steps += 1
        table.add(h)
        longest = max(longest, steps)
    return longest, wrapped


# ---- storage -------------------------------------------------------------------------------------------------------------------------------
def other_orientation(ptr, idx, val):
    """matrix_sparse::change_orientation: the same matrix in the other storage order, entries of a slice in the order they are met"""
    n = len(ptr) - 1
    cnt = [0] * (n + 1)
    for c in idx:
        cnt[c + 1] += 1
    for i in range(n):
        cnt[i + 1] += cnt[i]
    optr, fill = list(cnt), list(cnt[:n])
    oidx, oval = [0] * len(idx), [0.0] * len(idx)
    for r in range(n):
        for j in range(ptr[r], ptr[r + 1]):
            q = fill[idx[j]]
            oidx[q], oval[q] = r, val[j]
            fill[idx[j]] += 1
    return optr, oidx, oval


def _finish(n_slices, ptr, idx, val, renumber):
    """compress() (|x| > 0 stays), the indices renumbered, normal_order(): as arrays"""
    optr, oidx, oval = [0], [], []
    for r in range(n_slices):
        row = [(renumber(idx[j]), val[j]) for j in range(ptr[r], ptr[r + 1]) if abs(val[j]) > 0.0]
        row.sort(key=lambda t: t[0])
        oidx.extend(t[0] for t in row); oval.extend(t[1] for t in row)
        optr.append(len(oidx))
    return optr, oidx, oval


def _arrays(m):
    ptr, idx, val = m
    return (np.array(val, dtype=np.float64), np.array(idx, dtype=np.int32), np.array(ptr, dtype=np.int32))


def _fdiv(a, b):
    """a / b as the hardware divides: by zero gives an infinity or a NaN, no exception"""
    if b == 0.0:
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _inv(p):
    return _fdiv(1.0, p)


# ---- the dropping rules --------------------------------------------------------------------------------------------------------------------
def _combine(P, x, y):
    if P.combine_factor == 1:
        return x + y
    if P.combine_factor == 2:
        return x * y
    if P.combine_factor == 3:
        m = y if x < y else x
        return m if P.min_weight < m else P.min_weight
    return y if x < y else x


def _norm1(v):
    z = 0.0
    for x in v.data:
        z += abs(x)
    return z


def _norm2(v):
    z = 0.0
    for x in v.data:
        z += x * x
    return math.sqrt(z)


def _weight(P, own, other, dinv):
    w = P.neutral_element
    if P.drop_rules & DROP_STANDARD:
        norm = _norm2(own)
        if norm == 0.0:
            norm = 1e-16
        w = _combine(P, w, P.weight_standard_drop / norm)
    if P.drop_rules & DROP_STANDARD2:
        w = _combine(P, w, P.weight_standard_drop2)
    if P.drop_rules & DROP_ERR_PROP:
        w = _combine(P, w, P.weight_err_prop_drop * _norm1(other))
    if P.drop_rules & DROP_ERR_PROP2:
        w = _combine(P, w, _fdiv(P.weight_err_prop_drop2 * _norm1(other), abs(dinv)))
    if P.drop_rules & DROP_PIVOT:
        w = _combine(P, w, P.weight_pivot_drop * abs(dinv))
    if P.scale_weight_invdiag:
        w *= abs(dinv)
    return w


def _keep(key, lst, limit):
    """keep_largest_sorted: more candidates than limit => the limit largest by select_largest; then by index.  (candidates, limit, kept)"""
    cnt = len(lst)
    if cnt > limit:
        if limit > 0:
            select_largest(key, lst, 0, cnt - 1, limit)
        lst = lst[cnt - limit:]
    return sorted(lst), (cnt, limit, min(cnt, limit))


def _take_single(v, weight, limit, tau):
    key, lst = [], []
    for x, c in zip(v.data, v.pointer):
        prod = weight * abs(x)
        if prod >= tau:
            key.append(prod); lst.append(c)
    return _keep(key, lst, limit)


def _take_largest(v, limit, tau):
    norm = _norm2(v)
    key, lst = [], []
    for x, c in zip(v.data, v.pointer):
        if abs(x) > norm * tau:
            key.append(abs(x)); lst.append(c)
    return _keep(key, lst, limit)


def _chunk_class(rows, bpr, epr, iprow, prow, numb, pnum):
    """what k_pilucdp_lds decides for one chunk of at most 64 bucket moves from the state before the chunk"""
    inr = [bpr <= b0 <= epr for b0 in rows]
    cntb = [numb[iprow[b0]] + 1 if ok else 0 for b0, ok in zip(rows, inr)]
    if any(ok and c >= PNL for ok, c in zip(inr, cntb)):
        return "far"
    for i, b0 in enumerate(rows):
        if not inr[i]:
            continue
        rank = sum(1 for q in range(i) if inr[q] and cntb[q] == cntb[i])
        ra = prow[pnum[cntb[i]] - 1 - rank]
        if any(inr[q] and q != i and rows[q] == ra for q in range(len(rows))):
            return "clash"
    return "once"


def _moves_at_once(rows, bpr, epr, iprow, prow, numb, pnum):
    """the lanes' parallel form of a chunk's moves, whatever its class (a variant: right only for class "once")"""
    plan = []
    inr = [bpr <= b0 <= epr for b0 in rows]
    cntb = [numb[iprow[b0]] + 1 if ok else 0 for b0, ok in zip(rows, inr)]
    for i, b0 in enumerate(rows):
        if inr[i]:
            rank = sum(1 for q in range(i) if inr[q] and cntb[q] == cntb[i])
            b = iprow[b0]
            a = pnum[cntb[i]] - 1 - rank
            plan.append((b0, b, a, prow[a], cntb[i]))
    for b0, b, a, ra, c in plan:
        pnum[c] -= 1
        if a != b:
            iprow[ra] = b; iprow[b0] = a
            prow[a] = b0; prow[b] = ra
            numb[a] = c; numb[b] = c - 1
        else:
            numb[b] = c


# ---- one level -----------------------------------------------------------------------------------------------------------------------------
def level(rows, P, force_finish, threshold, bp, bpr, epr, forget_dead_at=None, stale_restart_at=None, moves_at_once=False, first_copy=False):
    """partialILUCDP on the rows (ptr, idx, val) of a level.  Variants: forget_dead_at = k: from step k on the subtractions know only the
    dead columns and rows marked from step k on (a hand-over that loses zrec / wrec slot -2); stale_restart_at = k: step k starts as
    after DPL_STOP's ctrl[6] = ctrl[7] = 0, ctrl[11] = -1 in the memory flavour (nothing of step k - 1 is cleared: its indices still
    answer with their slots and values); moves_at_once: every chunk of bucket moves in the lanes' parallel form; first_copy: the FIRST
    value of a doubly stored index stands."""
    ptr, idx, val = [int(x) for x in rows[0]], [int(x) for x in rows[1]], [float(x) for x in rows[2]]
    n = len(ptr) - 1
    cp, ci, cv = other_orientation(ptr, idx, val)
    nnzA = cp[n]
    max_fill = P.max_fill_in if P.max_fill_in > 0 else n
    max_fill = min(max(max_fill, 1), n)
    epr = min(max(epr, 0), n - 1)
    bpr = min(max(bpr, 0), n - 1)
    Dinv = [1.0] * n
    perm, prow, iperm, iprow = list(range(n)), list(range(n)), list(range(n)), list(range(n))
    nonpiv, unused = [True] * n, [True] * n
    zdead, wdead = set(), set()                     # what the subtractions take for dead (the kernels' slot -2)
    zstale, wstale = {}, {}
    startU, startL = [-1] * n, [-1] * n
    numb, pnum = [0] * (n + 1), [0] + [epr + 1] * (n + 1)
    Up, Ui, Uv, linkU, rowU = [0], [], [], [], []
    Lp, Li, Lv, linkL, colL = [0], [], [], [], []
    Sp, Si, Sv = [0], [], []
    eliminate, end_level_now = True, False
    last, nA, zero_pivots = n - 1, 0, 0
    piv_tol, pivot, pos_pivot = P.piv_tol, 0.0, -1
    records = []
    z, w = _Vec(), _Vec()

    def sub(v, stale, c, prod):
        if v.occ.get(c, -1) < 0 and c in stale:
            stale[c] -= prod
            return
        v.data[v.slot(c)] -= prod

    def load(v, stale, lo, hi, ai, av, alive, dups):
        for e in range(lo, hi):
            c = ai[e]
            if not alive[c]:
                continue
            stale.pop(c, None)
            if v.occ.get(c, -1) >= 0:
                dups.append((e - lo) // PASS)
                if first_copy:
                    continue
            v.data[v.slot(c)] = av[e]

    for k in range(n):
        rec = dict(step=k, eliminate=eliminate, pU=Up[k], pL=Lp[k], pS=Sp[-1], checks=[], stop=None, moves=[], group=0, dupz=[], dupw=[],
                   takeL=None, far=False)

        def check(point):
            rec["checks"].append((point, len(z.data), len(w.data)))
            if rec["stop"] is None and max(len(z.data), len(w.data)) > LV_CAP:
                rec["stop"] = point
        if P.begin_total_piv and k == bp:
            piv_tol = 1.0
        sel = prow[k]
        if stale_restart_at == k:
            zstale = {c: x for c, x in zip(z.pointer, z.data) if c not in zdead}
            wstale = {r: x for r, x in zip(w.pointer, w.data) if r not in wdead}
        if forget_dead_at == k:
            zdead, wdead = set(), set()
        unused[sel] = False
        wdead.add(sel)
        wstale.pop(sel, None)
        z, w = _Vec(), _Vec()
        load(z, zstale, ptr[sel], ptr[sel + 1], idx, val, nonpiv, rec["dupz"])
        check("row_load")
        h = startL[sel]
        while h != -1:
            c, lv = colL[h], Lv[h]
            h = linkL[h]
            f = _fdiv(lv, Dinv[c])
            for j in range(Up[c], Up[c + 1]):
                if Ui[j] not in zdead:
                    sub(z, zstale, Ui[j], f * Uv[j])
        check("l_sub")

        def touch(c, point):
            if z.occ.get(c, -1) < 0 and c in zstale:
                return zstale[c]
            if z.occ.get(c, -1) < 0:
                z.slot(c)
                check(point)
            return z.data[z.occ[c]]
        if eliminate:
            mx, val_larg_el, pos_pivot = 0.0, 0.0, -1
            for x, c in zip(z.data, z.pointer):
                if abs(x) > mx:
                    mx, val_larg_el, pos_pivot = abs(x), x, c
            if nonpiv[sel]:
                zs = touch(sel, "diag_touch")
                if abs(val_larg_el * piv_tol) > abs(zs) and pos_pivot >= 0 and P.piv_tol > 0:
                    pivot = val_larg_el
                else:
                    pos_pivot, pivot = sel, zs
            elif abs(val_larg_el) > 0.0 and pos_pivot >= 0:
                pivot = val_larg_el
            else:
                pos_pivot = perm[k]
                pivot = touch(pos_pivot, "perm_touch")
        if eliminate and not force_finish and float(k) > P.min_elim_factor * float(n) and P.small_pivot_terminates and abs(pivot) < P.min_pivot:
            eliminate, end_level_now = False, True
            threshold *= P.threshold_shift_schur
            last, nA = k - 1, n - k
            Sp, Si, Sv = [0], [], []
        rec["elim_step"] = eliminate
        if eliminate:
            Dinv[k] = _inv(pivot)
            z.data = [x * Dinv[k] for x in z.data]
            if z.occ.get(pos_pivot, -1) >= 0:
                z.data[z.occ[pos_pivot]] = 0.0
            else:
                z.data[z.slot(pos_pivot)] = 0.0
            zstale.pop(pos_pivot, None)
            p = iperm[pos_pivot]
            iperm[perm[k]], iperm[pos_pivot] = iperm[pos_pivot], iperm[perm[k]]
            perm[k], perm[p] = perm[p], perm[k]
            nonpiv[pos_pivot] = False
            zdead.add(pos_pivot)
            c = perm[k]
            own = c == sel
            load(w, wstale, cp[c], cp[c + 1], ci, cv, unused, rec["dupw"])
            check("col_load_own" if own else "col_load_other")
            h = startU[c]
            while h != -1:
                r, uv = rowU[h], Uv[h]
                h = linkU[h]
                f = _fdiv(uv, Dinv[r])
                for j in range(Lp[r], Lp[r + 1]):
                    if Li[j] not in wdead:
                        sub(w, wstale, Li[j], f * Lv[j])
            check("u_sub_own" if own else "u_sub_other")
            rec.update(pivot_col=pos_pivot, sel=sel)
        w.data = [x * Dinv[k] for x in w.data]
        rec.update(znnz=len(z.data), wnnz=len(w.data), zprobe=probe_stats(z.pointer), wprobe=probe_stats(w.pointer))
        if not eliminate:
            lU, rec["takeU"] = _take_largest(z, max_fill, threshold)
        else:
            lU, rec["takeU"] = _take_single(z, _weight(P, z, w, Dinv[k]), max_fill - 1, threshold)
        nU = len(lU)
        if eliminate:
            Uv.append(1.0); Ui.append(pos_pivot); linkU.append(-1); rowU.append(k)
            for j in range(nU):
                c = lU[nU - 1 - j]
                Uv.append(z.data[z.occ[c]]); Ui.append(c)
                linkU.append(startU[c]); startU[c] = len(Uv) - 1; rowU.append(k)
            Up.append(len(Uv))
            if pivot == 0.0:
                zero_pivots += 1
                Dinv[k] = 1.0
        else:
            Uv.append(1.0); Ui.append(perm[k]); linkU.append(-1); rowU.append(k)
            Dinv[k] = 1.0
            Up.append(len(Uv))
            for j in range(nU):
                c = lU[nU - 1 - j]
                Sv.append(z.data[z.occ[c]]); Si.append(c)
            Sp.append(len(Sv))
        if eliminate:
            lL, rec["takeL"] = _take_single(w, _weight(P, w, z, Dinv[k]), max_fill, threshold)
            Lv.append(1.0); Li.append(sel); linkL.append(-1); colL.append(k)
            for b in lL:
                Lv.append(w.data[w.occ[b]]); Li.append(b)
                linkL.append(startL[b]); startL[b] = len(Lv) - 1; colL.append(k)
            Lp.append(len(Lv))
            for base in range(0, len(lL), PASS):
                chunk = lL[base:base + PASS]
                rec["moves"].append(_chunk_class(chunk, bpr, epr, iprow, prow, numb, pnum))
                if moves_at_once:
                    _moves_at_once(chunk, bpr, epr, iprow, prow, numb, pnum)
                    continue
                for b0 in chunk:
                    if bpr <= b0 <= epr:
                        b = iprow[b0]
                        numb[b] += 1
                        pnum[numb[b]] -= 1
                        a = pnum[numb[b]]
                        iprow[prow[a]], iprow[prow[b]] = iprow[prow[b]], iprow[prow[a]]
                        prow[a], prow[b] = prow[b], prow[a]
                        numb[a], numb[b] = numb[b], numb[a]
            rec["far"] = "far" in rec["moves"]
            rec["pnum_seen"] = max([numb[iprow[b0]] for b0 in lL if bpr <= b0 <= epr], default=0)
            if pnum[numb[k] + 1] == k + 1:
                g0, g1 = k + 1, pnum[numb[k] + 2] - 1
                rec["group"] = max(0, g1 - g0 + 1)
                grp = sorted(prow[g0:g1 + 1])
                for q, r in enumerate(grp):
                    prow[g0 + q] = r; iprow[r] = g0 + q
        else:
            Lv.append(1.0); Li.append(sel); linkL.append(-1); colL.append(k)
            Lp.append(len(Lv))
        records.append(rec)
        if eliminate and not force_finish:
            if float(k) > P.min_elim_factor * float(n):
                dens, cnt, crit = float(nnzA), float(numb[k]), P.final_row_crit
                factor = {-1: P.move_level_factor, 0: 0.5, 1: None, 2: 2.0, 3: 4.0, 4: 6.0, 6: 1.5, 8: 3.0, 9: 1.2}
                if crit == 1:
                    end_level_now = end_level_now or cnt > dens / float(n)
                elif crit in factor:
                    end_level_now = end_level_now or cnt > (factor[crit] * dens) / float(n)
                elif crit == 5:
                    end_level_now = end_level_now or numb[k] > 10
                elif crit == 7:
                    end_level_now = end_level_now or _norm2(z) > P.row_u_max
            if end_level_now:
                eliminate = False
                threshold *= P.threshold_shift_schur
                last, nA = k, n - k - 1
                Sp, Si, Sv = [0], [], []
    L = _finish(n, Lp, Li, Lv, lambda r: iprow[r])
    U = _finish(n, Up, Ui, Uv, lambda c: iperm[c])
    if eliminate:
        Anew = ([0], [], [])
    else:
        Anew = _finish(nA, Sp, Si, Sv, lambda c: iperm[c] - last - 1)
    a32 = lambda p: np.array(p, dtype=np.int32)
    return Level(n, _arrays(L), _arrays(U), np.array(Dinv, dtype=np.float64), a32(prow), a32(perm), a32(iprow), a32(iperm), zero_pivots, Anew, records,
                 eliminate, last, max_fill, nnzA)


# ---- all levels ----------------------------------------------------------------------------------------------------------------------------
def refuses(P):
    """why the model does not run these parameters, or None"""
    if P.n_preprocessing:
        return "preprocessing"
    if P.drop_rules & DROP_INVERSE:
        return "inverse-based dropping"
    if P.drop_rules & (DROP_WEIGHTED | DROP_WEIGHTED2):
        return "weighted dropping"
    if (P.permute_rows in (0, 1)) and (not P.begin_total_piv or P.total_piv == 0) and P.piv_tol == 0.0:
        return "the factorisation without pivoting (partialILUC)"
    return None


def multilevel(ptr, idx, val, is_csr, P, **variants):
    """orc_ml_create's loop for parameters without preprocessing: the levels; variants go to level 0"""
    why = refuses(P)
    if why:
        raise NotImplementedError("tests/dp_ref.py does not model " + why)
    rows = ([int(x) for x in ptr], [int(x) for x in idx], [float(x) for x in val])
    if not is_csr:
        rows = other_orientation(*rows)
    tau, levels = P.threshold, []
    while True:
        m, nz = len(rows[0]) - 1, rows[0][-1]
        in_loop = m > P.min_ml_size and len(levels) < P.max_levels - 1 and nz > 0
        if not in_loop and not m > 0:
            break
        if not in_loop and P.use_final_threshold:
            tau *= P.final_threshold
        last = (m - 1) // 2 if in_loop else m - 1
        bpr, epr = {0: (0, 0), 1: (m, m - 1), 2: (0, last if in_loop else m - 1)}.get(P.permute_rows, (0, m - 1))
        bp = {0: m, 1: last + 1 if in_loop else m}.get(P.total_piv, 0)
        lev = level(rows, P, not in_loop, tau, bp, bpr, epr, **(variants if not levels else {}))
        levels.append(lev)
        rows = lev.Anew
        if not in_loop:
            break
        tau *= P.vary_threshold_factor
    return levels


def level_arrays(lev):
    """a level of the model in the order of ml_cases.level_arrays"""
    one = np.ones(lev.n)
    return [lev.L[0], lev.L[1], lev.L[2], lev.U[0], lev.U[1], lev.U[2], lev.D, lev.perm_rows, lev.perm_cols, lev.inv_perm_rows, lev.inv_perm_cols, one, one]


def launches(levels, store=None, start_lds=True):
    """[(n, "LDS" | "memory", status, step)]: what pilucdp_level's loop prints under ILUPP_DEBUG, level after level.  store: the value of
    ILUPP_DP_STORE (None: the stores of the library, 2 nnz + 8 n + 1024 and nnz + 2 n + 1024 entries, doubled when they fill up)"""
    out = []
    for lev in levels:
        n, recs = lev.n, lev.records
        row_max = lev.max_fill + 1
        if store is None:
            cap = {1: 2 * lev.nnz + 8 * n + 1024, 2: 2 * lev.nnz + 8 * n + 1024, 3: lev.nnz + 2 * n + 1024}
        else:
            cap = {1: n + 2 + store, 2: n + 2 + store, 3: n + 2 + store}
        in_lds, k = start_lds, 0
        while True:
            status = 0
            while k < n:
                r = recs[k]
                if r["pU"] + row_max > cap[1]:
                    status = 1
                elif r["pL"] + row_max > cap[2]:
                    status = 2
                elif not r["eliminate"] and r["pS"] + row_max > cap[3]:
                    status = 3
                elif in_lds and r["stop"] is not None:
                    status = 4
                if status:
                    break
                k += 1
            out.append((n, "LDS" if in_lds else "memory", status, k))
            if status == 0:
                break
            if status == 4:
                in_lds = False
            else:
                cap[status] = cap[status] + n + 2 + store if store is not None else 2 * cap[status] + n + 1024
    return out


def figures(levels):
    """the largest znnz, wnnz and probe seen over all steps of all levels"""
    recs = [r for lev in levels for r in lev.records]
    return dict(znnz=max(r["znnz"] for r in recs), wnnz=max(r["wnnz"] for r in recs),
                probe=max(max(r["zprobe"][0], r["wprobe"][0]) for r in recs), wrapped=any(r["zprobe"][1] or r["wprobe"][1] for r in recs))
