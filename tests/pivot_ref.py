"""A stepwise CPU model of the two pivoting chains, ILUTP2 (ilupp_amd/csrc/ilutp.hip: tp_chain / tp_select) and ILUCP4
(ilupp_amd/csrc/ilucp.hip: cp_chain), in plain Python floats.  It restates the reference's order of operations -- the insertion order of
the working row, norms summed in slot order, candidates in slot order, the reference's partial sort (select_largest, piluc_dev.h) exactly
as written, the FIRST of equal maxima, ILUCP's linked lists threaded as ILUC.hpp:37-101 -- so that its factors, permutation, zero-pivot
count and error have the oracle's bits (tests/test_pivot_ref.py), and it keeps one record per row (ILUTP) or step (ILUCP) that says which
pass boundary, tie rule and selection branch the row reached.  route(records) sums the records up into the figures the cases of
tests/pivot_cases.py pin.

What the oracle does not return and the model does: the row or step at which an error is raised, and which store overflowed
(ILUTP checks L then U, ILUCP checks U then L).

The arrays are the major-order view of the input (ILUTP: rows; ILUCP: the reference's Acol); both orientations of one set of arrays give
the same factors, only apply differs."""
import collections
import heapq
import math

import numpy as np

OK, ERR_ZERO_PIVOT, ERR_MEMORY = 0, 1, 3
PASS = 64                                   # entries per pass of every loop of the two kernels

Result = collections.namedtuple("Result", "L U perm zero_pivots err err_at err_store records")


def tp_cap(n):
    """slots of ILUTP's working row (ilutp_factor): 4 * ((n + 64) & ~15)"""
    return 4 * ((n + 64) & ~15)


def select_largest(data, lst, left, right, m):
    """vector_dense::sort(list, left, right, m), sparse_implementation.h:507-563, as piluc_dev.h states it: the m largest to the end"""
    k = right - m + 1

    def sw(x, y):
        data[x], data[y] = data[y], data[x]
        lst[x], lst[y] = lst[y], lst[x]
    while True:
        if right <= left + 1:
            if right == left + 1 and data[right] < data[left]:
                sw(left, right)
            return
        mid = (left + right) // 2
        sw(mid, left + 1)
        if data[left] > data[right]:
            sw(left, right)
        if data[left + 1] > data[right]:
            sw(left + 1, right)
        if data[left] > data[left + 1]:
            sw(left, left + 1)
        i, j = left + 1, right
        a, a_list = data[left + 1], lst[left + 1]
        while True:
            i += 1
            while data[i] < a:
                i += 1
            j -= 1
            while data[j] > a:
                j -= 1
            if j < i:
                break
            sw(i, j)
        data[left + 1], lst[left + 1] = data[j], lst[j]
        data[j], lst[j] = a, a_list
        if j >= k:
            right = j - 1
        if j <= k:
            left = i


def first_max(key, lo, hi):
    """(position of the first largest key in [lo, hi), positions of all keys equal to it); strictly greater wins"""
    pos = lo
    for i in range(lo + 1, hi):
        if key[i] > key[pos]:
            pos = i
    return pos, [i for i in range(lo, hi) if key[i] == key[pos]]


def reserved(n, nnz, fill_in, mem_factor):
    """(the fill bound as clipped, the entries either store may hold): min(max_fill_in * n, (Integer) mem_factor * nnz)"""
    fill_in = max(1, fill_in)
    fill_in = min(fill_in, n)
    return fill_in, max(0, min(fill_in * n, int(mem_factor) * nnz))


def _compress(ptr, idx, val):
    """matrix_sparse::compress(0): keep |x| > 0 (a NaN goes too), in order"""
    n = len(ptr) - 1
    optr, oidx, oval = [0], [], []
    for r in range(n):
        for j in range(ptr[r], ptr[r + 1]):
            if abs(val[j]) > 0.0:
                oidx.append(idx[j]); oval.append(val[j])
        optr.append(len(oidx))
    return optr, oidx, oval


def _arrays(ptr, idx, val):
    return (np.array(val, dtype=np.float64), np.array(idx, dtype=np.int32), np.array(ptr, dtype=np.int32))


def _sort_rows(ptr, idx, val, key):
    for r in range(len(ptr) - 1):
        b0, b1 = ptr[r], ptr[r + 1]
        order = sorted(range(b0, b1), key=lambda j: key(idx[j]))
        idx[b0:b1], val[b0:b1] = [idx[j] for j in order], [val[j] for j in order]


# ------------------------------------------------------------------ ILUTP ------------------------------------------------------------------
def _tp_select(data, pointer, invperm, n_L, n_U, tau_L, tau_U, mid, with_piv, piv_tol):
    """ilutp_select of the oracle / tp_select of the kernel; returns (list_L, list_U, record)"""
    nnz = len(data)
    accL = accU = larg = potpiv = 0.0
    pos_pot = -1
    termsL, termsU = [], []
    for i in range(nnz):
        a = abs(data[i])
        if invperm[pointer[i]] < mid:
            accL += data[i] * data[i]; termsL.append(data[i] * data[i])
        else:
            accU += data[i] * data[i]; termsU.append(data[i] * data[i])
            if with_piv:
                if a > larg:
                    larg = a
                if invperm[pointer[i]] == mid:
                    potpiv, pos_pot = a, i
    nrmL, nrmU = math.sqrt(accL), math.sqrt(accU)
    keep_diag = pos_pot if (with_piv and not (larg * piv_tol >= potpiv or pos_pot < 0)) else -1
    kL, lL, kU, lU, slotU = [], [], [], [], []
    for i in range(nnz):
        a = nrmU if i == keep_diag else abs(data[i])
        if invperm[pointer[i]] < mid:
            if a > nrmL * tau_L:
                kL.append(a); lL.append(pointer[i])
        elif a > nrmU * tau_U:
            kU.append(a); lU.append(pointer[i]); slotU.append(i)
    cL, cU = len(kL), len(kU)
    rec = dict(ns=nnz, cL=cL, cU=cU, cutL=cL > n_L, cutU=cU > n_U, n_L=n_L, n_U=n_U, keep_diag=keep_diag >= 0, diag_slot=pos_pot,
               at_tol=bool(with_piv and pos_pot >= 0 and larg * piv_tol == potpiv), termsL=termsL, termsU=termsU, with_piv=with_piv,
               max_pos=None, max_ties=[], max_slots=[], offU=0, tie_at_cutL=False, tie_at_cutU=False, max_key=None, key_before_cut=None)
    if cL > n_L:
        off = cL - n_L
        select_largest(kL, lL, 0, cL - 1, n_L)
        rec["tie_at_cutL"] = n_L > 0 and kL[off - 1] == kL[off]
        lL = lL[off:]
    if cU > 0:
        off = 0
        if cU > n_U:
            off = cU - n_U
            select_largest(kU, lU, 0, cU - 1, n_U)
            rec.update(tie_at_cutU=kU[off - 1] == kU[off], key_before_cut=kU[off - 1])        # (the largest key the cut leaves out)
            slotU = None
        pos, ties = first_max(kU, off, cU)
        rec.update(max_pos=pos, max_key=kU[pos], max_ties=ties, offU=off, max_slots=[slotU[t] for t in ties] if slotU else [])
        lU[pos], lU[cU - 1] = lU[cU - 1], lU[pos]
        lU = lU[off:]
    return lL, lU, rec


def ilutp(ptr, idx, val, fill_in=100, threshold=0.1, piv_tol=0.1, rp=-1, mem_factor=10.0):
    """ILUTP2 (ILUTP.hpp:13-140) on the rows ptr / idx / val"""
    ptr, idx, val = [int(x) for x in ptr], [int(x) for x in idx], [float(x) for x in val]
    n = len(ptr) - 1
    fill_in, cap_store = reserved(n, ptr[n], fill_in, mem_factor)
    perm, invperm = list(range(n)), list(range(n))
    Lp, Li, Lv, Up, Ui, Uv = [0], [], [], [0], [], []
    zero_pivots, records = 0, []
    err, err_at, err_store = OK, n, None
    for i in range(n):
        if i == rp:
            piv_tol = 1.0
        data, pointer, occ, keyslot, heap = [], [], {}, {}, []
        rec = dict(row=i, stored=ptr[i + 1] - ptr[i], elims=[], drops=0, dropped_cols=[], selects=[], second=False, zp=None, pL0=Lp[i], pU0=Up[i], reserved=cap_store)

        def slot(j, k):
            if occ.get(j, -1) < 0:
                occ[j] = len(data); pointer.append(j); data.append(0.0)
                heapq.heappush(heap, k); keyslot[k] = occ[j]
            return occ[j]
        acc, terms = 0.0, []
        for k in range(ptr[i], ptr[i + 1]):
            j = invperm[idx[k]]
            data[slot(idx[k], j)] = val[k]
            if j < i:
                acc += val[k] * val[k]; terms.append(val[k] * val[k])
        norm_wL = math.sqrt(acc)
        rec.update(distinct=len(data), ns_load=len(data), norm_terms=terms)
        while heap and heap[0] < i:
            k = heap[0]
            x = keyslot[k]
            if abs(data[x]) < threshold * norm_wL:
                if occ.get(pointer[x], -1) >= 0:
                    data[occ[pointer[x]]] = 0.0; occ[pointer[x]] = -1
                keyslot[k] = -1; heapq.heappop(heap)
                rec["drops"] += 1
                rec["dropped_cols"].append(pointer[x])
            else:
                if threshold > 0.0 and norm_wL > 0.0:
                    rec.setdefault("kept_at_eq", []).append(abs(data[x]) == threshold * norm_wL)
                data[x] = data[x] / Uv[Up[k]]
                wk = data[x]
                heapq.heappop(heap)
                new, ns0 = 0, len(data)
                for j in range(Up[k] + 1, Up[k + 1]):
                    y = slot(Ui[j], invperm[Ui[j]])
                    data[y] -= wk * Uv[j]
                new = len(data) - ns0
                rec["elims"].append(dict(pos=k, slot=x, ns=ns0, ulen=Up[k + 1] - Up[k] - 1, new=new))
        rec.update(ns_elim=len(data), dead=sum(1 for s in range(len(data)) if occ.get(pointer[s], -1) != s),
                   nonfinite=any(not math.isfinite(x) for x in data))
        lL, lU, s1 = _tp_select(data, pointer, invperm, fill_in - 1, fill_in, threshold, threshold, i, True, piv_tol)
        rec["selects"].append(s1)
        if not lU:
            if threshold > 0.0:
                lL, lU, s2 = _tp_select(data, pointer, invperm, fill_in - 1, fill_in, threshold, 0.0, i, False, 0.0)
                rec["selects"].append(s2); rec["second"] = True
            if not lU:
                zero_pivots += 1
                rec["zp"] = "reuse" if occ.get(perm[i], -1) >= 0 else "new"
                data[slot(perm[i], i)] = 1.0
                lU = [perm[i]]
        nL, nU = len(lL), len(lU)
        rec.update(ns=len(data), nL=nL, nU=nU)
        records.append(rec)
        if Lp[i] + nL + 1 > cap_store:
            err, err_at, err_store = ERR_MEMORY, i, "L"
            break
        for j in range(nL):
            c = lL[nL - 1 - j]
            Lv.append(data[occ[c]]); Li.append(invperm[c])
        Lv.append(1.0); Li.append(i); Lp.append(Lp[i] + nL + 1)
        if Up[i] + nU > cap_store:
            err, err_at, err_store = ERR_MEMORY, i, "U"
            break
        for j in range(nU):
            c = lU[nU - 1 - j]
            Uv.append(data[occ[c]]); Ui.append(c)
        Up.append(Up[i] + nU)
        c = Ui[Up[i]]
        p = invperm[c]
        invperm[perm[i]], invperm[c] = invperm[c], invperm[perm[i]]
        perm[i], perm[p] = perm[p], perm[i]
        rec.update(pL1=Lp[i + 1], pU1=Up[i + 1], pivot_col=c)
        if Uv[Up[i]] == 0:
            err, err_at = ERR_ZERO_PIVOT, i
            break
    if err != OK:
        return Result(None, None, None, zero_pivots, err, err_at, err_store, records)
    Lp, Li, Lv = _compress(Lp, Li, Lv)
    Up, Ui, Uv = _compress(Up, Ui, Uv)
    _sort_rows(Up, Ui, Uv, lambda c: invperm[c])
    _sort_rows(Lp, Li, Lv, lambda c: c)
    return Result(_arrays(Lp, Li, Lv), _arrays(Up, Ui, Uv), np.array(perm, dtype=np.int32), zero_pivots, OK, n, None, records)


# ------------------------------------------------------------------ ILUCP ------------------------------------------------------------------
class _Vec:
    """vector_sparse_dynamic: slots in insertion order, occupancy by index"""

    def __init__(self):
        self.data, self.pointer, self.occ = [], [], {}

    def slot(self, j):
        if self.occ.get(j, -1) < 0:
            self.occ[j] = len(self.data); self.pointer.append(j); self.data.append(0.0)
        return self.occ[j]


def _cp_take_pivot_last(v, n, tau, pivot_position, piv_tol):
    """take_largest_elements_by_abs_value_with_threshold_pivot_last, sparse_implementation.h:1151-1216; returns (list, record)"""
    larg = norm = 0.0
    for x in v.data:
        if abs(x) > larg:
            larg = abs(x)
        norm += x * x
    at_pivot = v.data[v.occ[pivot_position]] if v.occ.get(pivot_position, -1) >= 0 else 0.0
    rec = dict(at_tol=larg * piv_tol == abs(at_pivot) and at_pivot != 0, lim=n, terms=[x * x for x in v.data], max_ties=[], tie_at_cut=False)
    key, lst = [], []
    if larg * piv_tol > abs(at_pivot):
        norm = math.sqrt(norm)
        for x, c in zip(v.data, v.pointer):
            if abs(x) > norm * tau:
                key.append(abs(x)); lst.append(c)
        cnt = len(lst)
        rec.update(branch="pivoting", cnt=cnt, cut=cnt > n)
        if cnt > n:
            off = cnt - n
            select_largest(key, lst, 0, cnt - 1, n)
            rec["tie_at_cut"] = key[off - 1] == key[off]
            lst = lst[off:]
        elif cnt > 0:
            pos, mx = 0, 0.0
            for i in range(cnt):
                if key[i] > mx:
                    pos, mx = i, key[i]
            rec["max_ties"] = [i for i in range(cnt) if key[i] == key[pos]]
            lst[pos], lst[cnt - 1] = lst[cnt - 1], lst[pos]
        return lst, rec
    if at_pivot == 0:
        rec.update(branch="neither", cnt=0, cut=False)
        return [], rec
    norm = math.sqrt(norm)
    for x, c in zip(v.data, v.pointer):
        if abs(x) > norm * tau and c != pivot_position:
            key.append(abs(x)); lst.append(c)
    cnt = len(lst)
    rec.update(branch="kept", cnt=cnt, cut=cnt > n - 1)
    if cnt > n - 1:
        off = cnt - n + 1
        select_largest(key, lst, 0, cnt - 1, n)
        rec["tie_at_cut"] = n > 1 and key[off - 1] == key[off]
        lst = lst[off:off + n - 1] + [pivot_position]
    else:
        lst.append(pivot_position)
    return lst, rec


def ilucp(ptr, idx, val, fill_in=100, threshold=0.1, piv_tol=0.1, rp=-1, mem_factor=10.0):
    """ILUCP4 (ILUC.hpp:212-370) on the major slices ptr / idx / val (the reference's columns)"""
    ptr, idx, val = [int(x) for x in ptr], [int(x) for x in idx], [float(x) for x in val]
    n = len(ptr) - 1
    fill_in, cap_store = reserved(n, ptr[n], fill_in, mem_factor)
    perm, invperm, nonpiv = list(range(n)), list(range(n)), [True] * n
    firstL, listL = [0] * (n + 1), [-1] * (n + 1)
    listA, headA, firstA = [0] * (n + 1), [-1] * (n + 1), [0] * (n + 1)
    startU, linkU, rowU = [-1] * n, {}, {}
    Lp, Li, Lv, Up, Ui, Uv = [0], [], [], [0], [], []
    for k in range(n):                                      # initialize_sparse_matrix_fields, ILUC.hpp:74-84
        firstA[k] = ptr[k]
        if ptr[k] < ptr[k + 1]:
            listA[k] = headA[idx[ptr[k]]]; headA[idx[ptr[k]]] = k
    zero_pivots, records = 0, []
    err, err_at, err_store = OK, n, None
    for k in range(n):
        if k == rp:
            piv_tol = 1.0
        z = _Vec()
        rec = dict(step=k, nrow=0, nonpiv=0, zsubs=[], selects=[], zp=False, pU0=Up[k], pL0=Lp[k], wsubs=[], reserved=cap_store)
        h = headA[k]
        while h != -1:
            rec["nrow"] += 1
            if nonpiv[h]:
                rec["nonpiv"] += 1
                z.data[z.slot(h)] = val[firstA[h]]
            h = listA[h]
        h = listL[k]
        while h != -1:
            ns0, dead = len(z.data), 0
            for j in range(Up[h], Up[h + 1]):
                if nonpiv[Ui[j]]:
                    x = z.slot(Ui[j])
                    z.data[x] -= Lv[firstL[h]] * Uv[j]
                else:
                    dead += 1
            rec["zsubs"].append(dict(len=Up[h + 1] - Up[h], dead=dead, new=len(z.data) - ns0, ns=ns0))
            h = listL[h]
        rec.update(znnz=len(z.data), nonfinite=any(not math.isfinite(x) for x in z.data))
        lU, s = _cp_take_pivot_last(z, fill_in, threshold, perm[k], piv_tol)
        rec["selects"].append(s)
        if not lU and threshold > 0.0:
            lU, s = _cp_take_pivot_last(z, fill_in, 0.0, perm[k], piv_tol)
            rec["selects"].append(s)
        if not lU:
            zero_pivots += 1
            rec["zp"] = True
            z.data[z.slot(perm[k])] = 1.0
            lU = [perm[k]]
        nU = len(lU)
        rec["nU"] = nU
        records.append(rec)
        if Up[k] + nU > cap_store:
            err, err_at, err_store = ERR_MEMORY, k, "U"
            break
        Uv.append(z.data[z.occ[lU[nU - 1]]]); Ui.append(lU[nU - 1])
        for j in range(1, nU):
            pos, c = Up[k] + j, lU[nU - 1 - j]
            Uv.append(z.data[z.occ[c]]); Ui.append(c)
            linkU[pos] = startU[c]; startU[c] = pos; rowU[pos] = k
        Up.append(Up[k] + nU)
        c = Ui[Up[k]]
        p = invperm[c]
        invperm[perm[k]], invperm[c] = invperm[c], invperm[perm[k]]
        perm[k], perm[p] = perm[p], perm[k]
        nonpiv[c] = False
        w = _Vec()
        below = dups = 0
        seen = set()
        for i in range(ptr[perm[k]], ptr[perm[k] + 1]):
            if idx[i] > k:
                below += 1
                dups += idx[i] in seen
                seen.add(idx[i])
                w.data[w.slot(idx[i])] = val[i]
        rec.update(pivot_col=c, col_len=ptr[c + 1] - ptr[c], col_below=below, col_dups=dups)
        h = startU[perm[k]]
        while h != -1:
            r, uv = rowU[h], Uv[h]
            h = linkU[h]
            ns0 = len(w.data)
            for j in range(Lp[r], Lp[r + 1]):
                x = w.slot(Li[j])
                w.data[x] -= uv * Lv[j]
            rec["wsubs"].append(dict(len=Lp[r + 1] - Lp[r], new=len(w.data) - ns0, ns=ns0))
        # take_largest_elements_by_abs_value_with_threshold(list_L, max_fill_in - 1, threshold, k + 1, n), :1322-1357
        zz, terms = 0.0, []
        for x, r in zip(w.data, w.pointer):
            if k + 1 <= r < n:
                zz += x * x; terms.append(x * x)
        norm = math.sqrt(zz)
        key, lL = [], []
        for x, r in zip(w.data, w.pointer):
            if k + 1 <= r < n and abs(x) > norm * threshold:
                key.append(abs(x)); lL.append(r)
        cntL, lim = len(lL), fill_in - 1
        tie = False
        if cntL > lim:
            off = cntL - lim
            select_largest(key, lL, 0, cntL - 1, lim)
            tie = lim > 0 and key[off - 1] == key[off]
            lL = lL[off:]
        lL.sort()
        nL = len(lL)
        rec.update(wnnz=len(w.data), cntL=cntL, limL=lim, nL=nL, cutL=cntL > lim, tie_at_cutL=tie, wterms=terms)
        if Lp[k] + nL + 1 > cap_store:
            err, err_at, err_store = ERR_MEMORY, k, "L"
            break
        Lv.append(1.0); Li.append(k)
        for r in lL:
            Lv.append(w.data[w.occ[r]] / Uv[Up[k]]); Li.append(r)
        Lp.append(Lp[k] + nL + 1)
        rec.update(pU1=Up[k + 1], pL1=Lp[k + 1])
        # update_sparse_matrix_fields, ILUC.hpp:86-101
        h = headA[k]
        while h != -1:
            firstA[h] += 1
            h = listA[h]
        h = headA[k]
        while h != -1:
            i = h
            h = listA[i]
            if firstA[i] < ptr[i + 1]:
                listA[i] = headA[idx[firstA[i]]]; headA[idx[firstA[i]]] = i
        # update_triangular_fields, ILUC.hpp:37-63
        h = listL[k]
        while h != -1:
            firstL[h] += 1
            h = listL[h]
        firstL[k] = Lp[k] + 1
        h = listL[k]
        if Lp[k] + 1 < Lp[k + 1]:
            j = Li[Lp[k] + 1]
            listL[k] = listL[j]; listL[j] = k
        while h != -1:
            i = h
            h = listL[i]
            if firstL[i] < Lp[i + 1]:
                j = Li[firstL[i]]
                listL[i] = listL[j]; listL[j] = i
    if err != OK:
        return Result(None, None, None, zero_pivots, err, err_at, err_store, records)
    Lp, Li, Lv = _compress(Lp, Li, Lv)
    Up, Ui, Uv = _compress(Up, Ui, Uv)
    return Result(_arrays(Lp, Li, Lv), _arrays(Up, Ui, Uv), np.array(perm, dtype=np.int32), zero_pivots, OK, n, None, records)


# ------------------------------------------------------------------ figures ------------------------------------------------------------------
def passes(count):
    """how many 64-entry passes a loop over `count` entries takes"""
    return (count + PASS - 1) // PASS


def route(records):
    """the figures the cases pin, over all rows (ILUTP) or steps (ILUCP) of one run"""
    f = collections.OrderedDict()
    if records and "row" in records[0]:
        sel = [s for r in records for s in r["selects"]]
        el = [e for r in records for e in r["elims"]]
        f["max_stored"] = max(r["stored"] for r in records)
        f["max_distinct"] = max(r["distinct"] for r in records)
        f["max_ns"] = max(r["ns"] for r in records)
        f["max_norm_terms"] = max(len(r["norm_terms"]) for r in records)
        f["max_ulen"] = max([e["ulen"] for e in el], default=-1)
        f["ulens"] = sorted(set(e["ulen"] for e in el))
        f["max_new"] = max([e["new"] for e in el], default=0)
        f["append_across_pass"] = any(e["new"] > 0 and e["ns"] // PASS != (e["ns"] + e["new"] - 1) // PASS for e in el)
        f["mixed_pass"] = any(0 < e["new"] < e["ulen"] for e in el)
        f["min_search_ns"] = sorted(set(e["ns"] for e in el))
        f["drops"] = sum(r["drops"] for r in records)
        f["dead"] = max(r["dead"] for r in records)
        f["cL"] = sorted(set(s["cL"] for s in sel))
        f["cU"] = sorted(set(s["cU"] for s in sel))
        f["cutL"] = sorted(set(s["n_L"] for s in sel if s["cutL"]))
        f["cutU"] = sorted(set(s["n_U"] for s in sel if s["cutU"]))
        f["tie_at_cut"] = any(s["tie_at_cutL"] or s["tie_at_cutU"] for s in sel)
        f["keep_diag"] = sum(1 for s in sel if s["keep_diag"])
        f["at_tol"] = sum(1 for s in sel if s["at_tol"])
        f["second"] = sum(1 for r in records if r["second"])
        f["zp_new"] = sum(1 for r in records if r["zp"] == "new")
        f["zp_reuse"] = sum(1 for r in records if r["zp"] == "reuse")
        f["max_nL"] = max(r["nL"] for r in records)
        f["max_nU"] = max(r["nU"] for r in records)
        f["nonfinite"] = any(r["nonfinite"] for r in records)
    elif records:
        sel = [s for r in records for s in r["selects"]]
        f["nrow"] = sorted(set(r["nrow"] for r in records))
        f["filtered"] = max(r["nrow"] - r["nonpiv"] for r in records)
        f["zsub_lens"] = sorted(set(s["len"] for r in records for s in r["zsubs"]))
        f["wsub_lens"] = sorted(set(s["len"] for r in records for s in r["wsubs"]))
        f["zsub_dead"] = max([s["dead"] for r in records for s in r["zsubs"]], default=0)
        f["append_across_pass"] = any(s["new"] > 0 and s["ns"] // PASS != (s["ns"] + s["new"] - 1) // PASS for r in records for s in r["zsubs"] + r["wsubs"])
        f["max_znnz"] = max(r["znnz"] for r in records)
        f["branches"] = sorted(set((s["branch"], q) for r in records for q, s in enumerate(r["selects"])))
        f["cuts"] = sorted(set((s["branch"], s["cnt"], s["lim"]) for s in sel if s["cut"]))
        f["at_tol"] = sum(1 for s in sel if s["at_tol"])
        f["zp"] = sum(1 for r in records if r["zp"])
        f["col_len"] = sorted(set(r["col_len"] for r in records if "col_len" in r))
        f["col_dups"] = max([r["col_dups"] for r in records if "col_dups" in r], default=0)
        f["nL"] = sorted(set(r["nL"] for r in records if "nL" in r))
        f["cutL"] = sorted(set(r["limL"] for r in records if r.get("cutL")))
        f["max_wnnz"] = max([r["wnnz"] for r in records if "wnnz" in r], default=0)
        f["nonfinite"] = any(r["nonfinite"] for r in records)
    return f
