"""The capacity ladders of the dataflow factorisations (iluc_df.hip, piluc_df.hip, icholt_df.hip): matrices whose working rows sit exactly
on a capacity or one past it, the capacity tables of the kernels' classes, and a CPU model of the per-step demands of ILUC and of one
level of partial ILUC that gives the route (the classes tried, in order) a matrix takes.  ICholT has no such model here: its touch records
count the reaches of PRE-drop working columns, which the oracle's finished factor does not show; its cases are arrows whose demands
follow from the pattern alone.  numpy / scipy only: shared by tests/test_capacity_cases.py (no GPU) and
tests/test_gpu_capacity_ladders.py.

A class holds three quantities per step and half: gathered entries (ne <= NE), slots (na, ns <= NS) and touch records (nt <= T).  The
kernels stop an attempt with a capacity code -- 11 (A's part) / 13 (entries) / 14 (slots): "entries"; 12 (records read) / 15 (records
written): "records" -- and the host goes on in another class.  The first code written wins a race, so a route is deterministic only where
every step that can fail first fails for the same cause: the model reports a mixed cause as None."""
import numpy as np
import scipy.sparse as sp

# (NE, NS, T) of the LDS classes: the template arguments of k_iluc_df / k_piluc_df / k_icholt_df at their launches
ILUC_CLASSES = ((256, 128, 32), (768, 256, 64), (1024, 512, 128), (960, 256, 512))
PILUC_CLASSES = ((256, 128, 32), (768, 256, 64), (1024, 512, 128), (768, 256, 512))
ICHOLT_CLASSES = ((128, 64, 32), (256, 128, 64), (1024, 512, 128))
ICHOLT_LARGEST = (1 << 18, 2048, 1 << 16)           # class 3: gNE, gNS, the limit of T
ILUC_REFUSAL = "ILUC: a working row does not fit the largest capacity class"

RECORDS, ENTRIES = "records", "entries"


def iluc_class(cls, n):
    """(NE, NS, T) of ILUC's class `cls` for a matrix of n rows (iluc_attempt: the global class sizes its arrays by n; its 2^19 entries are
    halved, down to 4 096, while the waves' slices together exceed the memory set aside for them, which depends on the device: with
    16 384 slots and 4 096 records a wave may be left with as few as 16 384 entries)"""
    if cls < 4:
        return ILUC_CLASSES[cls]
    T = 16
    while T < 4096 and T < n:
        T *= 2
    ns = 1024
    while ns < n + 1 and ns < 16384:
        ns *= 2
    return (1 << 19, ns, T)


def iluc_start(nnz, n, fill):
    """iluc_factor's rule for the class it starts in"""
    fill = max(int(fill), 1)
    est = (nnz // n // 2 + 1 + fill) * fill
    return 0 if est <= 192 else (1 if est <= 640 else 2)


def iluc_next(cls, cause):
    """the class iluc_factor tries after a capacity failure in `cls` (5: refused).  Records: 0 -> 3, 1 -> 3, 2 -> 3 -> 4 (cls = 2 inside a
    loop that then increments); entries or slots: 0 -> 1 -> 2 -> 4"""
    if cause == RECORDS:
        return 3 if cls < 2 else cls + 1
    return 4 if cls == 2 else cls + 1


def piluc_start(nnz, n):
    avg = nnz // n + 1
    return 0 if avg <= 16 else (1 if avg <= 40 else 2)


def piluc_next(cls, cause):
    """piluc_level's ladder below the global class: records 0 / 1 -> 2 -> 3 -> 4, entries or slots 0 -> 1 -> 2 -> 4, 3 -> 4"""
    if cause == RECORDS:
        return 2 if cls < 2 else cls + 1
    return cls + 1 if cls < 2 else 4


def icholt_T(nnz_tri, n, fill, cls):
    """touch records per row of icholt_attempt (nnz_tri: entries of the triangle it factorises); None where the class refuses T"""
    avg = nnz_tri // n + 1
    T = 16
    limit = ICHOLT_LARGEST[2] if cls == 3 else 128
    while T < 4 * (avg + max(fill, 0)) and T < limit:
        T *= 2
    if cls == 3:
        while T < limit and T < n and n * T * 64 <= (8 << 30):
            T *= 2
    if (cls == 1 and T > 64) or (cls == 0 and T > 32):
        return None
    return T


# ---- generators: strictly diagonally dominant, no cancellation, every stored entry of the factors nonzero ------------------------
def _csr(n, rows, cols, vals):
    A = sp.csr_matrix((np.asarray(vals, dtype=np.float64), (np.asarray(rows), np.asarray(cols))), shape=(n, n))
    A.sort_indices()
    return A


def arrow_last(N):
    """diagonal, a dense last row, a dense last column: step N-1 is reached by N-1 stored entries in each factor (the touch-record family)"""
    i = np.arange(N - 1)
    rows = np.concatenate([np.arange(N), np.full(N - 1, N - 1), i])
    cols = np.concatenate([np.arange(N), i, np.full(N - 1, N - 1)])
    vals = np.concatenate([4.0 * N + 0.25 * np.arange(N), -(1.0 + i / N), 1.0 + 0.5 * i / N])
    return _csr(N, rows, cols, vals)


def arrow_first(N):
    """diagonal, a dense first row, a dense first column: the factors fill completely"""
    i = np.arange(1, N)
    rows = np.concatenate([np.arange(N), np.zeros(N - 1, dtype=int), i])
    cols = np.concatenate([np.arange(N), i, np.zeros(N - 1, dtype=int)])
    vals = np.concatenate([4.0 * N + 0.25 * np.arange(N), -(1.0 + i / N), 1.0 + 0.5 * i / N])
    return _csr(N, rows, cols, vals)


def row_first(N, ties=False):
    """diagonal plus a dense first row: step 0 has N entries of A right of the diagonal (na = ns = ne = N).  ties: every off-diagonal entry
    of the same magnitude, so the cut of the top (fill - 1) falls between equal candidates (the kernel's one-lane sort)"""
    j = np.arange(1, N)
    rows = np.concatenate([np.arange(N), np.zeros(N - 1, dtype=int)])
    cols = np.concatenate([np.arange(N), j])
    off = np.ones(N - 1) if ties else 0.5 + j / (2.0 * N)
    vals = np.concatenate([2.0 * N + 0.25 * (np.arange(N) % 64), off])
    return _csr(N, rows, cols, vals)


def comb(c, t, e):
    """n = c + 1 + t.  Rows 0..c-1: the diagonal and t entries in the last t columns; row c: an entry in every column < c, the diagonal and e
    of the last t columns; rows > c: the diagonal.  Step c gathers 1 + e + c t entries from c records into t + 1 slots (the gathered-entries
    family); the steps above it read c + 1 records each"""
    n = c + 1 + t
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [4.0 * (c + t) + 0.5 * np.arange(n)]
    last = np.arange(c + 1, n)
    for r in range(c):
        rows.append(np.full(t, r)); cols.append(last); vals.append(0.25 + (r % 7) / 16.0 + np.arange(t) / 64.0)
    rows.append(np.full(c, c)); cols.append(np.arange(c)); vals.append(-(0.5 + (np.arange(c) % 5) / 8.0))
    rows.append(np.full(e, c)); cols.append(last[:e]); vals.append(1.0 + np.arange(e) / 32.0)
    return _csr(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def spd_arrow_last(N):
    A = sp.lil_matrix((N, N))
    A.setdiag(float(N))
    A[N - 1, :N - 1] = -0.5
    A[:N - 1, N - 1] = -0.5
    A = A.tocsr(); A.sort_indices()
    return A


def spd_arrow_first(N):
    A = sp.lil_matrix((N, N))
    A.setdiag(float(N))
    A[0, 1:] = -0.5
    A[1:, 0] = -0.5
    A = A.tocsr(); A.sort_indices()
    return A


def without_diagonal(A, rows):
    """A with the diagonal entries of `rows` removed from the pattern (structural zero pivots)"""
    B = A.tolil()
    for r in rows:
        B[r, r] = 0.0
    B = B.tocsr(); B.eliminate_zeros(); B.sort_indices()
    return B


def as_input(A):
    A = A.copy(); A.sort_indices()
    return (A.data.astype(np.float64), A.indices.astype(np.int32), A.indptr.astype(np.int32), sp.isspmatrix_csr(A))


# ---- the demand model of ILUC ------------------------------------------------------------------------------------------------------
def iluc_demands(A, L, U, w_from_diagonal=False):
    """for every step k and both halves (0: z, row k of U; 1: w, column k of L) the (na, nt, ne, ns) that k_iluc_df counts, from A (CSR: the
    major-order view the kernel gets) and the finished factors L (by columns, the 1 first) and U (by rows, the pivot first) as the oracle
    returns them.  nt: the stored l(k,h) / u(h,k); ne: na plus the stored tails u(h, j >= k) / l(i > k, h); ns: the union of the index sets.
    w_from_diagonal: partial ILUC, whose tails l(i >= k, h) start AT the diagonal index.
    Returns (dem, deps): dem[k][half] = (na, nt, ne, ns), deps[k] = the steps whose records step k reads"""
    A = sp.csr_matrix(A); A.sort_indices()
    n = A.shape[0]
    Ac = A.tocsc(); Ac.sort_indices()
    Ld, Li, Lp = L[0], L[1], L[2]
    Ud, Ui, Up = U[0], U[1], U[2]
    # stored entries besides the leading 1 / pivot: column h of L -> rows > h ascending, row h of U -> columns > h ascending
    Lcol = [Li[Lp[h] + 1:Lp[h + 1]] for h in range(n)]
    Urow = [Ui[Up[h] + 1:Up[h + 1]] for h in range(n)]
    Lrows_of = [[] for _ in range(n)]               # row k -> the h with l(k,h) stored
    Ucols_of = [[] for _ in range(n)]               # column k -> the h with u(h,k) stored
    for h in range(n):
        for i in Lcol[h]:
            Lrows_of[int(i)].append(h)
        for j in Urow[h]:
            Ucols_of[int(j)].append(h)
    dem, deps = [], []
    for k in range(n):
        arow = A.indices[A.indptr[k]:A.indptr[k + 1]]
        acol = Ac.indices[Ac.indptr[k]:Ac.indptr[k + 1]]
        halves = []
        for own, contributors, stored, lo in ((arow[arow >= k], Lrows_of[k], Urow, k), (acol[acol > k], Ucols_of[k], Lcol, k if w_from_diagonal else k + 1)):
            tails = [stored[h][np.searchsorted(stored[h], lo):] for h in contributors]
            na, nt = int(own.shape[0]), len(contributors)
            ne = na + sum(int(t.shape[0]) for t in tails)
            ns = int(np.unique(np.concatenate([own] + tails)).shape[0]) if ne else 0
            halves.append((na, nt, ne, ns))
        dem.append(tuple(halves))
        deps.append(sorted(set(Lrows_of[k]) | set(Ucols_of[k])))
    return dem, deps


def maxima(dem):
    """max over steps and halves of (na, nt, ne, ns)"""
    return tuple(max(h[q] for d in dem for h in d) for q in range(4))


def step_cause(d, cap):
    """why a step with demands d = (z, w) cannot run in a class of capacities cap = (NE, NS, T): RECORDS, ENTRIES or None.  A step reached by
    more than T stored entries never starts: the writer of record T + 1 stops the attempt (code 15), whatever the step would gather"""
    NE, NS, T = cap
    if any(h[1] > T for h in d):
        return RECORDS
    if any(h[0] > NS or h[2] > NE or h[3] > NS for h in d):
        return ENTRIES
    return None


def failing_causes(dem, deps, cap):
    """the causes of the steps that can stop an attempt in a class: a step whose own demand does not fit and whose contributors all finish
    (a step behind a failed one never starts).  {} = the class completes the factorisation; {step: cause} else"""
    failed = np.zeros(len(dem), dtype=bool)
    out = {}
    for k, d in enumerate(dem):
        behind = any(failed[h] for h in deps[k])
        c = step_cause(d, cap)
        if c is not None and not behind:
            out[k] = c
        failed[k] = behind or c is not None
    return out


def iluc_route(dem, deps, n, start):
    """the classes iluc_factor tries from `start`: a list of (class, cause or None for the class that completes), or None where the steps that
    fail in a class disagree about the cause; ends with (4, cause) where class 4 refuses as well"""
    route, cls = [], start
    while cls < 5:
        causes = set(failing_causes(dem, deps, iluc_class(cls, n)).values())
        if not causes:
            route.append((cls, None))
            return route
        if len(causes) > 1:
            return None
        c = causes.pop()
        route.append((cls, c))
        cls = iluc_next(cls, c)
    return route


def piluc_route(dem, deps, n, start):
    """the attempts of piluc_level with the chain kernel switched off: a list of (class, slots of the global class or 0, cause or None), or
    None for a mixed cause.  The global class starts with 2 048 slots and 65 536 entries and grows by factors of 4"""
    route, cls, gns, gne = [], start, 2048, 65536
    T4 = 16
    while T4 < 4096 and T4 < n:
        T4 *= 2
    while True:
        cap = PILUC_CLASSES[cls] if cls < 4 else (max(gne, 2 * gns), gns, T4)
        fails = failing_causes(dem, deps, cap)
        causes = set(fails.values())
        if not causes:
            route.append((cls, gns if cls == 4 else 0, None))
            return route
        if len(causes) > 1:
            return None
        c = causes.pop()
        route.append((cls, gns if cls == 4 else 0, c))
        if cls < 4:
            cls = piluc_next(cls, c)
        elif c == RECORDS:
            return route
        else:
            # (which of the two arrays grows depends on the code: 13 the entries, 11 / 14 the slots)
            over_slots = any(any(h[0] > gns or h[3] > gns for h in dem[k]) for k in fails)
            if over_slots:
                if gns > 2 * n + 2:
                    return route
                gns *= 4
                gne = max(gne, 8 * gns)
            else:
                gne *= 4


def classes_of(route):
    return [c for c, _ in route]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# name -> (builder, fill, forced starting class or None, expected classes tried (None: asserted only as "leaves the first class"),
#          (na, nt, ne, ns) maxima).  Threshold 0 everywhere.  The routes and maxima are what the model must reproduce.
ILUC_TABLE = {
    "arrow_last_33": (lambda: arrow_last(33), 5, None, [0], (2, 32, 33, 2)),
    "arrow_last_34": (lambda: arrow_last(34), 5, None, [0, 3], (2, 33, 34, 2)),
    "arrow_last_140": (lambda: arrow_last(140), 5, None, [0, 3], (2, 139, 140, 2)),
    "arrow_last_600": (lambda: arrow_last(600), 5, None, [0, 3, 4], (2, 599, 600, 2)),
    "row_first_128": (lambda: row_first(128, True), 5, None, [0], (128, 1, 128, 128)),
    "row_first_129": (lambda: row_first(129, True), 5, None, [0, 1], (129, 1, 129, 129)),
    "row_first_300": (lambda: row_first(300), 5, None, [0, 1, 2], (300, 1, 300, 300)),
    "row_first_600": (lambda: row_first(600, True), 5, None, [0, 1, 2, 4], (600, 1, 600, 600)),
    "comb_31_8_7": (lambda: comb(31, 8, 7), 10, None, [0], (9, 32, 256, 9)),
    "comb_32_8_0": (lambda: comb(32, 8, 0), 10, None, [0, 1], (9, 33, 257, 9)),
    "comb_63_12_11": (lambda: comb(63, 12, 11), 14, None, [1], (13, 64, 768, 13)),
    "comb_127_8_7": (lambda: comb(127, 8, 7), 30, None, [2], (9, 128, 1024, 9)),
    "comb_119_8_7": (lambda: comb(119, 8, 7), 10, None, [0, 3], (9, 120, 960, 9)),
}

# (on the capacity, one over): name -> (builder, fill, forced class or None, expected classes, which quantity, the capacity it sits on)
ILUC_TWINS = {
    "comb_31_8_8": (lambda: comb(31, 8, 8), 10, None, [0, 1], 2, 256),
    "comb_63_12_12": (lambda: comb(63, 12, 12), 14, None, [1, 2], 2, 768),
    "comb_127_8_8": (lambda: comb(127, 8, 8), 30, None, [2, 4], 2, 1024),
    "comb_119_8_8": (lambda: comb(119, 8, 8), 10, None, [0, 3, 4], 2, 960),
    "row_first_256": (lambda: row_first(256), 5, 1, [1], 0, 256),
    "row_first_257": (lambda: row_first(257), 5, 1, [1, 2], 0, 256),
    "row_first_256_c3": (lambda: row_first(256, True), 5, 3, [3], 0, 256),
    "row_first_257_c3": (lambda: row_first(257, True), 5, 3, [3, 4], 0, 256),
    "row_first_512": (lambda: row_first(512), 5, 2, [2], 0, 512),
    "row_first_513": (lambda: row_first(513), 5, 2, [2, 4], 0, 512),
    "arrow_last_65": (lambda: arrow_last(65), 5, 1, [1], 1, 64),
    "arrow_last_66": (lambda: arrow_last(66), 5, 1, [1, 3], 1, 64),
    "arrow_last_129": (lambda: arrow_last(129), 5, 2, [2], 1, 128),
    "arrow_last_130": (lambda: arrow_last(130), 5, 2, [2, 3], 1, 128),
    "arrow_last_513": (lambda: arrow_last(513), 5, None, [0, 3], 1, 512),
    "arrow_last_514": (lambda: arrow_last(514), 5, None, [0, 3, 4], 1, 512),
}
# the on-capacity cases of the table and the quantity / capacity they fill (their one-over twins: the next size, or e = t)
ON_CAPACITY = {"arrow_last_33": (1, 32, "arrow_last_34"), "row_first_128": (0, 128, "row_first_129"), "comb_31_8_7": (2, 256, "comb_31_8_8"),
               "comb_63_12_11": (2, 768, "comb_63_12_12"), "comb_127_8_7": (2, 1024, "comb_127_8_8"), "comb_119_8_7": (2, 960, "comb_119_8_8"),
               "row_first_256": (0, 256, "row_first_257"), "row_first_256_c3": (0, 256, "row_first_257_c3"), "row_first_512": (0, 512, "row_first_513"),
               "arrow_last_65": (1, 64, "arrow_last_66"), "arrow_last_129": (1, 128, "arrow_last_130"), "arrow_last_513": (1, 512, "arrow_last_514")}


def iluc_case(name):
    """(A, fill, forced class or None, expected classes) of a case of either table"""
    t = ILUC_TABLE.get(name) or ILUC_TWINS[name]
    return t[0](), t[1], t[2], t[3]


_model_cache = {}


def iluc_model(name, oracle, transposed=False):
    """(dem, deps, start, route) of a case, computed once: the oracle's factors of the view the kernel gets (A, or A^T for column input)"""
    key = (name, transposed)
    if key not in _model_cache:
        A, fill, forced, _ = iluc_case(name)
        V = (A.T if transposed else A).tocsr(); V.sort_indices()
        L, U = oracle.iluc(as_input(V), fill, 0.0)
        dem, deps = iluc_demands(V, L, U)
        start = forced if forced is not None else iluc_start(V.nnz, V.shape[0], fill)
        _model_cache[key] = (dem, deps, start, iluc_route(dem, deps, V.shape[0], start))
    return _model_cache[key]


def piluc_model(A, ml_oracle_level0, start=None):
    """(dem, deps, start, route) of one level of partial ILUC from the level's arrays as the multilevel oracle returns them"""
    A = sp.csr_matrix(A); A.sort_indices()
    dem, deps = iluc_demands(A, ml_oracle_level0["L"], ml_oracle_level0["U"], w_from_diagonal=True)
    if start is None:
        start = piluc_start(A.nnz, A.shape[0])
    return dem, deps, start, piluc_route(dem, deps, A.shape[0], start)
