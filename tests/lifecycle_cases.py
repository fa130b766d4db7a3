"""Cases, op model and sequence generator of the apply-state lifecycle tests (test_gpu_apply_lifecycle.py, test_lifecycle_cases.py).

One object lives through a SEQUENCE of operations.  The host layer (ilupp_amd/csrc/api.hip) keeps lazily built forms per object --
transposed static records, transposed storages with schedules and packed sweeps, four level-ordered copies, the LL^T pair, the armed
control words, the block buffers, the CSR value copy --, and a re-factorisation has to throw every copy of the OLD values away.  A stale
copy gives a plausible vector: the oracle's result for ANOTHER value set.  So a test holds K value sets on one pattern, and the expected
result of every operation is the oracle's for the CURRENT set; a mismatch is looked up among the other sets.

Nothing here touches the GPU: the matrices, value sets and right-hand sides, the oracle's factors and applies (cached per case and value
set, read-only), the expected result of an operation, and the sequences."""
import functools
import os

import numpy as np
import scipy.sparse as sp

import golden_util as G
import matgen

K_SETS = 3
POOL = 9                     # right-hand sides per case: column 0 = G.rhs(n), column 3 carries a NaN at row n // 3
NAN_COL = 3
B3_COLS = (0, 1, 3)          # the k = 3 block: two finite columns and the NaN column
BATCH_CAP_N = 16384          # cases up to this n take the batched launch (C, Ct); the GPU module asserts route 0 for them
SEQ_LEN = 12
MAX_R = 3

OPS = ("a", "t", "A", "T", "AA", "TA", "B3", "Bt3", "B9", "Bt9", "C", "Ct", "R", "F")

# the fixed sequences: each targets one state transition (the numbers are the issue's)
FIXED = {
    1: "t a",                                   # transposed first on a fresh object: the armed state construction leaves
    2: "t a R t a F",                           # transposed forms exist when the values change
    3: "R t a",                                 # re-factorisation before any apply has built anything
    4: "a t Bt9 B9 R B9 Bt9 t a",               # block state and the level copies of all four slots across R
    5: "AA TA R R TA AA",                       # applies in flight, two re-factorisations in a row
    6: "a C R C Ct t F",                        # a batched launch still reads the old factor when R starts; the CSR value copy after R
    7: "a t a t B3 a",                          # static, then generic sweeps: the work vector comes back all-sentinel each time
}


def _csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.data.astype(np.float64), A.indices.astype(np.int32), A.indptr.astype(np.int32)


def _tridiagonal_blocks():
    b = sp.csr_matrix(matgen.laplace1d(37), shape=(37, 37))
    return _csr(sp.block_diag([b] * 3000))


def _mesh_missing_upper():
    d, i, p = matgen.poisson3d(32)
    n = p.shape[0] - 1
    A = sp.csr_matrix((d, i, p), shape=(n, n)).tolil()
    for r in np.random.default_rng(11).integers(40, n - 40, size=300):
        if A[r, r + 32] != 0:
            A[r, r + 32] = 0                                  # some transposed entries are missing
    A = A.tocsr(); A.eliminate_zeros()
    return _csr(A)


def _lower_mesh():
    d, i, p = matgen.poisson3d(24, 24, 24)
    n = p.shape[0] - 1
    rng = np.random.default_rng(4)
    return _csr(sp.tril(sp.csr_matrix((d * (1.0 + 0.3 * rng.random(d.shape[0])), i, p), shape=(n, n))))


def _upwind_mesh(off, lo, hi):
    """the 32^3 mesh without the upper neighbour at distance `off` in the rows [lo, hi): there L^T has an offset that U's lanes do not"""
    d, i, p = matgen.poisson3d(32, 32, 32)
    n = p.shape[0] - 1
    rng = np.random.default_rng(4)
    A = sp.csr_matrix((d * (1.0 + 0.3 * rng.random(d.shape[0])), i, p), shape=(n, n)).tocoo()
    keep = ~((A.col == A.row + off) & (A.row >= lo) & (A.row < hi))
    return _csr(sp.csr_matrix((A.data[keep], (A.row[keep], A.col[keep])), shape=(n, n)))


def _arrow():
    n = 4000
    A = sp.lil_matrix((n, n)); A.setdiag(4.0); A[n - 1, :] = -0.001; A[:, n - 1] = -0.001; A[n - 1, n - 1] = 4.0
    return _csr(A)


def _short_l_long_u():
    """short L rows, long U rows: only one of the two sweeps has a level-major form"""
    n = 6000
    rng = np.random.default_rng(3)
    rows, cols, vals = [], [], []
    for r in range(n):
        cs = {r}
        if r > 0: cs.add(r - 1)
        if r > 70: cs.add(r - 64)
        for c in rng.integers(r + 1, min(n, r + 400), size=6) if r + 1 < n else []:
            cs.add(int(c))
        for c in sorted(cs):
            rows.append(r); cols.append(c); vals.append(20.0 if c == r else -rng.random())
    return _csr(sp.csr_matrix((vals, (rows, cols)), shape=(n, n)))


def _ichol0_scaled(nx, ny, nz):
    d, i, p = matgen.poisson3d(nx, ny, nz)
    n = p.shape[0] - 1
    D = sp.diags(1.0 + 0.5 * np.random.default_rng(7).random(n))          # symmetric scaling: stays positive definite
    return _csr(D @ sp.csr_matrix((d, i, p), shape=(n, n)) @ D)


def _box27_symmetric():
    d, i, p = matgen.box_stencil((13, 13, 13))
    n = p.shape[0] - 1
    A = sp.csr_matrix((d, i, p), shape=(n, n))
    return _csr((A + A.T) * 0.5)


def _wv(names, vecwave):
    """box grid: the wave-exchange factor kernel; vector-wave sweeps, or k_sptrsv_wx on the level-major copies without them"""
    if not (len(names) == 3 and names[0].startswith("k_ilu0_wa<")):
        return False
    if vecwave:
        return names[1].startswith("k_sptrsv_wv<1, ") and names[2].startswith("k_sptrsv_wv<-1, ")
    return names[1:] == ("k_sptrsv_wx<1, false>", "k_sptrsv_wx<-1, true>")


_SD = ("k_ilu0_sd", "k_sptrsv_st<1, false>", "k_sptrsv_st<-1, false>")
_ST = ("k_ilu0_st", "k_sptrsv_st<1, false>", "k_sptrsv_st<-1, false>")
_PAIR_SWEEPS = (("k_sptrsv_wv<1, true>", "k_sptrsv_wv<-1, true, true>"), ("k_sptrsv_wx<1, true>", "k_sptrsv_wx<-1, true, true>"),
                ("k_sptrsv_st<1, true>", "k_sptrsv_st<-1, true>"))


class Case:
    """name; kind and params of the constructor; n (declared, so that collecting the tests builds no matrix) and the matrix; the path the object must report, a predicate on kernel_names() (after the
    first apply for the LL^T kinds, whose pair is analysed there), the block route for k >= 2; whether the kind has a re-factorisation;
    batch: the object is member 0 of a batched first construction (member 1 is the twin of its batched applies)."""

    def __init__(self, name, kind, n, make, path, kernels, block, params=None, batch=False):
        self.name, self.kind, self.n, self.make, self.path, self.kernels, self.block = name, kind, n, make, path, kernels, block
        self.params = params or {}
        self.batch = batch
        self.refactor = kind == "ILU0"

    def __repr__(self):
        return self.name

    @functools.cached_property
    def matrix(self):
        """(v0, indices, indptr), read-only"""
        out = tuple(np.ascontiguousarray(a) for a in self.make())
        for a in out:
            a.setflags(write=False)
        assert out[2].shape[0] - 1 == self.n, (self.name, out[2].shape[0] - 1)
        return out

    @property
    def sets(self):
        """how many value sets the case uses: K for the kinds with a re-factorisation, else the given one alone"""
        return K_SETS if self.refactor else 1

    @property
    def small(self):
        return self.n <= BATCH_CAP_N

    @functools.cached_property
    def alphabet(self):
        return tuple(t for t in OPS if (t != "R" or self.refactor) and (t not in ("C", "Ct") or self.small))


CASES = [
    Case("box24x30x20", "ILU0", 14400, lambda: matgen.poisson3d(24, 30, 20), "ilu0:static-direct", _wv, "block:columns"),
    Case("tridiagonal_blocks", "ILU0", 111000, _tridiagonal_blocks, "ilu0:static-direct", lambda nm, v: nm == _SD, "block:columns"),
    Case("mesh32_missing_upper", "ILU0", 32768, _mesh_missing_upper, "ilu0:static-level-major", lambda nm, v: nm == _ST, "block:columns"),
    # the lower triangle of a mesh (U is the diagonal alone): the static form declines it, CSR program and packed sweeps
    Case("lower_mesh24", "ILU0", 13824, _lower_mesh, "ilu0:csr-program", lambda nm, v: nm == (), "block:columns"),
    # upwind stencils: static sweeps for apply, but L^T has an offset that U's lanes do not -- the transposed records are declined
    # (no_static_T) and apply_trans runs the generic sweeps, which use the work vector as their ready flags (work_clean); the first has
    # the wave-exchange sweeps whose apply is armed ahead (ctrl_armed), the second the sweeps of the static form's first generation
    Case("upwind_z_slab32", "ILU0", 32768, lambda: _upwind_mesh(1024, 8 * 1024, 16 * 1024), "ilu0:static-direct",
         lambda nm, v: nm == ("k_ilu0_sd", "k_sptrsv_wv<1, false>", "k_sptrsv_wv<-1, true>"), "block:columns"),
    Case("upwind_y32", "ILU0", 32768, lambda: _upwind_mesh(32, 0, 32768), "ilu0:static-direct", lambda nm, v: nm == _SD, "block:columns"),
    Case("ninepoint40x40", "ILU0", 1600, lambda: matgen.box_stencil((40, 40)), "ilu0:level-order", lambda nm, v: nm == (), "block:level"),
    Case("mesh20", "ILU0", 8000, lambda: matgen.poisson3d(20), "ilu0:csr-program", lambda nm, v: nm == (), "block:columns"),
    Case("arrow4000", "ILU0", 4000, _arrow, "ilu0:csr", lambda nm, v: nm == (), "block:columns"),
    Case("short_L_long_U", "ILU0", 6000, _short_l_long_u, "ilu0:level-order", lambda nm, v: nm == (), "block:level"),
    Case("batch_member", "ILU0", 210, lambda: matgen.poisson2d(15, 14), "ilu0:batch", lambda nm, v: nm == (), "block:columns", batch=True),
    Case("ichol0_pair", "IChol0", 36465, lambda: _ichol0_scaled(17, 33, 65), "ichol0:static-level-major",
         lambda nm, v: nm[0] == "k_ichol0_st" and nm[1:] in _PAIR_SWEEPS, "block:columns"),
    # (64 x 24 x 16: the static factor kernel and the pair both decline -- chain kernel, packed sweeps)
    Case("ichol0_declined", "IChol0", 24576, lambda: _ichol0_scaled(64, 24, 16), "ichol0", lambda nm, v: nm == ("k_ichol0",), "block:columns"),
    Case("ichol0_chain", "IChol0", 2197, _box27_symmetric, "ichol0", lambda nm, v: nm == ("k_ichol0",), "block:level"),
    Case("icholt_grid", "ICholT", 66000, lambda: matgen.poisson3d(33, 50, 40), "icholt:grid-static",
         lambda nm, v: nm[0] == "k_icholt_grid" and len(nm) == 3, "block:columns", params={"add_fill_in": 0, "threshold": 0.0}),
    Case("icholt5", "ICholT", 2744, lambda: matgen.poisson3d(14), "icholt", lambda nm, v: nm == ("k_icholt_df",), "block:level",
         params={"add_fill_in": 5, "threshold": 1e-3}),
    Case("ilut", "ILUT", 8000, lambda: matgen.poisson3d(20), "ilut", lambda nm, v: nm == (), "block:level", params={"fill_in": 10, "threshold": 1e-4}),
    Case("iluc", "ILUC", 8000, lambda: matgen.poisson3d(20), "iluc", lambda nm, v: nm == (), "block:level", params={"fill_in": 8, "threshold": 1e-2}),
]
BY_NAME = {c.name: c for c in CASES}


def twin_matrix():
    """the small second member of the batched applies (and of the batched construction of the batch-built case)"""
    d, i, p = matgen.poisson2d(12)
    return d * (1.0 + 0.25 * np.random.default_rng(21).random(d.shape[0])), i, p


@functools.lru_cache(maxsize=None)
def values(case, k):
    """value set k on the case's pattern: v0 as given, v_k = v0 * (1 + 0.25 * rng_k.random(nnz))"""
    assert 0 <= k < case.sets
    v0 = case.matrix[0]
    v = v0 if k == 0 else v0 * (1.0 + 0.25 * np.random.default_rng(7000 + k).random(v0.shape[0]))
    v = np.ascontiguousarray(v)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def rhs_pool(n):
    """(n, POOL): column 0 = G.rhs(n), the others random; column NAN_COL has a NaN at row n // 3 (its canonical NaNs must come out where
    the oracle puts them)"""
    X = np.random.default_rng(3).standard_normal((n, POOL))
    X[:, 0] = G.rhs(n)
    X[n // 3, NAN_COL] = np.nan
    X.setflags(write=False)
    return X


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _libs():
    from oracle import oracle as O
    return O, (O.ref() if O.ref_available() else O.orc())


def _factorise(kind, params, M):
    O, fac = _libs()
    if kind == "ILU0":
        return fac.ilu0(M)
    if kind == "ILUT":
        return fac.ilut(M, params["fill_in"], params["threshold"])
    if kind == "ILUC":
        return fac.iluc(M, params["fill_in"], params["threshold"])
    if kind == "IChol0":
        return (fac.ichol0(M),)
    return (fac.icholt(M, params["add_fill_in"], params["threshold"]),)


def _apply_columns(kind, F, X):
    O, _ = _libs()
    orc = O.orc()
    if kind in ("IChol0", "ICholT"):
        ap = lambda x, use: orc.apply_llt(F[0], x, use)
    else:
        ap = lambda x, use: orc.apply_lu(F[0], F[1], x, use)
    out = []
    for use in (O.ID, O.TRANSPOSE):
        Y = np.column_stack([ap(X[:, j], use) for j in range(X.shape[1])])
        Y.setflags(write=False)
        out.append(Y)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_factors(case, k):
    """the oracle's factorisation of value set k: a tuple of (data, indices, indptr, is_csr)"""
    _, i, p = case.matrix
    return tuple(_factorise(case.kind, case.params, (values(case, k), i, p, True)))


@functools.lru_cache(maxsize=None)
def oracle_columns(case, k):
    """the oracle's apply of every column of the pool on the factors of value set k: ((n, POOL) plain, (n, POOL) transposed), read-only"""
    return _apply_columns(case.kind, oracle_factors(case, k), rhs_pool(case.n))


@functools.lru_cache(maxsize=None)
def twin_columns():
    d, i, p = twin_matrix()
    n = p.shape[0] - 1
    return _apply_columns("ILU0", _factorise("ILU0", {}, (d, i, p, True)), G.rhs(n)[:, None])


def expected(case, k, op):
    """What operation `op` returns on an object that holds value set k -- a function of (case, k, op) alone, whatever ran before.  A list
    of arrays in the order the operation produces them: vectors for the applies, one (n, k) block for B*, the twin's vector last for
    C / Ct, the factors' value arrays for F, nothing for R."""
    if op == "R":
        return []
    if op == "F":
        return [f[0] for f in oracle_factors(case, k)]
    plain, trans = oracle_columns(case, k)
    if op in ("a", "t"):
        return [(plain if op == "a" else trans)[:, 0]]
    if op in ("A", "T"):
        return [(plain if op == "A" else trans)[:, 1]]
    if op in ("AA", "TA"):
        return [(plain if op == "AA" else trans)[:, 1], plain[:, 2]]
    if op in ("B9", "Bt9"):
        return [plain if op == "B9" else trans]
    if op in ("B3", "Bt3"):
        return [(plain if op == "B3" else trans)[:, B3_COLS]]
    if op in ("C", "Ct"):
        tw = twin_columns()
        return [(plain if op == "C" else trans)[:, 2], (tw[0] if op == "C" else tw[1])[:, 0]]
    raise ValueError("unknown operation %r" % (op,))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def diagnose(case, k, op, idx, got):
    """which OTHER value set's expected result `got` equals (the signature of a stale copy, and which one), in words"""
    for j in range(case.sets):
        if j != k and same_bits(np.asarray(got), expected(case, j, op)[idx]):
            return "equals the result under value set %d: a stale copy of v%d" % (j, j)
    return "equals the result under no other value set"


class Model:
    """the value set an object holds after a sequence of operations: R moves to the next one (cyclically), nothing else changes it"""

    def __init__(self, case):
        self.case, self.cur = case, 0

    def step(self, op):
        """advance over `op`; returns the expected results of the operation (of the NEW set for R: nothing)"""
        if op == "R":
            assert self.case.refactor
            self.cur = (self.cur + 1) % self.case.sets
        return expected(self.case, self.cur, op)


def parse(seq):
    toks = tuple(seq.split()) if isinstance(seq, str) else tuple(seq)
    for t in toks:
        if t not in OPS:
            raise ValueError("unknown operation %r" % (t,))
    return toks


def fixed_sequences(case):
    """{number: tokens} of the fixed sequences the case runs: operations it does not have are skipped (R elsewhere than ILU(0)), number 6
    runs below the batched cap only, and a sequence that becomes equal to an earlier one is left out"""
    out, seen = {}, set()
    for num, seq in FIXED.items():
        if num == 6 and not case.small:
            continue
        toks = tuple(t for t in parse(seq) if t in case.alphabet)
        if toks and toks not in seen:
            seen.add(toks)
            out[num] = toks
    return out


def fuzz_offset():
    return int(os.environ.get("ILUPP_FUZZ_OFFSET", "0"))


def random_sequence(alphabet, seed, length=SEQ_LEN, max_r=MAX_R):
    """`length` operations drawn from `alphabet`, at most `max_r` of them R; a function of its arguments alone"""
    alphabet = tuple(alphabet)
    rng = np.random.default_rng(seed)
    rest = tuple(t for t in alphabet if t != "R")
    alphabet = rest + ("R",) * (3 if "R" in alphabet else 0)      # (R three times as likely as any other: it is what makes copies stale)
    out = []
    for _ in range(length):
        pick = alphabet if out.count("R") < max_r else rest
        out.append(pick[int(rng.integers(len(pick)))])
    return tuple(out)


def random_sequences(case, count=2):
    """the case's seeded sequences; ILUPP_FUZZ_OFFSET shifts the seeds"""
    base = 9100 + 16 * CASES.index(case) + fuzz_offset()
    return [random_sequence(case.alphabet, base + j) for j in range(count)]
