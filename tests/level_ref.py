"""A plain CPU model of what the level-order family (ilupp_amd/csrc/sptrsv_lvl.hip, ilu0_lvl.hip, sptrsm_lvl.hip) must compute before a
sweep runs: the level of every row, the order of the rows, and the constants the host code derives from them.  numpy / scipy only.

The contract (DESIGN_OTHER_PATHS, "level order"):
  level(r) = 0 for a row without STORED off-diagonal entry (an explicit zero is a dependency), else 1 + max level(c) over them:
             levels are minimal;
  perm     = the rows sorted by (level, row): ties by row (the device's stable radix sort of the levels);
  nlevels  = max level + 1.
`levels` computes it by frontiers (Kahn's rounds), `levels_by_relaxation` by repeated whole-vector relaxation to a fixed point: two
methods that share nothing but the edge list.

The thresholds of lvl_order / lvl_build / csr_and_level_fallbacks are RESTATED here (not imported), so that a threshold that drifts in
the code fails a test.  The matrices of the family's tests are built here as well (tests/test_level_ref.py asserts the figures that put
each one on its route)."""
import functools

import numpy as np
import scipy.sparse as sp

import matgen

# what ilupp_hip_debug_level_order's info[3] and info[6] say
GIVEN, NATURAL, RELAXED, GIVEN_UP = 0, 1, 2, 3
ROUTE_STATIC, ROUTE_LEVEL_MAJOR, ROUTE_LEVEL_ORDER, ROUTE_ROWS, ROUTE_ROWS_DEGENERATE, ROUTE_DESCRIPTORS, ROUTE_GENERIC = 1, 2, 3, 4, 5, 6, 7


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def _edges(T):
    """(n, rows, cols) of the stored off-diagonal entries of T in CSR order -- the pattern, explicit zeros included"""
    T = T if sp.isspmatrix_csr(T) else T.tocsr()
    n = T.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(T.indptr))
    cols = T.indices.astype(np.int64)
    keep = rows != cols
    return n, rows[keep], cols[keep]


def _result(level):
    perm = np.argsort(level, kind="stable").astype(np.int32)
    return level, perm, int(level.max()) + 1


def levels(T):
    """(level, perm, nlevels) of the triangular matrix a sweep solves with (lower for a forward sweep, upper for a backward one).
    Frontier by frontier: a row joins the round after the last row it reads has joined."""
    n, rows, cols = _edges(T)
    waiting = np.bincount(rows, minlength=n)                   # entries of a row whose column has no level yet
    order = np.argsort(cols, kind="stable")                    # the readers of every column
    readers = rows[order]
    rptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=rptr[1:])
    level = np.zeros(n, dtype=np.int64)
    frontier = np.flatnonzero(waiting == 0)
    numbered, cur = frontier.shape[0], 0
    while frontier.shape[0]:
        lo, cnt = rptr[frontier], rptr[frontier + 1] - rptr[frontier]
        tot = int(cnt.sum())
        if tot == 0:
            break
        first = np.cumsum(cnt) - cnt
        hit, times = np.unique(readers[np.repeat(lo - first, cnt) + np.arange(tot)], return_counts=True)
        waiting[hit] -= times
        frontier = hit[waiting[hit] == 0]
        cur += 1
        level[frontier] = cur
        numbered += frontier.shape[0]
    assert numbered == n, "the pattern is not triangular (a cycle)"
    return _result(level)


def levels_by_relaxation(T):
    """the same numbers by another method: every row at once takes 1 + max over the rows it reads, from all-zero until nothing changes
    (the operator is monotone, so the fixed point reached from zero is the least one: the minimal levels)"""
    n, rows, cols = _edges(T)
    level = np.zeros(n, dtype=np.int64)
    if rows.shape[0]:
        starts = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
        heads = rows[starts]
        for _ in range(n + 1):
            new = np.zeros(n, dtype=np.int64)
            new[heads] = np.maximum.reduceat(level[cols] + 1, starts)
            if np.array_equal(new, level):
                break
            level = new
        else:
            raise AssertionError("the pattern is not triangular (a cycle)")
    return _result(level)


def lower_part(A):
    """the strictly-lower part of A plus the diagonal, as stored: the dependencies of the ILU(0) rows (the factor order, mode 2)"""
    A = A if sp.isspmatrix_csr(A) else A.tocsr()
    n = A.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr))
    keep = A.indices <= rows
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=ptr[1:])
    return sp.csr_matrix((A.data[keep], A.indices[keep], ptr), shape=A.shape)


# ---- which triangle a slot holds -----------------------------------------------------------------------------------------------------
# slots: 0 = Lc, 1 = Uc, 2 = UcT, 3 = LcT (sweep_parts in api.hip).  For every class and `transpose` the two sweeps of an apply
# (apply_plan in api.hip) as (slot, the matrix the sweep solves with), first the forward sweep.  L and U are the matrices P.factors()
# returns (A ~ L U, or L L^T).
def plan(cls, L, U, csr_input, transpose):
    """cls: "lu" (ILU(0), ILUT), "iluc", "ichol0", "icholt"; returns [(slot, T forward), (slot, T backward)]"""
    if cls == "lu":
        mats = (L.T, U.T)[::-1] if transpose else (L, U)                 # ID: L then U; TRANSPOSE: U^T then L^T
        slots = (0, 1) if transpose == (not csr_input) else (2, 3)       # (CSC input: factors of the row-major view A^T, ID and TRANSPOSE swap)
        return [(slots[0], mats[0]), (slots[1], mats[1])]
    if cls == "iluc":
        return [(2, U.T), (0, L.T)] if transpose else [(3, L), (1, U)]
    if cls == "ichol0":
        return [(0, L), (3, L.T)]
    if cls == "icholt":
        return [(3, L), (0, L.T)]
    raise ValueError(cls)


# ---- the constants the host code derives (restated) ----------------------------------------------------------------------------------
def window(per_row):
    return 4 if per_row <= 4.5 else (8 if per_row <= 8.5 else 16)


def offdiag_per_row(T):
    return T.nnz / T.shape[0] - 1.0


def factor_per_row(A):
    """the part left of the diagonal of a general matrix: half of its off-diagonal entries"""
    return 0.5 * (A.nnz / A.shape[0] - 1.0)


def sweep_block(n, nlevels):
    return 256 if n // nlevels < 4096 else 1024


def reach(T, upper):
    """the farthest dependency of any row, rows sorted by column: the first entry of a lower part, the last of an upper one"""
    T = T if sp.isspmatrix_csr(T) else T.tocsr()
    T = T.copy(); T.sort_indices()
    ne = np.flatnonzero(np.diff(T.indptr) > 0)
    if ne.shape[0] == 0:
        return 0
    d = T.indices[T.indptr[ne + 1] - 1] - ne if upper else ne - T.indices[T.indptr[ne]]
    return max(int(d.max()), 0)


def relaxation_eligible(per_row, n, rch):
    return per_row <= 4.5 and n >= 65536 and rch > 0 and 3.0 * n / rch <= 1024.0


def expected_slot(T, upper, given=False):
    """what ilupp_hip_debug_level_order must report for a slot that holds T: perm, and info[0 .. 3] and [5]"""
    level, perm, nlevels = levels(T)
    n = T.shape[0]
    per_row = offdiag_per_row(T)
    how = GIVEN if given else (RELAXED if relaxation_eligible(per_row, n, reach(T, upper)) else NATURAL)
    return {"perm": perm, "nlevels": nlevels, "w": window(per_row), "block": sweep_block(n, nlevels), "how": how,
            "natural_w": window(per_row) if how == NATURAL else 0}


def expected_factor_order(A):
    """... and for the factor order (which = 4) of an "ilu0:level-order" object made from the row-major matrix A"""
    T = lower_part(A)
    level, perm, nlevels = levels(T)
    per_row = factor_per_row(A)
    how = RELAXED if relaxation_eligible(per_row, A.shape[0], reach(A, False)) else NATURAL
    return {"perm": perm, "nlevels": nlevels, "how": how, "natural_w": window(per_row) if how == NATURAL else 0}


def by_level(A, nlevels):
    """csr_and_level_fallbacks: does ILU(0) of the row-major matrix A run in level order?  (long rows always; short rows when the levels
    are deep and wide)"""
    n = A.shape[0]
    if n < 1024 or int(np.diff(A.indptr).max()) > 64:
        return False
    return A.nnz > 8 * n or (nlevels > 64 and n // nlevels >= 256)


# ---- the matrices --------------------------------------------------------------------------------------------------------------------
def unsym(d, seed):
    """values that are neither symmetric nor constant (the pattern stays)"""
    return d * (1.0 + 0.25 * np.random.default_rng(seed).random(d.shape[0]))


def _csr(d, i, p):
    n = p.shape[0] - 1
    return sp.csr_matrix((d, i, p), shape=(n, n))


def _stencil(dip, seed):
    """a matgen matrix (data, indices, indptr) with `unsym` values, as scipy CSR"""
    d, i, p = dip
    return _csr(unsym(d, seed), i, p)


def dense_blocks(bs, nblocks, seed=17):
    """block-diagonal, every block dense bs x bs and diagonally dominant by rows: ILU(0) is a full LU of every block, row k of a block has
    k pivots and level k"""
    n = bs * nblocks
    rng = np.random.default_rng(seed)
    base = (np.arange(n, dtype=np.int64) // bs) * bs
    cols = (base[:, None] + np.arange(bs, dtype=np.int64)[None, :]).astype(np.int32)
    vals = -(0.25 + 0.75 * rng.random((n, bs)))
    vals[np.arange(n), np.arange(n) % bs] = bs + rng.random(n)
    return sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(n + 1, dtype=np.int32) * bs), shape=(n, n))


COUNTS_K = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63)


def counts_matrix(n=4096, seed=23):
    """lower triangular (U of its ILU(0) is the diagonal alone): row r has COUNTS_K[r % 15] entries left of the diagonal (fewer only where
    r itself is smaller), half of them 128 .. 255 rows back -- near enough to land in the reader's workgroup of the level-ordered sweep,
    far enough that the levels stay few --, the other half anywhere before that"""
    rng = np.random.default_rng(seed)
    ptr = np.zeros(n + 1, dtype=np.int32)
    cols, vals = [], []
    for r in range(n):
        k = min(COUNTS_K[r % len(COUNTS_K)], r)
        if r < 512:
            c = rng.choice(r, size=k, replace=False) if k else np.zeros(0, dtype=np.int64)
        else:
            near = rng.choice(np.arange(r - 255, r - 127), size=(k + 1) // 2, replace=False)
            far = rng.choice(r - 255, size=k // 2, replace=False)
            c = np.concatenate([near, far])
        c = np.sort(c).astype(np.int32)
        cols.append(c); cols.append(np.array([r], dtype=np.int32))
        vals.append(-(0.25 + 0.75 * rng.random(k))); vals.append(np.array([k + 1.0 + rng.random()]))
        ptr[r + 1] = ptr[r] + k + 1
    return sp.csr_matrix((np.concatenate(vals), np.concatenate(cols), ptr), shape=(n, n))


def _sym(dims):
    """the symmetrised box stencil for the LL^T classes: values not constant, the diagonal raised so that the matrix stays definite"""
    d, i, p = matgen.box_stencil(dims)
    A = _csr(*matgen.symmetrize(unsym(d, 13), i, p))
    return (A + sp.diags(0.5 * A.diagonal())).tocsr()


_BUILDERS = {
    "holes42": lambda: _stencil(matgen.mesh_with_holes(42), 5),
    "nine256": lambda: _stencil(matgen.box_stencil((256, 257)), 6),
    "box27_41": lambda: _stencil(matgen.box_stencil((41, 41, 41)), 7),
    "nine48": lambda: _stencil(matgen.box_stencil((48, 48)), 8),
    "nine3x700": lambda: _stencil(matgen.box_stencil((3, 700)), 9),
    "nine200x7": lambda: _stencil(matgen.box_stencil((200, 7)), 10),
    "nine8x300": lambda: _stencil(matgen.box_stencil((8, 300)), 12),
    "box27_3x26x27": lambda: _stencil(matgen.box_stencil((3, 26, 27)), 11),
    "dense64x16": lambda: dense_blocks(64, 16),
    "dense9": lambda: dense_blocks(9, 4104),
    "dense14": lambda: dense_blocks(14, 4200),
    "dense24": lambda: dense_blocks(24, 4104),
    "dense14_small": lambda: dense_blocks(14, 100),
    "counts": counts_matrix,
    "below_floor": lambda: dense_blocks(64, 16)[:1023][:, :1023].tocsr(),
    "sym_nine48": lambda: _sym((48, 48)),
    "sym_box27_13": lambda: _sym((13, 13, 13)),
}
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """the named matrix in CSR with sorted int32 indices; shared, so nobody writes into it"""
    A = _BUILDERS[name]().tocsr()
    A.sort_indices()
    A = sp.csr_matrix((A.data.astype(np.float64), A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)
    for a in (A.data, A.indices, A.indptr):
        a.setflags(write=False)
    return A
