"""The CPU model of the level numbering (tests/level_ref.py) checked against closed forms, against a second method and against a plain
row loop, and the figures that put every matrix of the level-order tests (tests/test_gpu_level_order.py) on its route: a generator that
changes cannot quietly move a case off the kernel instantiation it is there for.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import level_ref as R
import matgen


def _csr(dip):
    d, i, p = dip
    n = p.shape[0] - 1
    return sp.csr_matrix((d, i, p), shape=(n, n))


def _upper_part(A):
    return R.lower_part(A.T.tocsr()).T.tocsr()


def _row_loop(T):
    """the definition, row by row (lower triangular patterns only)"""
    T = T.tocsr()
    level = np.zeros(T.shape[0], dtype=np.int64)
    for r in range(T.shape[0]):
        for c in T.indices[T.indptr[r]:T.indptr[r + 1]]:
            if c != r:
                assert c < r
                level[r] = max(level[r], level[c] + 1)
    return level


def _both(T):
    a, b = R.levels(T), R.levels_by_relaxation(T)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    return a


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def test_seven_point_box_levels_are_x_plus_y_plus_z():
    nx, ny, nz = 6, 5, 4
    A = _csr(matgen.poisson3d(nx, ny, nz))
    r = np.arange(nx * ny * nz)
    want = r % nx + (r // nx) % ny + r // (nx * ny)
    level, perm, nlevels = _both(R.lower_part(A))
    assert np.array_equal(level, want) and nlevels == nx + ny + nz - 2
    level, perm, nlevels = _both(_upper_part(A))
    assert np.array_equal(level, (nx + ny + nz - 3) - want) and nlevels == nx + ny + nz - 2


def test_chain_diagonal_and_order():
    n = 300
    level, perm, nlevels = _both(R.lower_part(_csr(matgen.laplace1d(n))))
    assert nlevels == n and np.array_equal(level, np.arange(n)) and np.array_equal(perm, np.arange(n))
    level, perm, nlevels = _both(_upper_part(_csr(matgen.laplace1d(n))))
    assert nlevels == n and np.array_equal(perm, np.arange(n)[::-1])
    level, perm, nlevels = _both(sp.identity(50, format="csr"))
    assert nlevels == 1 and not level.any() and np.array_equal(perm, np.arange(50))
    # ties by row: rows 0, 2, 3 have no dependency, rows 1 and 4 read row 0, row 5 reads row 4
    T = sp.csr_matrix((np.ones(9), np.array([0, 0, 1, 2, 3, 0, 4, 4, 5]), np.array([0, 1, 3, 4, 5, 7, 9])), shape=(6, 6))
    level, perm, nlevels = _both(T)
    assert level.tolist() == [0, 1, 0, 0, 1, 2] and perm.tolist() == [0, 2, 3, 1, 4, 5] and nlevels == 3
    assert perm.dtype == np.int32


def test_an_explicit_zero_is_a_dependency():
    T = sp.csr_matrix((np.array([1.0, 0.0, 1.0, 0.0, 1.0]), np.array([0, 0, 1, 1, 2]), np.array([0, 1, 3, 5])), shape=(3, 3))
    assert T.nnz == 5
    for Tm in (T, T.tocsc()):
        level, perm, nlevels = _both(Tm)
        assert level.tolist() == [0, 1, 2] and nlevels == 3
    level, perm, nlevels = _both(T.T)                 # (upper: row 2 is the free one)
    assert level.tolist() == [2, 1, 0] and perm.tolist() == [2, 1, 0]


def test_a_cycle_is_refused():
    T = sp.csr_matrix(np.array([[1.0, 1.0], [1.0, 1.0]]))
    with pytest.raises(AssertionError):
        R.levels(T)
    with pytest.raises(AssertionError):
        R.levels_by_relaxation(T)


@pytest.mark.parametrize("seed", range(6))
def test_random_dags_three_methods_agree(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(40, 400))
    k = int(rng.integers(1, 12))
    rows = np.repeat(np.arange(1, n), k)
    cols = (rng.random(rows.shape[0]) * rows).astype(np.int64)             # any earlier row
    if seed % 2:
        cols = np.maximum(rows - 1 - (rng.random(rows.shape[0]) * 5).astype(np.int64), 0)      # a band: deep chains
    T = sp.coo_matrix((np.ones(rows.shape[0]), (rows, cols)), shape=(n, n)).tocsr() + sp.identity(n, format="csr")
    level, perm, nlevels = _both(T)
    assert np.array_equal(level, _row_loop(T))
    assert np.array_equal(perm, np.lexsort((np.arange(n), level)))
    lu, pu, nu = _both(T.T.tocsr())
    assert nu == nlevels                                # (the longest path is the same one, walked from the other end)
    # (the upper matrix with rows and columns reversed is a lower one: row r there is row n - 1 - r here)
    assert np.array_equal(lu, _row_loop(T.T.tocsr()[::-1][:, ::-1])[::-1]) and np.array_equal(pu, np.lexsort((np.arange(n), lu)))


# ---- the apply plan and the restated thresholds --------------------------------------------------------------------------------------
def test_plan_matches_the_table():
    L = sp.csr_matrix(np.tril(np.arange(1.0, 10.0).reshape(3, 3)))
    U = sp.csr_matrix(np.triu(np.arange(1.0, 10.0).reshape(3, 3)))
    same = lambda got, want: [s for s, _ in got] == [s for s, _ in want] and all((a != b).nnz == 0 for (_, a), (_, b) in zip(got, want))
    assert same(R.plan("lu", L, U, True, False), [(0, L), (1, U)])
    assert same(R.plan("lu", L, U, True, True), [(2, U.T), (3, L.T)])
    assert same(R.plan("lu", L, U, False, False), [(2, L), (3, U)])           # (CSC input: the slots of ID and TRANSPOSE swap)
    assert same(R.plan("lu", L, U, False, True), [(0, U.T), (1, L.T)])
    assert same(R.plan("iluc", L, U, True, False), [(3, L), (1, U)])
    assert same(R.plan("iluc", L, U, True, True), [(2, U.T), (0, L.T)])
    for tr in (False, True):
        assert same(R.plan("ichol0", L, None, True, tr), [(0, L), (3, L.T)])
        assert same(R.plan("icholt", L, None, True, tr), [(3, L), (0, L.T)])


def test_thresholds_as_the_code_states_them():
    assert [R.window(x) for x in (0.0, 4.5, 4.51, 8.5, 8.51, 31.5)] == [4, 4, 8, 8, 16, 16]
    assert R.sweep_block(4095 * 7 + 6, 7) == 256 and R.sweep_block(4096 * 7, 7) == 1024 and R.sweep_block(4096, 1) == 1024
    assert R.relaxation_eligible(4.5, 65536, 192) and not R.relaxation_eligible(4.51, 65536, 192)
    assert not R.relaxation_eligible(4.0, 65535, 192) and not R.relaxation_eligible(4.0, 65536, 191) and not R.relaxation_eligible(4.0, 65536, 0)


# ---- the matrices: both methods agree, and the figures that decide the route ---------------------------------------------------------
@pytest.fixture(scope="module")
def figures():
    out = {}
    for name in R.NAMES:
        A = R.matrix(name)
        lo, up = R.lower_part(A), _upper_part(A)
        out[name] = {"A": A, "lo": lo, "up": up, "lower": _both(lo), "upper": _both(up)}
    return out


@pytest.mark.parametrize("name", R.NAMES)
def test_values_are_neither_symmetric_nor_constant(name):
    A = R.matrix(name)
    assert np.unique(A.data).shape[0] > A.shape[0]
    if not name.startswith("sym_") and name != "counts":
        assert abs(A - A.T).max() > 1e-3
    assert (np.abs(A.diagonal()) > 0).all()
    with pytest.raises(ValueError):
        A.data[0] = 0.0                                 # shared between tests: read-only


def test_holes42(figures):
    f = figures["holes42"]; A = f["A"]; n = A.shape[0]
    assert n == 71766 and round(R.factor_per_row(A), 2) == 2.84 and R.reach(A, False) == 1731 and int(3 * n / 1731) == 124
    assert f["lower"][2] == 124 and f["upper"][2] == 124 and round(n / 124) == 579 and R.by_level(A, 124)
    assert R.expected_factor_order(A)["how"] == R.RELAXED
    # ILU(0) has A's pattern: U, U^T and L^T are numbered by relaxation as well (L takes the factor order)
    for T, upper in ((f["up"], True), (f["up"].T.tocsr(), False), (f["lo"].T.tocsr(), True)):
        e = R.expected_slot(T, upper)
        assert (e["how"], e["w"], e["block"], e["nlevels"]) == (R.RELAXED, 4, 256, 124)


def test_nine256(figures):
    f = figures["nine256"]; A = f["A"]; n = A.shape[0]
    assert n == 65792 and round(A.nnz / n, 2) == 8.95 and A.nnz > 8 * n and round(R.factor_per_row(A), 2) == 3.98
    assert R.reach(A, False) == 257 and 3.0 * n / 257 == 768.0
    assert f["lower"][2] == 768 and R.by_level(A, 768) and R.expected_factor_order(A)["how"] == R.RELAXED
    e = R.expected_slot(f["lo"], False, given=True)
    assert (e["how"], e["w"], e["block"]) == (R.GIVEN, 4, 256) and R.offdiag_per_row(f["lo"]) <= 4.0
    assert R.expected_slot(f["up"], True)["how"] == R.RELAXED


def test_box27_41(figures):
    f = figures["box27_41"]; A = f["A"]; n = A.shape[0]
    assert n == 68921 and round(R.factor_per_row(A), 2) == 12.35 and f["lower"][2] == 281
    e = R.expected_factor_order(A)
    assert (e["how"], e["natural_w"]) == (R.NATURAL, 16) and R.by_level(A, 281)
    e = R.expected_slot(f["up"], True)
    assert (e["how"], e["natural_w"], e["w"], e["block"]) == (R.NATURAL, 16, 16, 256)


@pytest.mark.parametrize("name,dims,n,level_order", [("nine48", (48, 48), 2304, True), ("nine3x700", (3, 700), 2100, False),
                                                     ("nine200x7", (200, 7), 1400, True)])
def test_small_nine_point_grids(figures, name, dims, n, level_order):
    """lines of 48 and 200 rows (longer than the level pass' ring of 16) and of 3 rows (shorter); 48, 700 and 7 lines: no multiple of the
    64 lanes of the level pass.  3 x 700 has fewer than 8 entries per row and 1 401 levels of one or two rows: its numbering runs, and
    csr_and_level_fallbacks drops it (deep but not wide), so that ILU(0) of it is NOT an "ilu0:level-order" object"""
    f = figures[name]; A = f["A"]
    assert A.shape[0] == n and dims[1] % 64 != 0 and (dims[0] > 16 or dims[0] < 16)
    assert R.by_level(A, f["lower"][2]) == level_order
    assert R.expected_factor_order(A) ["how"] == R.NATURAL and R.expected_factor_order(A)["natural_w"] == 4
    if not level_order:
        assert A.nnz < 8 * n and f["lower"][2] == 1401 and f["lo"].nnz <= 4 * n          # (its sweeps are no long-row sweeps either)


def test_nine8x300(figures):
    """lines of 8 rows (shorter than the ring of 16) with W = 4 on a matrix that IS an "ilu0:level-order" object: a 9-point grid 8 wide
    still has more than 8 entries per row"""
    f = figures["nine8x300"]; A = f["A"]; n = A.shape[0]
    assert n == 2400 and A.nnz > 8 * n and 300 % 64 != 0 and R.by_level(A, f["lower"][2])
    e = R.expected_factor_order(A)
    assert (e["how"], e["natural_w"]) == (R.NATURAL, 4)
    for T, upper in ((f["up"], True), (f["up"].T.tocsr(), False), (f["lo"].T.tocsr(), True)):
        e = R.expected_slot(T, upper)
        assert (e["how"], e["natural_w"], e["w"], e["block"]) == (R.NATURAL, 4, 4, 256)


def test_box27_3x26x27(figures):
    """lines of 3 rows (shorter than the ring of 16) on a matrix that IS an "ilu0:level-order" object: long rows"""
    f = figures["box27_3x26x27"]; A = f["A"]; n = A.shape[0]
    assert n == 3 * 26 * 27 and A.nnz > 8 * n and (26 * 27) % 64 != 0 and R.by_level(A, f["lower"][2])
    e = R.expected_factor_order(A)
    assert (e["how"], e["natural_w"]) == (R.NATURAL, 16)
    e = R.expected_slot(f["up"], True)
    assert (e["how"], e["w"], e["block"]) == (R.NATURAL, 16, 256)


def test_dense64x16_and_the_matrix_below_the_floor(figures):
    f = figures["dense64x16"]; A = f["A"]
    assert A.shape[0] == 1024 and (np.diff(A.indptr) == 64).all()
    pivots = np.diff(f["lo"].indptr) - 1
    assert np.array_equal(np.bincount(pivots, minlength=64), np.full(64, 16))          # every count 0 .. 63: all edges of the batches of 16
    assert f["lower"][2] == 64 and np.array_equal(np.bincount(f["lower"][0]), np.full(64, 16))
    assert R.by_level(A, 64) and R.expected_factor_order(A)["natural_w"] == 16
    e = R.expected_slot(f["lo"], False, given=True)
    assert (e["w"], e["block"]) == (16, 256)
    B = figures["below_floor"]["A"]
    assert B.shape[0] == 1023 and not R.by_level(B, 64) and (B != A[:1023][:, :1023]).nnz == 0


@pytest.mark.parametrize("name,bs,nblocks,offd,w,block", [("dense9", 9, 4104, 4.0, 4, 1024), ("dense14", 14, 4200, 6.5, 8, 1024),
                                                          ("dense24", 24, 4104, 11.5, 16, 1024), ("dense14_small", 14, 100, 6.5, 8, 256)])
def test_dense_blocks(figures, name, bs, nblocks, offd, w, block):
    f = figures[name]; A = f["A"]; n = A.shape[0]
    assert n == bs * nblocks and n <= 98496 and A.nnz > 8 * n and R.by_level(A, bs)
    assert f["lower"][2] == bs and np.array_equal(np.bincount(f["lower"][0]), np.full(bs, nblocks)) and (nblocks >= 4096) == (block == 1024)
    for T, upper in ((f["lo"], False), (f["up"], True)):
        e = R.expected_slot(T, upper)
        assert R.offdiag_per_row(T) == offd and (e["w"], e["block"], e["how"], e["nlevels"]) == (w, block, R.NATURAL, bs)


def test_counts(figures):
    f = figures["counts"]; A = f["A"]; n = A.shape[0]
    assert n == 4096 and A.nnz > 8 * n and int(np.diff(A.indptr).max()) == 64 and (A != f["lo"]).nnz == 0
    k = np.diff(A.indptr) - 1
    assert np.array_equal(k[63:], np.array(R.COUNTS_K)[np.arange(63, n) % 15])        # exactly k(r) entries left of the diagonal
    assert set(k.tolist()) >= set(R.COUNTS_K)                                          # refills at W, W + 1 and 2 W for W = 4, 8, 16
    level, perm, nlevels = f["lower"]
    e = R.expected_slot(f["lo"], False, given=True)
    assert (e["w"], e["block"]) == (16, 256) and nlevels > 1 and R.by_level(A, nlevels)
    # the sweep over L: some row reads both from its own workgroup of 256 positions (LDS) and from an earlier one (memory)
    pos = np.empty(n, dtype=np.int64); pos[perm] = np.arange(n)
    rows = np.repeat(np.arange(n), np.diff(A.indptr)); off = rows != A.indices
    own = pos[A.indices[off]] // 256 == pos[rows[off]] // 256
    both = np.bincount(rows[off][own], minlength=n).astype(bool) & np.bincount(rows[off][~own], minlength=n).astype(bool)
    assert both.sum() > 100
    # U is the diagonal alone: one level, no off-diagonal entry, the wide block
    e = R.expected_slot(f["up"], True)
    assert f["up"].nnz == n and (e["nlevels"], e["w"], e["block"], e["how"]) == (1, 4, 1024, R.NATURAL)
    assert np.array_equal(e["perm"], np.arange(n))


@pytest.mark.parametrize("name", ["sym_nine48", "sym_box27_13"])
def test_symmetrised_stencils(figures, name):
    A = figures[name]["A"]
    assert abs(A - A.T).max() == 0.0 and A.shape[0] == {"sym_nine48": 2304, "sym_box27_13": 2197}[name]
    assert (A.diagonal() > np.abs(A).sum(axis=1).A1 - A.diagonal()).all()              # dominant: the LL^T factors exist
