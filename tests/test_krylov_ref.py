"""CPU tests of tests/krylov_ref.py, the references that test_gpu_krylov_reference.py holds the Krylov kernels against: the ILU(0) and
IChol(0) factors and their applies against the oracle's restatement (arrays equal), the emulated block dot against the exactly
computed sum, the block updates against the loops they are taken from, and the float64 runs of cg / bicgstab against the long-double
runs.

Relative deviation max|x64 - xld| / max|xld| of the float64 run from the long-double run after iterations 1 .. 12, right-hand side
default_rng(1).standard_normal(n) (test_float64_run_against_long_double prints these rows and bounds every entry by 1e-14):

matrix            solver   M      1       2       3       4       5       6       7       8       9       10      11      12
poisson3d(7)      cg       None   3.2e-16 2.6e-16 4.3e-16 5.2e-16 6.8e-16 8.0e-16 7.5e-16 6.7e-16 5.7e-16 5.1e-16 4.5e-16 4.5e-16
poisson3d(7)      cg       IChol0 6.4e-16 8.3e-16 2.6e-16 2.4e-16 2.2e-16 2.1e-16 2.7e-16 3.0e-16 3.1e-16 3.4e-16 3.5e-16 3.8e-16
poisson3d(7)      cg       ILU0   3.8e-16 3.9e-16 3.2e-16 2.3e-16 2.4e-16 2.3e-16 2.8e-16 3.5e-16 3.0e-16 3.6e-16 3.8e-16 4.0e-16
poisson3d(5,6,7)  cg       None   6.8e-16 5.7e-16 4.9e-16 5.2e-16 5.1e-16 3.8e-16 3.6e-16 2.9e-16 2.6e-16 2.4e-16 2.2e-16 2.1e-16
poisson3d(5,6,7)  cg       IChol0 1.0e-15 5.6e-16 3.0e-16 1.9e-16 1.9e-16 2.4e-16 2.5e-16 2.6e-16 2.9e-16 2.7e-16 3.1e-16 3.7e-16
poisson3d(5,6,7)  cg       ILU0   8.7e-16 5.2e-16 3.6e-16 2.6e-16 2.8e-16 3.0e-16 3.2e-16 3.3e-16 3.2e-16 2.7e-16 3.0e-16 3.2e-16
poisson3d(5,6,7)  bicgstab None   2.7e-16 2.3e-16 2.2e-16 2.0e-16 2.1e-16 3.2e-16 3.8e-16 4.4e-16 3.6e-16 3.4e-16 3.8e-16 3.9e-16
poisson3d(5,6,7)  bicgstab ILU0   5.1e-16 3.2e-16 3.7e-16 3.4e-16 3.0e-16 2.9e-16 4.1e-16 4.2e-16 4.9e-16 5.5e-16 6.7e-16 6.1e-16
poisson3d(7)      bicgstab None   3.1e-16 2.9e-16 3.1e-16 3.0e-16 6.1e-16 3.7e-16 4.0e-16 3.5e-16 3.9e-16 5.7e-16 5.0e-16 5.1e-16
poisson3d(7)      bicgstab ILU0   5.1e-16 5.3e-16 3.3e-16 3.9e-16 4.1e-16 4.4e-16 4.9e-16 5.6e-16 5.8e-16 6.1e-16 6.7e-16 6.4e-16
random_dd(400)    bicgstab None   3.6e-16 4.1e-16 4.6e-16 4.7e-16 4.3e-16 4.7e-16 3.9e-16 4.5e-16 4.6e-16 4.5e-16 4.5e-16 4.5e-16
random_dd(400)    bicgstab ILU0   8.0e-16 8.3e-16 8.9e-16 8.8e-16 8.8e-16 8.8e-16 8.8e-16 8.8e-16 8.8e-16 8.8e-16 8.8e-16 8.8e-16
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import krylov_ref as K
import matgen
from oracle import oracle as O

MATRICES = {
    "poisson3d(7)": lambda: matgen.poisson3d(7),
    "poisson3d(5,6,7)": lambda: matgen.poisson3d(5, 6, 7),
    "random_dd(400)": lambda: matgen.random_dd(400),
}
# (matrix, solver, preconditioner): what the GPU loops are tested on
CASES = [(m, "cg", p) for m in ("poisson3d(7)", "poisson3d(5,6,7)") for p in (None, "IChol0", "ILU0")] + \
        [(m, "bicgstab", p) for m in sorted(MATRICES) for p in (None, "ILU0")]
ITERATIONS = 12


def test_long_double_is_wider_than_float64():
    """the GPU tests measure float64 rounding against long-double runs: that needs the 64-bit significand of x87"""
    assert np.finfo(np.longdouble).eps < 2e-19


@pytest.mark.parametrize("name", ["poisson3d(7)", "random_dd(400)"])
def test_ilu0_and_apply_against_the_oracle(name):
    A = MATRICES[name]()
    n = A[2].shape[0] - 1
    L, U = K.ilu0(A, np.float64)
    Lo, Uo = O.orc().ilu0((A[0], A[1], A[2], True))
    for mine, theirs in ((L, Lo), (U, Uo)):
        assert np.array_equal(mine[1], theirs[1]) and np.array_equal(mine[2], theirs[2])
        assert mine[0].dtype == np.float64 and np.array_equal(mine[0].view(np.uint64), theirs[0].view(np.uint64))
    rng = np.random.default_rng(3)
    b = rng.standard_normal(n)
    x = K.apply_lu(L, U, b, np.float64)
    assert np.array_equal(x.view(np.uint64), O.orc().apply_lu(Lo, Uo, b, O.ID).view(np.uint64))
    B = rng.standard_normal((n, 3))
    X = K.apply_lu(L, U, B, np.float64)
    for j in range(3):
        assert np.array_equal(X[:, j], K.apply_lu(L, U, B[:, j], np.float64))


@pytest.mark.parametrize("name", ["poisson3d(7)", "poisson3d(5,6,7)"])
def test_ichol0_and_apply_against_the_oracle(name):
    A = MATRICES[name]()
    n = A[2].shape[0] - 1
    L = K.ichol0(A, np.float64)
    Lo = O.orc().ichol0((A[0], A[1], A[2], True))
    assert np.array_equal(L[1], Lo[1]) and np.array_equal(L[2], Lo[2])
    assert np.array_equal(L[0].view(np.uint64), Lo[0].view(np.uint64))
    upper_poisoned = (np.where(A[1] > np.repeat(np.arange(n), np.diff(A[2])), np.nan, A[0]), A[1], A[2])
    assert np.array_equal(K.ichol0(upper_poisoned, np.float64)[0], L[0])                   # the lower triangle alone is read
    b = np.random.default_rng(4).standard_normal(n)
    assert np.array_equal(K.apply_llt(L, b, np.float64).view(np.uint64), O.orc().apply_llt(Lo, b, O.ID).view(np.uint64))


def test_csr_matvec_by_rows_in_stored_order():
    A = MATRICES["random_dd(400)"]()
    n = A[2].shape[0] - 1
    x = np.random.default_rng(5).standard_normal(n)
    y = K.csr_matvec(A, x, np.float64)
    for i in range(n):
        s = 0.0
        for q in range(A[2][i], A[2][i + 1]):
            s = s + A[0][q] * x[A[1][q]]
        assert y[i] == s
    yl = K.csr_matvec(A, x, np.longdouble)
    mass = K.csr_matvec((np.abs(A[0]), A[1], A[2]), np.abs(x), np.float64)      # sum |a_ij x_j|; a row has at most 20 entries
    assert yl.dtype == np.longdouble and np.all(np.abs(yl - y) <= 20 * 2.0 ** -53 * mass)


# ---- the block dot ----
def _exact_dot(a, b):
    """(sum a_i b_i, sum |a_i b_i|) as Fractions: the significands as integers, the products shifted to one exponent"""
    ma, ea = np.frexp(a)
    mb, eb = np.frexp(b)
    ia, ib = (ma * 2.0 ** 53).astype(np.int64), (mb * 2.0 ** 53).astype(np.int64)
    assert np.array_equal(ia.astype(np.float64) * 2.0 ** -53, ma) and np.array_equal(ib.astype(np.float64) * 2.0 ** -53, mb)
    e = ea.astype(np.int64) + eb.astype(np.int64)
    low = int(e.min())
    total = absolute = 0
    for x, y, s in zip(ia.tolist(), ib.tolist(), (e - low).tolist()):
        p = (x * y) << s
        total += p
        absolute += abs(p)
    unit = Fraction(2) ** (low - 106)
    return total * unit, absolute * unit


def test_exact_dot_is_exact():
    a, b = np.array([1.0, 2.0 ** -60, -1.0, 3.0]), np.array([1.0, 1.0, 1.0, 2.0 ** -70])
    total, absolute = _exact_dot(a, b)
    assert total == Fraction(2) ** -60 + 3 * Fraction(2) ** -70 and absolute == 2 + total
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal(1000), rng.standard_normal(1000)
    two = []                                                    # math.fsum over exact two-products (Dekker), correctly rounded
    for x, y in zip(a.tolist(), b.tolist()):
        p = x * y
        xh = (x * 134217729.0) - ((x * 134217729.0) - x)
        yh = (y * 134217729.0) - ((y * 134217729.0) - y)
        xl, yl = x - xh, y - yh
        two += [p, ((xh * yh - p) + xh * yl + xl * yh) + xl * yl]
    total = _exact_dot(a, b)[0]
    assert math.fsum(two) == float(total)


@pytest.mark.parametrize("n", [1, 257, 262145])
def test_block_dot_exact_against_the_exact_sum(n):
    """one rounding per product, ceil(chunk / 256) serial adds and an 8-level tree in a workgroup, ceil(nb / 256) serial adds and an
    8-level tree in the finishing one: |result - sum| <= D 2^-53 sum|a_i b_i|, D = ceil(chunk / 256) + ceil(nb / 256) + 17"""
    nb, chunk = K.block_dot_shape(n)
    assert (nb, chunk) == {1: (1, 1), 257: (2, 129), 262145: (1024, 257)}[n]
    D = -(-chunk // 256) + -(-nb // 256) + 17
    rng = np.random.default_rng(n)
    scales = np.logspace(-3, 3, 3)
    a, b = rng.standard_normal((n, 3)), rng.standard_normal((n, 3)) * scales
    got = K.block_dot_exact(a, b)
    assert got.shape == (3,) and got.dtype == np.float64
    for j in range(3):
        assert K.block_dot_exact(a[:, j], b[:, j]) == got[j]
        total, absolute = _exact_dot(a[:, j], b[:, j])
        err = abs(Fraction(float(got[j])) - total)
        print("n = %d column %d: error %.3g of the bound" % (n, j, float(err / (D * Fraction(1, 2 ** 53) * absolute))))
        assert err <= D * Fraction(1, 2 ** 53) * absolute
    if n == 1:
        assert got[0] == a[0, 0] * b[0, 0]


def test_block_dot_exact_order():
    """the vectorised emulation against the same shape written out with scalar loops"""
    # 513 rows: nb = 3, chunk = 171; 600 rows: chunk = 200; 70000 rows: nb = 274, the finishing group's second sweep
    for n in (513, 600, 70000):
        rng = np.random.default_rng(n)
        a, b = rng.standard_normal(n), rng.standard_normal(n)
        nb, chunk = K.block_dot_shape(n)
        part = []
        for g in range(nb):
            p = (a * b)[g * chunk:min(n, (g + 1) * chunk)]
            sh = np.zeros(256)
            for v in range(256):
                for t in p[v::256].tolist():
                    sh[v] = sh[v] + t
            s = 128
            while s:
                for w in range(s):
                    sh[w] = sh[w] + sh[w + s]
                s >>= 1
            part.append(sh[0])
        sh = np.zeros(256)
        for t in range(256):
            for v in part[t::256]:
                sh[t] = sh[t] + v
        s = 128
        while s:
            for w in range(s):
                sh[w] = sh[w] + sh[w + s]
            s >>= 1
        assert K.block_dot_exact(a, b) == sh[0], n


# ---- the block updates are the statements of the loops ----
def test_block_updates_reproduce_the_loops():
    """cg / bicgstab of krylov_ref, run again with every vector statement replaced by block_update: the same bits, and a column switched
    off keeps its bits"""
    A = MATRICES["random_dd(400)"]()
    S = matgen.symmetrize(*A)
    n = A[2].shape[0] - 1
    B = K.rhs_block(A, 7)
    k = B.shape[1]
    on = np.ones(k, dtype=np.uint8)
    none = None
    # CG
    want = K.cg(S, B, 4, np.float64)[0]
    x, r = np.zeros_like(B), B.copy()
    p = r.copy()
    rz = K._dot(r, r)
    for it in range(4):
        Ap = K.csr_matvec(S, p, np.float64)
        alpha = rz / K._dot(p, Ap)
        K.block_update("cg", 0, on, alpha, none, none, x, r, p, none, Ap, none)
        assert np.array_equal(x, want[it])
        rz_new = K._dot(r, r)
        K.block_update("cg", 1, on, rz_new / rz, none, none, x, r, p, none, r, none)
        rz = rz_new
    # BiCGstab
    want = K.bicgstab(A, B, 4, np.float64)[0]
    y, r = np.zeros_like(B), B.copy()
    r0, p, s = r.copy(), r.copy(), np.zeros_like(B)
    for it in range(4):
        Ap = K.csr_matvec(A, p, np.float64)
        rho = K._dot(r, r0)
        alpha = rho / K._dot(Ap, r0)
        K.block_update("bicgstab", 0, on, alpha, none, none, y, r, p, s, Ap, none)
        As = K.csr_matvec(A, s, np.float64)
        omega = K._dot(As, s) / K._dot(As, As)
        K.block_update("bicgstab", 1, on, alpha, omega, none, y, r, p, s, Ap, As)
        beta = (K._dot(r, r0) / rho) * (alpha / omega)
        K.block_update("bicgstab", 2, on, alpha, omega, beta, y, r, p, s, Ap, As)
        assert np.array_equal(y, want[it])
    # a column that is switched off
    off = on.copy()
    off[2] = 0
    before = [v.copy() for v in (y, r, p, s)]
    for stage in range(3):
        K.block_update("bicgstab", stage, off, alpha, omega, beta, y, r, p, s, Ap, As)
    for v, w in zip((y, r, p, s), before):
        assert np.array_equal(v[:, 2], w[:, 2]) and not np.array_equal(v[:, 1], w[:, 1])


# ---- float64 against long double ----
@pytest.mark.parametrize("matrix,solver,kind", CASES)
def test_float64_run_against_long_double(matrix, solver, kind):
    A = MATRICES[matrix]()
    n = A[2].shape[0] - 1
    b = np.random.default_rng(1).standard_normal(n)
    pair = K.Pair(solver, A, kind, b, ITERATIONS)
    rel = [float(d / s) for d, s in zip(pair.dev, pair.scale)]
    print("%-17s %-8s %-6s " % (matrix, solver, kind) + " ".join("%.1e" % v for v in rel))
    assert pair.xld[0].dtype == np.longdouble and pair.x64[0].dtype == np.float64
    assert all(np.isfinite(v) and v <= 1e-14 for v in rel), rel
    assert max(rel) > 0.0                                       # the two runs do differ: the long-double run is no float64 run
    # the long-double run solves the system: its true residual follows its recurrence residual
    true = b - K.csr_matvec(A, pair.xld[-1], np.longdouble)
    if solver == "cg":
        assert float(np.sqrt(K._dot(true, true)) / np.sqrt(K._dot(b, b))) <= float(pair.rel[-1]) + 1e-15
    assert float(np.sqrt(K._dot(true, true))) <= 1e-2 * float(np.sqrt(K._dot(b, b)))
