"""The Krylov layer against references from outside the package (tests/krylov_ref.py, numpy only):

  - ilupp_hip_block_dot_device, called directly with leading dimensions of its own: the bits of the documented reduction shape;
  - the block updates, called directly: the bits of one numpy statement per kernel statement, masked columns and every array a stage
    does not write bitwise unchanged;
  - cg / bicgstab (k columns and 1-D) and cg_batch / bicgstab_batch against the same recurrence run in long double with factors built
    in long double by krylov_ref: the iterates after m iterations within 8 times the deviation of a float64 run of the reference from
    the long-double run, and the iteration at which a column stops.

Measured on an MI355X, the largest max|x_gpu - x_ld| / max(dev64) of each case over its columns and m (the bound is 8):

matrix            solver   M       k columns                1-D                      cg_batch / bicgstab_batch
poisson3d(7)      cg       None    1.50 (m = 2, column 4)   1.00 (m = 3, column 4)   1.00 (m = 1, column 0)
poisson3d(7)      cg       IChol0  1.00 (m = 2, column 1)   1.30 (m = 12, column 1)  1.00 (m = 1, column 1)
poisson3d(7)      cg       ILU0    1.18 (m = 1, column 1)   1.00 (m = 1, column 1)   0.81 (m = 12, column 2)
poisson3d(5,6,7)  cg       None    3.98 (m = 1, column 3)   3.98 (m = 1, column 3)   3.98 (m = 1, column 3)
poisson3d(5,6,7)  cg       IChol0  1.46 (m = 2, column 2)   1.49 (m = 1, column 2)   0.95 (m = 12, column 4)
poisson3d(5,6,7)  cg       ILU0    0.82 (m = 6, column 4)   0.93 (m = 12, column 0)  0.71 (m = 12, column 0)
poisson3d(7)      bicgstab None    1.62 (m = 12, column 4)  1.72 (m = 6, column 4)   0.61 (m = 1, column 0)
poisson3d(7)      bicgstab ILU0    1.14 (m = 3, column 3)   1.14 (m = 12, column 2)  1.02 (m = 1, column 1)
poisson3d(5,6,7)  bicgstab None    1.14 (m = 3, column 1)   2.99 (m = 1, column 0)   1.10 (m = 12, column 2)
poisson3d(5,6,7)  bicgstab ILU0    1.61 (m = 3, column 4)   2.94 (m = 3, column 4)   1.23 (m = 6, column 3)
random_dd(400)    bicgstab None    1.26 (m = 1, column 1)   1.26 (m = 1, column 1)   1.00 (m = 6, column 4)
random_dd(400)    bicgstab ILU0    1.01 (m = 1, column 1)   1.15 (m = 1, column 0)   1.00 (m = 1, column 0)
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import krylov_ref as K
import matgen

pytestmark = pytest.mark.gpu

PAYLOAD = np.uint64(0x7FF85EEDC0DE0001)                     # a quiet NaN with a payload: arithmetic on it would not give these bits back


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- 1. the block dot ------------------------------------------------------------------------------------------------------------
DOT_KS = (1, 2, 3, 7, 8, 15, 16, 17, 31, 33)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 262144, 262145])
def test_block_dot_has_the_bits_of_the_documented_shape(n):
    """n = 262145: chunk = 257, a second sweep of a workgroup's lanes that holds one row.  Column j is the same data for every k, so
    the expected bits are computed once per n."""
    import torch
    from ilupp_amd import _native
    lib = _native.lib()
    kmax = max(DOT_KS)
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, kmax))
    B = rng.standard_normal((n, kmax)) * np.logspace(-3, 3, kmax)
    want = K.block_dot_exact(A, B)
    assert want.shape == (kmax,) and np.all(np.isfinite(want))
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    nan = float("nan")
    for k in DOT_KS:
        for lda, ldb in ((k, k), (k + 3, k + 1)):
            a = torch.full((n, lda), nan, dtype=torch.float64, device="cuda")
            b = torch.full((n, ldb), nan, dtype=torch.float64, device="cuda")
            a[:, :k] = Ad[:, :k]
            b[:, :k] = Bd[:, :k]
            out = torch.from_numpy(np.full(k + 2, PAYLOAD).view(np.float64)).cuda()
            rc = lib.ilupp_hip_block_dot_device(n, k, a.data_ptr(), lda, b.data_ptr(), ldb, out.data_ptr(), _stream())
            assert rc == 0, (k, lda, ldb)
            got = out.cpu().numpy()
            assert np.array_equal(_bits(got[:k]), _bits(want[:k])), (n, k, lda, ldb, got[:k], want[:k])
            assert np.all(_bits(got[k:]) == PAYLOAD), (n, k, lda, ldb)


# ---- 2. the block updates --------------------------------------------------------------------------------------------------------
STAGES = [("cg", 0), ("cg", 1), ("bicgstab", 0), ("bicgstab", 1), ("bicgstab", 2)]
WRITTEN = {("cg", 0): (0, 1), ("cg", 1): (2,), ("bicgstab", 0): (3,), ("bicgstab", 1): (0, 1), ("bicgstab", 2): (2,)}


def _update_sizes(k):
    rows = 1 if k >= 4096 else -(-4096 // k)
    return sorted({n for n in (1, rows - 1, rows, rows + 1, 3 * rows + 1) if n >= 1})


@pytest.mark.parametrize("k", [1, 2, 3, 5, 7, 8, 16, 17, 255, 256, 257, 300, 4095, 4096, 4097])
def test_block_updates_have_the_bits_of_the_statements(k):
    """a workgroup owns `rows` rows and walks them with a column counter stepped by 256 % k: n around rows and 3 rows + 1, k on both
    sides of 256 and of 4096.  The active mask has period 7; inactive columns hold NaN, Inf and a NaN payload in every operand."""
    import torch
    from ilupp_amd import _native
    lib = _native.lib()
    active = np.isin(np.arange(k) % 7, (0, 2, 3, 5)).astype(np.uint8)
    poison = np.array([np.nan, np.inf, 0.0])
    poison.view(np.uint64)[2] = PAYLOAD
    fill = poison[np.arange(k) % 3]
    off = active == 0
    for n in _update_sizes(k):
        rng = np.random.default_rng(1000 * k + n)
        V = [rng.standard_normal((n, k)) for _ in range(4)]
        W = [rng.standard_normal((n, k)) for _ in range(2)]
        c = [rng.standard_normal(k) + 2.0 for _ in range(3)]
        for t in V + W:
            t[:, off] = fill[off]
        for t in c:
            t[off] = fill[off]
        for solver, stage in STAGES:
            want = [t.copy() for t in V]
            K.block_update(solver, stage, active, c[0], c[1], c[2], want[0], want[1], want[2], want[3], W[0], W[1])
            dV = [torch.from_numpy(t).cuda() for t in V]
            dW = [torch.from_numpy(t).cuda() for t in W]
            dc = [torch.from_numpy(t).cuda() for t in c]
            da = torch.from_numpy(active).cuda()
            if solver == "cg":
                rc = lib.ilupp_hip_cg_block_update_device(stage, n, k, da.data_ptr(), dc[0].data_ptr(), dV[0].data_ptr(), dV[1].data_ptr(),
                                                          dV[2].data_ptr(), dW[0].data_ptr(), _stream())
            else:
                rc = lib.ilupp_hip_bicgstab_block_update_device(stage, n, k, da.data_ptr(), dc[0].data_ptr(), dc[1].data_ptr(),
                                                                dc[2].data_ptr(), dV[0].data_ptr(), dV[1].data_ptr(), dV[2].data_ptr(),
                                                                dV[3].data_ptr(), dW[0].data_ptr(), dW[1].data_ptr(), _stream())
            assert rc == 0
            where = (k, n, solver, stage)
            for q in range(4):
                got = dV[q].cpu().numpy()
                assert np.array_equal(_bits(got), _bits(want[q])), where + ("V%d" % q,)
                assert np.array_equal(_bits(got[:, off]), _bits(V[q][:, off])), where + ("inactive columns of V%d" % q,)
                if q not in WRITTEN[(solver, stage)]:
                    assert np.array_equal(_bits(got), _bits(V[q])), where + ("V%d is not written by this stage" % q,)
                else:
                    assert not np.array_equal(_bits(got), _bits(V[q])), where + ("V%d is written by this stage" % q,)
            for q in range(2):
                assert np.array_equal(_bits(dW[q].cpu().numpy()), _bits(W[q])), where + ("W%d" % q,)
            for q in range(3):
                assert np.array_equal(_bits(dc[q].cpu().numpy()), _bits(c[q])), where + ("c%d" % q,)
            assert np.array_equal(da.cpu().numpy(), active)


# ---- 3. the loops ----------------------------------------------------------------------------------------------------------------
MATRICES = {
    "poisson3d(7)": lambda: matgen.poisson3d(7),
    "poisson3d(5,6,7)": lambda: matgen.poisson3d(5, 6, 7),
    "random_dd(400)": lambda: matgen.random_dd(400),                # nonsymmetric: BiCGstab only
}
CG_CASES = [(m, "cg", p) for m in ("poisson3d(7)", "poisson3d(5,6,7)") for p in (None, "IChol0", "ILU0")]
BICGSTAB_CASES = [(m, "bicgstab", p) for m in ("poisson3d(7)", "poisson3d(5,6,7)", "random_dd(400)") for p in (None, "ILU0")]
WITH_X0 = {("poisson3d(5,6,7)", "cg", "IChol0"), ("random_dd(400)", "bicgstab", "ILU0")}
MS = (1, 2, 3, 6, 12)
ITERATIONS = max(MS)


class Case:
    """one (matrix, solver, preconditioner): the k = 5 right-hand sides, the starting block where the case has one, and the pair of
    reference runs -- computed once, shared by every test below, never written to"""

    def __init__(self, matrix, solver, kind):
        self.key = (matrix, solver, kind)
        self.triple = MATRICES[matrix]()
        self.n = self.triple[2].shape[0] - 1
        self.B = K.rhs_block(self.triple, 11)
        # a starting block of the right-hand sides' own sizes (a column of 1e-6 started from O(1) would be a different problem)
        self.x0 = np.random.default_rng(12).standard_normal(self.B.shape) * (0.1 * np.abs(self.B).max(axis=0)) if self.key in WITH_X0 else None
        self.pair = K.Pair(solver, self.triple, kind, self.B, ITERATIONS, self.x0)
        for t in (self.B, self.x0):
            if t is not None:
                t.setflags(write=False)

    def well_conditioned(self):
        """on the reference alone: the float64 run stays within 1e-14 of the long-double run, relative to the iterate"""
        for m in range(ITERATIONS):
            dev, scale = self.pair.dev[m], self.pair.scale[m]
            assert np.all(np.isfinite(dev.astype(np.float64))) and np.all(dev <= 1e-14 * scale), (self.key, m + 1, dev / scale)

    def device(self):
        """(DeviceCSR, a fresh preconditioner or None)"""
        import ilupp_amd.device as ild
        A = sp.csr_matrix(self.triple, shape=(self.n, self.n))
        dA = ild.DeviceCSR.from_scipy(A)
        return dA, None if self.key[2] is None else ild.DevicePreconditioner(self.key[2], dA)

    def ratio(self, x, m, j):
        """max|x - x_ld| / max(dev64) of column j after m iterations, dev64 over the iterations up to m: the figure that must not exceed 8"""
        x = np.asarray(x, dtype=np.float64)
        assert np.all(np.isfinite(x)), (self.key, m, j)
        err = np.max(np.abs(x.astype(np.longdouble) - self.pair.xld[m - 1][:, j]))
        bound = self.pair.bound(m)[j]
        assert bound > 0, (self.key, m, j)
        return float(8 * err / bound)


@functools.lru_cache(maxsize=None)
def _case(matrix, solver, kind):
    return Case(matrix, solver, kind)


def _report(what, key, ratios):
    """prints the largest ratio of a case; returns the (ratio, m, column) above the bound"""
    worst = max(ratios)
    print("RATIO %-14s %-17s %-8s %-6s %.2f  (m = %d, column %d)" % ((what,) + tuple(str(v) for v in key) + worst))
    return [(what, key) + t for t in sorted(ratios, reverse=True) if not t[0] <= 8.0]


@pytest.mark.parametrize("matrix,solver,kind", CG_CASES + BICGSTAB_CASES)
def test_iterates_against_the_long_double_recurrence(matrix, solver, kind):
    """check_every = 0, the iterates after m = 1, 2, 3, 6, 12 iterations (CG: maxiter = m; BiCGstab: history), the k-column path and
    the 1-D path of every column: max|x_gpu - x_ld| <= 8 max(dev64), dev64 the float64 reference's own deviation from the long-double
    run over the iterations up to m of that column.  The kernel and the float64 reference round the same recurrence and differ in the
    order of the dot products' sums only, which changes the sign and size of the error, not its order: a factor of 8, three bits."""
    import torch
    import ilupp_amd.device as ild
    case = _case(matrix, solver, kind)
    case.well_conditioned()
    dA, M = case.device()
    k = case.B.shape[1]
    Bd = torch.from_numpy(case.B.copy()).cuda()
    x0d = None if case.x0 is None else torch.from_numpy(case.x0.copy()).cuda()
    block, single = [], []
    if solver == "cg":
        for m in MS:
            stats = {}
            X = ild.cg(dA, Bd, M, x0=x0d, maxiter=m, stats=stats).cpu().numpy()
            assert stats["iterations"].tolist() == [m] * k and not stats["converged"].any()
            block += [(case.ratio(X[:, j], m, j), m, j) for j in range(k)]
            for j in range(k):
                x = ild.cg(dA, Bd[:, j].contiguous(), M, x0=None if x0d is None else x0d[:, j].contiguous(), maxiter=m)
                single.append((case.ratio(x.cpu().numpy(), m, j), m, j))
    else:
        hist, stats = [], {}
        Y = ild.bicgstab(dA, Bd, M, x0=x0d, maxiter=ITERATIONS, history=hist, stats=stats)
        assert len(hist) == ITERATIONS and torch.equal(hist[-1], Y)
        assert stats["iterations"].tolist() == [ITERATIONS] * k and not stats["converged"].any()
        for m in MS:
            X = hist[m - 1].cpu().numpy()
            block += [(case.ratio(X[:, j], m, j), m, j) for j in range(k)]
        stats = {}
        Y3 = ild.bicgstab(dA, Bd, M, x0=x0d, maxiter=3, stats=stats)
        assert stats["iterations"].tolist() == [3] * k and torch.equal(Y3, hist[2])
        for j in range(k):
            hist1 = []
            ild.bicgstab(dA, Bd[:, j].contiguous(), M, x0=None if x0d is None else x0d[:, j].contiguous(), maxiter=ITERATIONS, history=hist1)
            assert len(hist1) == ITERATIONS
            single += [(case.ratio(hist1[m - 1].cpu().numpy(), m, j), m, j) for m in MS]
    over = _report("block", case.key, block) + _report("1-D", case.key, single)
    assert not over, over


def _stopping_run(case):
    """(rtol, maxiter), from the reference alone: no long-double relative residual that such a run looks at comes closer to rtol than a
    factor of 2.  Five columns' residuals lie densely, and a column that gains less than a factor of 4 per iteration cannot cross any
    rtol at that distance, so maxiter is searched too (12 down to 2, rtol = 10^-0.1, 10^-0.15 .. 10^-10): the pair that lets the
    most columns converge, then stops them at the most different iterations, then the longest run, then the widest margin.  Where no
    pair lets a column converge, the run checks that none stops."""
    best = None
    for maxiter in range(ITERATIONS, 1, -1):
        for e in range(10, 1001, 5):
            rtol = float(10.0 ** (-e / 100.0))
            margin = case.pair.margin(rtol, maxiter)
            its, conv = case.pair.stop(rtol, maxiter)
            score = (int(conv.sum()), len(set(its.tolist())), maxiter, margin)
            if margin >= 2.0 and (best is None or score > best[0]):
                best = (score, rtol, maxiter)
    assert best is not None, case.key
    return best[1], best[2]


@pytest.mark.parametrize("matrix,solver,kind", CG_CASES + BICGSTAB_CASES)
def test_stopping_against_the_long_double_residuals(matrix, solver, kind):
    """check_every = 1: every column stops at the iteration at which the reference's relative residual (CG: ||r|| / ||b||; BiCGstab:
    the preconditioned ||r|| / ||r_0||) first falls to rtol, and is reported converged exactly when that happens within maxiter"""
    import torch
    import ilupp_amd.device as ild
    case = _case(matrix, solver, kind)
    rtol, maxiter = _stopping_run(case)
    assert case.pair.margin(rtol, maxiter) >= 2.0               # on the reference alone, before the GPU is touched
    want_its, want_conv = case.pair.stop(rtol, maxiter)
    assert want_its.min() >= 1
    dA, M = case.device()
    Bd = torch.from_numpy(case.B.copy()).cuda()
    x0d = None if case.x0 is None else torch.from_numpy(case.x0.copy()).cuda()
    stats = {}
    solve = ild.cg if solver == "cg" else ild.bicgstab
    solve(dA, Bd, M, x0=x0d, maxiter=maxiter, rtol=rtol, check_every=1, stats=stats)
    print("STOP %s rtol %.2e maxiter %d iterations %s converged %s" % (case.key, rtol, maxiter, want_its.tolist(), want_conv.tolist()))
    assert stats["iterations"].tolist() == want_its.tolist(), (rtol, stats["iterations"].tolist(), want_its.tolist())
    assert stats["converged"].tolist() == want_conv.tolist(), (rtol, stats["converged"].tolist(), want_conv.tolist())


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_batched_kernels_against_the_long_double_recurrence(solver):
    """cg_batch / bicgstab_batch with one member per (matrix, preconditioner), member i solving column i mod 5 of its case, at unequal
    offsets with guard elements between them: every member within the bound of the iterates' test after m = 1, 6, 12 iterations,
    every member solved inside the launch, the guards bitwise untouched"""
    import torch
    import ilupp_amd.device as ild
    cases = [_case(*key) for key in (CG_CASES if solver == "cg" else BICGSTAB_CASES)]
    for case in cases:
        case.well_conditioned()
    cols = [i % 5 for i in range(len(cases))]
    offsets, total = [], 2
    for i, case in enumerate(cases):
        offsets.append(total)
        total += case.n + 1 + 3 * i                             # 1, 4, 7 .. guard elements behind the members
    b = np.full(total, PAYLOAD).view(np.float64).copy()
    x0 = b.copy()
    guard = np.ones(total, dtype=bool)
    for case, j, o in zip(cases, cols, offsets):
        b[o:o + case.n] = case.B[:, j]
        x0[o:o + case.n] = 0.0 if case.x0 is None else case.x0[:, j]
        guard[o:o + case.n] = False
    assert guard.sum() == 2 + sum(1 + 3 * i for i in range(len(cases)))
    devs = [case.device() for case in cases]
    bd, x0d = torch.from_numpy(b).cuda(), torch.from_numpy(x0).cuda()
    batch = ild.cg_batch if solver == "cg" else ild.bicgstab_batch
    ratios = {case.key: [] for case in cases}
    for m in (1, 6, 12):
        stats = {}
        x = batch([d[0] for d in devs], bd, offsets, [d[1] for d in devs], x0=x0d, maxiter=m, stats=stats)
        assert stats["route"] == [0] * len(cases), stats["route"]
        assert stats["iterations"].tolist() == [m] * len(cases) and not stats["converged"].any()
        xh = x.cpu().numpy()
        assert np.all(_bits(xh)[guard] == PAYLOAD)
        assert np.array_equal(_bits(bd.cpu().numpy()), _bits(b)) and np.array_equal(_bits(x0d.cpu().numpy()), _bits(x0))
        for case, j, o in zip(cases, cols, offsets):
            ratios[case.key].append((case.ratio(xh[o:o + case.n], m, j), m, j))
    over = sum((_report(solver + "_batch", case.key, ratios[case.key]) for case in cases), [])
    assert not over, over
