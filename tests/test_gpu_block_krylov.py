"""k right-hand sides on the device: the CSR SpMM against the SpMV column by column (bit for bit), the block dot products against
dots of one column, and the k-column CG / BiCGstab against the same solve of each column alone (bit for bit), with per-column
freezing, isolation of a NaN column, and a non-default stream."""
import numpy as np
import pytest
import scipy.sparse as sp

import matgen

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 7, 8, 9, 16, 17, 33, 64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _csr(t):
    d, i, p = t
    A = sp.csr_matrix((d, i, p), shape=(p.shape[0] - 1, p.shape[0] - 1))
    A.sort_indices()
    return A


def _empty_row_matrix():
    A = _csr(matgen.poisson3d(20)).tolil()
    A[37, :] = 0
    A[1000, :] = 0
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    assert A.indptr[38] == A.indptr[37] and A.indptr[1001] == A.indptr[1000]
    return A


MATRICES = {
    "poisson3d64": lambda: _csr(matgen.poisson3d(64)),
    "box27": lambda: sp.csr_matrix(matgen.box_stencil((40, 40, 40))),
    "random_dd": lambda: _csr(matgen.random_dd(200000)),
    "empty_row": _empty_row_matrix,
}


def _block(n, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, k))


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_spmm_equals_spmv_per_column(name):
    import torch
    import ilupp_amd.device as ild
    A = MATRICES[name]()
    A.sort_indices()
    n = A.shape[0]
    if name == "box27":
        assert A.nnz > 8 * n                           # the long-row variant
    dA = ild.DeviceCSR.from_scipy(A)
    for k in KS:
        X = _block(n, k, k)
        if k >= 3:
            X[5, 1] = np.nan                           # a NaN column (its bits are compared too)
            X[n - 1, 2] = np.inf
        Xd = torch.from_numpy(X).cuda()
        X0 = Xd.clone()
        Y = dA.matmat(Xd)
        cols = [dA.matvec(Xd[:, j].contiguous()) for j in range(k)]
        torch.cuda.synchronize()
        Yh = Y.cpu().numpy()
        assert Yh.shape == (n, k)
        assert np.array_equal(_bits(Xd.cpu().numpy()), _bits(X0.cpu().numpy())), "X changed"
        for j in range(k):
            assert np.array_equal(_bits(Yh[:, j]), _bits(cols[j].cpu().numpy())), (name, k, j)
            if np.all(np.isfinite(X[:, j])):
                assert np.array_equal(_bits(Yh[:, j]), _bits(A @ X[:, j])), (name, k, j)
        if k == 9:
            assert np.array_equal(_bits((dA @ Xd).cpu().numpy()), _bits(Yh))
    # a row-major sub-block with ldx > k, into a sub-block of a wider output (the columns around it untouched)
    W = torch.from_numpy(_block(n, 40, 7)).cuda()
    X = W[:, 3:20]
    out = torch.full((n, 30), -7.0, dtype=torch.float64, device="cuda")
    Y = dA.matmat(X, out=out[:, 5:22])
    torch.cuda.synchronize()
    Wh, Oh = W.cpu().numpy(), out.cpu().numpy()
    for j in range(17):
        assert np.array_equal(_bits(Oh[:, 5 + j]), _bits(A @ Wh[:, 3 + j])), j
    assert np.all(Oh[:, :5] == -7.0) and np.all(Oh[:, 22:] == -7.0)
    assert Y.data_ptr() == out[:, 5:22].data_ptr()
    # k = 0
    E = dA.matmat(torch.empty((n, 0), dtype=torch.float64, device="cuda"))
    assert tuple(E.shape) == (n, 0)


def test_matvec_of_a_block_is_matmat():
    """DeviceCSR.matvec on a 2-D tensor: before the SpMM it read the block as one vector of length n"""
    import torch
    import ilupp_amd.device as ild
    A = _csr(matgen.poisson3d(24))
    n = A.shape[0]
    dA = ild.DeviceCSR.from_scipy(A)
    X = torch.from_numpy(_block(n, 8, 3)).cuda()
    Y1 = dA.matvec(X)
    Y2 = dA.matmat(X)
    Y3 = dA @ X
    torch.cuda.synchronize()
    want = np.column_stack([A @ X.cpu().numpy()[:, j] for j in range(8)])
    for Y in (Y1, Y2, Y3):
        assert tuple(Y.shape) == (n, 8)
        assert np.array_equal(_bits(Y.cpu().numpy()), _bits(want))


def test_spmm_refuses_overlap():
    import torch
    import ilupp_amd.device as ild
    dA = ild.DeviceCSR.from_scipy(_csr(matgen.poisson3d(8)))
    X = torch.ones((dA.n, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="overlap"):
        dA.matmat(X, out=X)


@pytest.mark.parametrize("n", [1, 255, 300001])
def test_block_dot(n):
    import torch
    from ilupp_amd.device import _block_dot
    A = _block(n, 33, 11)
    B = _block(n, 33, 12) * np.logspace(-3, 3, 33)
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    for k in (9, 33):
        d = _block_dot(Ad[:, :k].contiguous(), Bd[:, :k].contiguous()).cpu().numpy()
        for j in range(k):
            d1 = _block_dot(Ad[:, j:j + 1].contiguous(), Bd[:, j:j + 1].contiguous()).cpu().numpy()
            assert _bits(d[j:j + 1]) == _bits(d1), (k, j)
            assert abs(d[j] - np.dot(A[:, j], B[:, j])) <= 1e-13 * np.dot(np.abs(A[:, j]), np.abs(B[:, j])), (k, j)
    # run to run
    d2 = _block_dot(Ad, Bd).cpu().numpy()
    d3 = _block_dot(Ad, Bd).cpu().numpy()
    assert np.array_equal(_bits(d2), _bits(d3))


def _rhs_columns(A, seed):
    """9 right-hand sides of different scales and difficulty, column 4 zero"""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    t = np.arange(n) / n
    cols = [np.ones(n), rng.standard_normal(n) * 1e4, rng.random(n) * 1e-6, np.sin(40 * np.pi * t), np.zeros(n),
            A @ rng.standard_normal(n), np.where(np.arange(n) == n // 3, 1.0, 0.0), t * 3.0 - 1.0, rng.standard_normal(n)]
    return np.ascontiguousarray(np.column_stack(cols))


def _check_block_solve(solve, A, dA, M, B, rtol, check_every, true_tol, distinct=2, maxiter=1000):
    import torch
    n, k = B.shape
    Bd = torch.from_numpy(B).cuda()
    stats = {}
    X = solve(dA, Bd, M, maxiter=maxiter, rtol=rtol, check_every=check_every, stats=stats)
    torch.cuda.synchronize()
    Xh = X.cpu().numpy()
    it, conv, rel = stats["iterations"].numpy(), stats["converged"].numpy(), stats["relres"].numpy()
    assert it.dtype == np.int64 and conv.dtype == np.bool_ and rel.dtype == np.float64 and it.shape == (k,)
    for j in range(k):
        s1 = {}
        x1 = solve(dA, Bd[:, j:j + 1].contiguous(), M, maxiter=maxiter, rtol=rtol, check_every=check_every, stats=s1)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Xh[:, j]), _bits(x1.cpu().numpy()[:, 0])), j
        assert int(s1["iterations"][0]) == it[j] and bool(s1["converged"][0]) == conv[j], j
    zero = [j for j in range(k) if not B[:, j].any()]
    for j in zero:
        assert it[j] == 0 and conv[j] and np.all(Xh[:, j] == 0.0) and rel[j] == 0.0
    for j in range(k):
        if j in zero:
            continue
        assert conv[j], (j, it[j], rel[j])
        assert rel[j] <= rtol
        assert np.linalg.norm(B[:, j] - A @ Xh[:, j]) <= true_tol * np.linalg.norm(B[:, j]), j
    assert len(set(it.tolist())) >= distinct, it
    return it


@pytest.mark.parametrize("kind", [None, "IChol0", "ICholT", "ILU0"])
def test_block_cg_columns_are_their_own_solves(kind):
    import ilupp_amd.device as ild
    A = _csr(matgen.poisson3d(48))
    dA = ild.DeviceCSR.from_scipy(A)
    M = None if kind is None else ild.DevicePreconditioner(kind, dA, **({"add_fill_in": 5, "threshold": 1e-3} if kind == "ICholT" else {}))
    B = _rhs_columns(A, 1)
    it = _check_block_solve(ild.cg, A, dA, M, B, 1e-8, 5, 1e-8, distinct=3 if kind in (None, "IChol0") else 2)
    assert it.max() > 0 and it.max() < 1000


@pytest.mark.parametrize("kind,params", [("ILUT", {"fill_in": 10, "threshold": 1e-4}), ("ILUC", {"fill_in": 8, "threshold": 1e-2})])
def test_block_bicgstab_columns_are_their_own_solves(kind, params):
    """the relative residual of BiCGstab is that of the left-preconditioned residual: rtol 1e-10 there keeps the true one below 1e-8"""
    import ilupp_amd.device as ild
    A = _csr(matgen.random_dd(50000))
    dA = ild.DeviceCSR.from_scipy(A)
    M = ild.DevicePreconditioner(kind, dA, **params)
    B = _rhs_columns(A, 2)
    _check_block_solve(ild.bicgstab, A, dA, M, B, 1e-10, 1, 1e-8, maxiter=200)


def test_block_bicgstab_history_and_fixed_count():
    """check_every = 0: every column runs maxiter iterations; history holds the iterates"""
    import torch
    import ilupp_amd.device as ild
    A = _csr(matgen.random_dd(20000))
    dA = ild.DeviceCSR.from_scipy(A)
    M = ild.DevicePreconditioner("ILUT", dA, fill_in=5, threshold=1e-2)
    B = torch.from_numpy(_rhs_columns(A, 3)).cuda()
    hist, stats = [], {}
    X = ild.bicgstab(dA, B, M, maxiter=4, history=hist, stats=stats)
    torch.cuda.synchronize()
    assert len(hist) == 4 and torch.equal(hist[-1], X)
    assert stats["iterations"].tolist() == [4, 4, 4, 4, 0, 4, 4, 4, 4]


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_nan_column_is_isolated(solver):
    import torch
    import ilupp_amd.device as ild
    A = _csr(matgen.poisson3d(32)) if solver == "cg" else _csr(matgen.random_dd(30000))
    dA = ild.DeviceCSR.from_scipy(A)
    M = ild.DevicePreconditioner("ICholT", dA, add_fill_in=5, threshold=1e-3) if solver == "cg" else \
        ild.DevicePreconditioner("ILUT", dA, fill_in=10, threshold=1e-4)
    solve = ild.cg if solver == "cg" else ild.bicgstab
    B = _rhs_columns(A, 4)[:, :6].copy()
    B[100, 2] = np.nan
    B[7, 3] = np.inf
    Bd = torch.from_numpy(B).cuda()
    stats = {}
    X = solve(dA, Bd, M, maxiter=300, rtol=1e-9, check_every=2, stats=stats)
    Xh = X.cpu().numpy()
    for j in (2, 3):
        assert not bool(stats["converged"][j]) and int(stats["iterations"][j]) == 0, j
        assert np.array_equal(_bits(Xh[:, j]), _bits(np.zeros(A.shape[0]))), j          # frozen at x0: never 0 * NaN
    for j in (0, 1, 4, 5):
        x1 = solve(dA, Bd[:, j:j + 1].contiguous(), M, maxiter=300, rtol=1e-9, check_every=2)
        assert np.array_equal(_bits(Xh[:, j]), _bits(x1.cpu().numpy()[:, 0])), j
    assert bool(stats["converged"][0]) and bool(stats["converged"][4])


def test_nonfinite_direction_with_x0():
    """a column that breaks down later keeps its bits from the moment it froze, x0 given"""
    import torch
    import ilupp_amd.device as ild
    A = _csr(matgen.poisson3d(16))
    n = A.shape[0]
    dA = ild.DeviceCSR.from_scipy(A)
    B = torch.from_numpy(_rhs_columns(A, 5)[:, :3].copy()).cuda()
    x0 = torch.from_numpy(_block(n, 3, 6)).cuda()
    x0[3, 1] = float("inf")                       # r = b - A x0 holds Inf and NaN in column 1
    stats = {}
    X = ild.cg(dA, B, None, x0=x0, maxiter=50, stats=stats)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(X[:, 1].cpu().numpy()), _bits(x0[:, 1].cpu().numpy()))
    assert not bool(stats["converged"][1]) and int(stats["iterations"][1]) == 0
    assert stats["iterations"].tolist()[0] == 50 and stats["iterations"].tolist()[2] == 50


def test_block_solve_on_a_side_stream():
    import torch
    import ilupp_amd.device as ild
    A = _csr(matgen.poisson3d(40))
    dA = ild.DeviceCSR.from_scipy(A)
    M = ild.DevicePreconditioner("ICholT", dA, add_fill_in=5, threshold=1e-3)
    B = torch.from_numpy(_rhs_columns(A, 7)).cuda()
    X1 = ild.cg(dA, B, M, maxiter=200, rtol=1e-8, check_every=5)
    Y1 = ild.bicgstab(dA, B, M, maxiter=50, rtol=1e-8, check_every=5)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        X2 = ild.cg(dA, B, M, maxiter=200, rtol=1e-8, check_every=5)
        Y2 = ild.bicgstab(dA, B, M, maxiter=50, rtol=1e-8, check_every=5)
        Z2 = dA.matmat(B)
    s.synchronize()
    assert np.array_equal(_bits(X1.cpu().numpy()), _bits(X2.cpu().numpy()))
    assert np.array_equal(_bits(Y1.cpu().numpy()), _bits(Y2.cpu().numpy()))
    assert np.array_equal(_bits(Z2.cpu().numpy()), _bits((dA @ B).cpu().numpy()))
