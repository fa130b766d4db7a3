"""The block apply (k right-hand sides per call: ilupp_hip_apply_block*, sptrsm_lvl.hip): P @ X, P.T @ X and DevicePreconditioner.apply_
on an (n, k) block must give, column by column, the bits of P @ X[:, j] -- and of the reference's apply of that column.  "Equal" is
bitwise (uint64 views, so NaN columns count too).  The routes: the level-ordered objects (ILUT, ILUC, ICholT with fill, ILU(0) of long-row
matrices) walk their records once per chunk of columns ("block:level"); the static sweeps of box grids and small or degenerate objects
apply column by column ("block:columns")."""
import numpy as np
import pytest
import scipy.sparse as sp

import golden_util as G
import matgen

pytestmark = pytest.mark.gpu

KS = (1, 2, 7, 8, 9, 16, 33)


def _oracle():
    from oracle import oracle as O
    return O, (O.ref() if O.ref_available() else O.orc())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _block(n, k, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, k))
    X[:, 0] = G.rhs(n)
    if k > 3:
        X[n // 3, 3] = np.nan          # a NaN column: its canonical NaNs must come out where the single apply puts them
    return X


def _matrix(case, fmt):
    if case == "ilu0_9pt":
        d, i, p = matgen.box_stencil((512, 512))
    elif case == "ilu0_holes":
        d, i, p = matgen.mesh_with_holes(64)
    elif case == "ilut":
        d, i, p = matgen.random_dd(200000)
    else:
        d, i, p = matgen.poisson3d(64)
    n = p.shape[0] - 1
    A = sp.csr_matrix((d, i, p), shape=(n, n))
    return A if fmt == "csr" else A.tocsc()


def _make(case, A):
    import ilupp_amd as ilupp
    if case.startswith("ilu0"):
        return ilupp.ILU0Preconditioner(A)
    if case == "ilut":
        return ilupp.ILUTPreconditioner(A, fill_in=10, threshold=1e-4)
    if case == "iluc":
        return ilupp.ILUCPreconditioner(A, fill_in=8, threshold=1e-2)
    if case == "ichol0":
        return ilupp.IChol0Preconditioner(A)
    if case == "icholt0":
        return ilupp.ICholTPreconditioner(A, add_fill_in=0, threshold=0.0)
    return ilupp.ICholTPreconditioner(A, add_fill_in=5, threshold=1e-3)


LEVEL_ROUTE = {"ilu0_9pt", "ilut", "iluc", "icholt5"}
COLUMNS_ROUTE = {"ilu0_7pt"}


def _reference_columns(case, A, fmt, X):
    """the reference's factors of A and its apply of every column of X: (ID, TRANSPOSE) blocks, or None for ILUC / IChol0"""
    O, ref = _oracle()
    M = (A.data, A.indices, A.indptr, fmt == "csr")
    if case.startswith("ilu0") or case == "ilut":
        Lo, Uo = ref.ilu0(M) if case.startswith("ilu0") else ref.ilut(M, 10, 1e-4)
        ap = lambda x, use: ref.apply_lu(Lo, Uo, x, use)
    elif case in ("icholt0", "icholt5"):
        Lo = ref.icholt(M, 0, 0.0) if case == "icholt0" else ref.icholt(M, 5, 1e-3)
        ap = lambda x, use: ref.apply_llt(Lo, x, use)
    else:
        return None
    return (np.column_stack([ap(X[:, j], O.ID) for j in range(X.shape[1])]),
            np.column_stack([ap(X[:, j], O.TRANSPOSE) for j in range(X.shape[1])]))


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("case", ["ilu0_9pt", "ilu0_holes", "ilu0_7pt", "ilut", "iluc", "ichol0", "icholt0", "icholt5"])
def test_block_equals_columns(case, fmt):
    A = _matrix(case, fmt)
    n = A.shape[0]
    P = _make(case, A)
    X = _block(n, max(KS))
    single = np.column_stack([P @ X[:, j] for j in range(X.shape[1])])
    single_t = np.column_stack([P.T @ X[:, j] for j in range(X.shape[1])])
    for k in KS:
        Xk = X[:, :k].copy()
        Y = P @ Xk
        assert np.array_equal(_bits(Xk), _bits(X[:, :k])), "P @ X changed X"
        assert Y.shape == (n, k)
        assert np.array_equal(_bits(Y), _bits(single[:, :k])), ("P @ X", k)
        assert np.array_equal(_bits(P.matmat(Xk)), _bits(Y))        # (scipy sends an (n, 1) block of P @ X to matvec, matmat never)
        path = P.pr.block_path()
        if k == 1:
            assert path == "block:columns"
        elif case in LEVEL_ROUTE:
            assert path == "block:level", (k, path)
        elif case in COLUMNS_ROUTE:
            assert path == "block:columns", (k, path)
        Yt = P.T @ Xk
        assert np.array_equal(_bits(Yt), _bits(single_t[:, :k])), ("P.T @ X", k)
        assert np.array_equal(_bits(P.T.matmat(Xk)), _bits(Yt))
    want = _reference_columns(case, A, fmt, X[:, :9])
    if want is not None:
        assert np.array_equal(_bits(single[:, :9]), _bits(want[0]))
        assert np.array_equal(_bits(single_t[:, :9]), _bits(want[1]))


def test_reference_test_matrix_takes_the_columns_route():
    import ilupp_amd as ilupp
    O, ref = _oracle()
    z = G.load("reftests.npz")
    for fmt in ("csr", "csc"):
        d, i, p, is_csr = G.get_mat(z, "laplace2d_%s/A" % fmt)
        n = p.shape[0] - 1
        A = (sp.csr_matrix if is_csr else sp.csc_matrix)((d, i, p), shape=(n, n))
        assert n < 1024
        for P in (ilupp.ILU0Preconditioner(A), ilupp.ILUTPreconditioner(A, fill_in=10, threshold=1e-4)):
            X = _block(n, 9)
            Y, Yt = P @ X, P.T @ X
            assert P.pr.block_path() == "block:columns"
            assert np.array_equal(_bits(Y), _bits(np.column_stack([P @ X[:, j] for j in range(9)])))
            assert np.array_equal(_bits(Yt), _bits(np.column_stack([P.T @ X[:, j] for j in range(9)])))
        Lo, Uo = ref.ilu0((A.data, A.indices, A.indptr, is_csr))
        P = ilupp.ILU0Preconditioner(A)
        X = _block(n, 9)
        want = np.column_stack([ref.apply_lu(Lo, Uo, X[:, j], O.ID) for j in range(9)])
        assert np.array_equal(_bits(P @ X), _bits(want))


def test_host_block_staged_in_pieces():
    """more columns than one staging piece holds (n = 2 * 10^5: 160 per piece): every column as its single apply"""
    import ilupp_amd as ilupp
    A = _matrix("ilut", "csr")
    n = A.shape[0]
    P = ilupp.ILUTPreconditioner(A, fill_in=10, threshold=1e-4)
    X = _block(n, 170, seed=8)
    Y = P @ X
    assert P.pr.block_path() == "block:level"
    for j in list(range(0, 170, 13)) + [159, 160, 169]:
        assert np.array_equal(_bits(Y[:, j]), _bits(P @ X[:, j])), j
    assert P.pr.timings()["last_apply_ms"] > 0.0


def test_pybind_shim_block_apply():
    from ilupp_amd import _ilupp_hip as m
    import ilupp_amd as ilupp
    A = _matrix("ilut", "csr")
    n = A.shape[0]
    P = ilupp.ILUTPreconditioner(A, fill_in=10, threshold=1e-4)
    f = m.ILUTPreconditioner(A.data, A.indices, A.indptr, True, 10, 1e-4)
    X = _block(n, 9)
    Y = X.copy(); f.apply_block(Y)
    Yt = X.copy(); f.apply_block_trans(Yt)
    assert np.array_equal(_bits(Y), _bits(P @ X))
    assert np.array_equal(_bits(Yt), _bits(P.T @ X))
    with pytest.raises(RuntimeError, match="vector has wrong size for preconditioner!"):
        f.apply_block(np.zeros((n + 1, 2)))


@pytest.mark.parametrize("kind", ["ILUT", "ILU0", "ICholT"])
def test_device_block_apply(kind):
    import torch
    import ilupp_amd.device as ild
    A = _matrix("ilut", "csr") if kind == "ILUT" else sp.csr_matrix(matgen.box_stencil((256, 256))) if kind == "ILU0" else _matrix("icholt5", "csr")
    n = A.shape[0]
    dA = ild.DeviceCSR.from_scipy(A)
    params = {"ILUT": {"fill_in": 10, "threshold": 1e-4}, "ICholT": {"add_fill_in": 5, "threshold": 1e-3}}.get(kind, {})
    M = ild.DevicePreconditioner(kind, dA, **params)
    X = torch.from_numpy(_block(n, 9)).cuda()
    for transpose in (False, True):
        Xb = X.clone()
        M.apply_(Xb, transpose=transpose)
        cols = [X[:, j].contiguous() for j in range(9)]
        for c in cols:
            M.apply_(c, transpose=transpose)
        Y2 = (M @ X) if not transpose else None
        M.sync()
        want = torch.stack(cols, dim=1).cpu().numpy()
        assert np.array_equal(_bits(Xb.cpu().numpy()), _bits(want)), transpose
        if Y2 is not None:
            assert np.array_equal(_bits(Y2.cpu().numpy()), _bits(want))
        assert M.pr.block_path() == "block:level"
    # 1-D: the same as before, and what the host object gives
    import ilupp_amd as ilupp
    P = {"ILUT": lambda: ilupp.ILUTPreconditioner(A, fill_in=10, threshold=1e-4), "ILU0": lambda: ilupp.ILU0Preconditioner(A),
         "ICholT": lambda: ilupp.ICholTPreconditioner(A, add_fill_in=5, threshold=1e-3)}[kind]()
    x = X[:, 1].contiguous()
    y = M @ x
    M.sync()
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(P @ X[:, 1].cpu().numpy()))
    # k = 0 and a wrong n
    E = torch.empty((n, 0), dtype=torch.float64, device="cuda")
    assert M.apply_(E).shape == (n, 0)
    with pytest.raises(RuntimeError, match="vector has wrong size for preconditioner!"):
        M.pr.apply_block_device(X.data_ptr(), n + 1, 2)
    M.sync()


def test_edge_cases():
    import ilupp_amd as ilupp
    A = _matrix("ilut", "csr")
    n = A.shape[0]
    P = ilupp.ILUTPreconditioner(A, fill_in=10, threshold=1e-4)
    X = _block(n, 8)
    with pytest.raises(RuntimeError, match="vector has wrong size for preconditioner!"):
        P.pr.apply_block(np.zeros((n + 1, 3)))
    assert (P @ np.zeros((n, 0))).shape == (n, 0)
    Y = P @ X
    # Fortran order: as matvec takes any layout; float32: refused with the message matvec gives
    assert np.array_equal(_bits(P @ np.asfortranarray(X)), _bits(Y))
    with pytest.raises(RuntimeError, match=r"Expected d \(d\) array for b, got f!"):
        P @ X[:, 0].astype(np.float32)
    with pytest.raises(RuntimeError, match=r"Expected d \(d\) array for b, got f!"):
        P @ X.astype(np.float32)
    # the caller's array stays as it was
    X0 = X.copy()
    P @ X
    P.T @ X
    assert np.array_equal(_bits(X), _bits(X0))


def test_unchanged_objects_keep_the_column_loop():
    import ilupp_amd as ilupp
    d, i, p = matgen.poisson2d(20)
    n = p.shape[0] - 1
    A = sp.csr_matrix((d, i, p), shape=(n, n))
    X = _block(n, 5)
    for P in (ilupp.ILUppPreconditioner(A), ilupp.ILUTPPreconditioner(A, fill_in=10, threshold=1e-4),
              ilupp.ILUCPPreconditioner(A, fill_in=10, threshold=1e-4)):
        Y = P @ X
        assert np.array_equal(_bits(Y), _bits(np.column_stack([P @ X[:, j] for j in range(5)]))), type(P).__name__
        Yt = P.T @ X
        assert np.array_equal(_bits(Yt), _bits(np.column_stack([P.T @ X[:, j] for j in range(5)]))), type(P).__name__
