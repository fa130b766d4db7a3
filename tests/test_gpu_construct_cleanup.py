"""A construction that fails through one of its documented error returns gives back every pool block it took: ilupp_hip_live_blocks()
reads the same after the exception as before it, through the host entry and through the device entry where one exists."""
import gc

import numpy as np
import pytest
import scipy.sparse as sp

import golden_util as G
import matgen

pytestmark = pytest.mark.gpu


def _missing_diagonal(kind):
    """3 x 3, row 1 without its diagonal entry (test_gpu_parity.py, test_missing_diagonal_is_reported)"""
    A = sp.csr_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 2.0]]))
    return (A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32), True), "%s: structurally missing diagonal entry in row 1" % kind


def _not_positive_definite():
    """a box grid whose one negative pivot ends ICholT's grid path (test_gpu_icholt_grid.py, test_not_positive_definite_reports_as_before)"""
    d, i, p = matgen.poisson3d(64, 48, 40)
    d = d.copy()
    r = 5 * 64 * 48 + 7 * 64 + 9
    d[p[r] + int(np.flatnonzero(i[p[r]:p[r + 1]] == r)[0])] = -1.0
    return (d, i, p, True), "not positive definite"


def _ilut_zero_pivot():
    z = G.load("edges.npz")
    return G.get_mat(z, "zeropivot/A"), "ILUT_heap: encountered zero pivot in row %d" % int(z["zeropivot/err_row"])


def _iluc_zero_pivot():
    z = G.load("iluc.npz")
    code, row = (int(v) for v in z["edge_nopivot/iluc_5_0.1_error"])
    assert code == 1
    return G.get_mat(z, "edge_nopivot/A"), "zero pivot on diagonal, k=%d" % row


def _small_grid(match):
    """ILUC with no fill allowed, ILUTP with mem_factor 1: the reservation is too small (the oracle fails the same way)"""
    d, i, p = matgen.poisson3d(5)
    return (d, i, p, True), match


def _host(name, *extra):
    def run(M):
        from ilupp_amd import _native
        return getattr(_native, name)(M[0], M[1], M[2], M[3], *extra)
    return run


def _device(name, *extra, **kw):
    def run(M):
        import torch
        from ilupp_amd import _native
        t = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (M[0].astype(np.float64), M[1].astype(np.int32), M[2].astype(np.int32))]
        torch.cuda.synchronize()
        return getattr(_native, name + "_device")(*[x.data_ptr() for x in t], M[2].shape[0] - 1, M[3], *extra, **kw)
    return run


def _ilu0():
    return _missing_diagonal("ILU0")


def _ichol0():
    return _missing_diagonal("IChol0")


def _iluc_memory():
    return _small_grid("insufficient memory reserved")


def _ilutp_memory():
    return _small_grid("memory reserved was insufficient")


CASES = [
    ("ilu0-missing-diagonal-host", _host("ILU0Preconditioner"), _ilu0),
    ("ilu0-missing-diagonal-device", _device("ILU0Preconditioner"), _ilu0),
    ("ilu0-missing-diagonal-device-nnz", _device("ILU0Preconditioner", nnz=6), _ilu0),
    ("ichol0-missing-diagonal-host", _host("IChol0Preconditioner"), _ichol0),
    ("ichol0-missing-diagonal-device", _device("IChol0Preconditioner"), _ichol0),
    ("icholt-not-spd-host", _host("ICholTPreconditioner", 0, 0.0), _not_positive_definite),
    ("icholt-not-spd-device", _device("ICholTPreconditioner", 0, 0.0), _not_positive_definite),
    ("ilut-zero-pivot-host", _host("ILUTPreconditioner", 100, 0.0), _ilut_zero_pivot),
    ("ilut-zero-pivot-device", _device("ILUTPreconditioner", 100, 0.0), _ilut_zero_pivot),
    ("iluc-zero-pivot-host", _host("ILUCPreconditioner", 5, 0.1), _iluc_zero_pivot),
    ("iluc-zero-pivot-device", _device("ILUCPreconditioner", 5, 0.1), _iluc_zero_pivot),
    ("iluc-memory-host", _host("ILUCPreconditioner", 0, 0.0), _iluc_memory),
    ("iluc-memory-device", _device("ILUCPreconditioner", 0, 0.0), _iluc_memory),
    ("ilutp-memory-host", _host("ILUTPPreconditioner", 100, 0.0, 0.1, -1, 1.0), _ilutp_memory),
]


@pytest.mark.parametrize("construct,make", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_failed_construction_leaves_no_block(construct, make):
    from ilupp_amd import _native
    M, match = make()
    # (a first run: what the process sets up once, on first use, is no leak)
    with pytest.raises(RuntimeError, match=match):
        construct(M)
    gc.collect()
    before = _native.live_blocks()
    with pytest.raises(RuntimeError, match=match):
        construct(M)
    gc.collect()
    assert _native.live_blocks() == before
