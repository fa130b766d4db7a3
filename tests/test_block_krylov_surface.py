"""CPU tests of the k-column Krylov surface: the C ABI exports the SpMM, the block dot and the masked updates and refuses bad arguments
before any launch; DeviceCSR.matmat and the 2-D paths of cg / bicgstab check their input before any native call."""
import ctypes

import pytest

NEW_SYMBOLS = ("ilupp_hip_spmm_device", "ilupp_hip_block_dot_device", "ilupp_hip_cg_block_update_device",
               "ilupp_hip_bicgstab_block_update_device")
FAKE = 4096          # a non-null pointer that no call below may dereference: every one is refused before any launch


def test_library_exports_the_block_krylov_entries():
    from ilupp_amd import _native
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _native.ABI_SYMBOLS, name


def _spmm(n=4, nnz=4, X=FAKE, ldx=2, Y=FAKE * 4, ldy=2, k=2, data=FAKE, idx=FAKE, ptr=FAKE):
    from ilupp_amd import _native
    return _native.lib().ilupp_hip_spmm_device(data, idx, ptr, n, nnz, X, ldx, Y, ldy, k, None)


def test_spmm_refuses_bad_arguments():
    from ilupp_amd import _native
    lib = _native.lib()
    bad = [dict(data=None), dict(idx=None), dict(ptr=None), dict(X=None), dict(Y=None), dict(n=0), dict(n=-3), dict(nnz=-1),
           dict(k=-1), dict(ldx=1), dict(ldy=1), dict(Y=FAKE)]          # (the last: Y and X overlap)
    for kw in bad:
        assert _spmm(**kw) == -1, kw         # ILUPP_ERR_INVALID
        assert lib.ilupp_hip_last_error().decode().startswith("spmm:"), kw
    assert _spmm(k=0, ldx=0, ldy=0) == 0                                 # k = 0: nothing to do


def test_block_dot_refuses_bad_arguments():
    from ilupp_amd import _native
    lib = _native.lib()

    def dot(n=4, k=2, A=FAKE, lda=2, B=FAKE, ldb=2, out=FAKE):
        return lib.ilupp_hip_block_dot_device(n, k, A, lda, B, ldb, out, None)
    for kw in (dict(A=None), dict(B=None), dict(out=None), dict(n=0), dict(n=-1), dict(k=-2), dict(lda=1), dict(ldb=1)):
        assert dot(**kw) == -1, kw
        assert lib.ilupp_hip_last_error().decode().startswith("block dot:"), kw
    assert dot(k=0, lda=0, ldb=0) == 0


def test_updates_refuse_bad_arguments():
    from ilupp_amd import _native
    lib = _native.lib()
    cg = lib.ilupp_hip_cg_block_update_device
    assert cg(2, 4, 2, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None) == -1
    assert cg(0, 4, 2, None, FAKE, FAKE, FAKE, FAKE, FAKE, None) == -1
    assert cg(0, 4, 2, FAKE, FAKE, None, FAKE, FAKE, FAKE, None) == -1
    assert cg(0, 0, 2, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None) == -1
    assert cg(1, 4, -1, FAKE, FAKE, None, None, FAKE, FAKE, None) == -1
    assert cg(1, 4, 0, FAKE, FAKE, None, None, FAKE, FAKE, None) == 0
    bi = lib.ilupp_hip_bicgstab_block_update_device
    assert bi(3, 4, 2, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None) == -1
    assert bi(0, 4, 2, FAKE, FAKE, None, None, None, FAKE, None, None, FAKE, None, None) == -1     # s missing
    assert bi(1, 4, 2, FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE, None, None, None) == -1     # As missing
    assert bi(2, 4, 2, FAKE, None, None, FAKE, None, FAKE, FAKE, None, FAKE, None, None) == -1     # omega missing
    assert bi(2, -4, 2, FAKE, None, FAKE, FAKE, None, FAKE, FAKE, None, FAKE, None, None) == -1
    assert bi(2, 4, 0, FAKE, None, FAKE, FAKE, None, FAKE, FAKE, None, FAKE, None, None) == 0
    assert ctypes.sizeof(ctypes.c_void_p) == 8


class _Boom:
    """stands in for the native library: any call fails the test"""
    def __getattr__(self, name):
        raise AssertionError("native call %s before the argument checks" % name)


def _fake_csr(n):
    import ilupp_amd.device as ild
    A = ild.DeviceCSR.__new__(ild.DeviceCSR)
    A.n, A.nnz, A.shape = n, 3 * n, (n, n)
    return A


def test_matmat_and_block_solvers_exist():
    import inspect
    import ilupp_amd.device as ild
    assert callable(ild.DeviceCSR.matmat)
    assert "stats" in inspect.signature(ild.cg).parameters
    assert "stats" in inspect.signature(ild.bicgstab).parameters
    assert "history" in inspect.signature(ild.bicgstab).parameters


def test_matmat_checks_before_any_native_call(monkeypatch):
    import torch
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    A = _fake_csr(6)
    with pytest.raises(ValueError, match="rows"):
        A.matmat(torch.zeros((5, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="rows"):
        A.matmat(torch.zeros((6, 2, 1), dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        A.matmat(torch.zeros((6, 2), dtype=torch.float32))
    with pytest.raises(ValueError, match="row-major"):
        A.matmat(torch.zeros((2, 6), dtype=torch.float64).t())
    with pytest.raises(ValueError, match="CUDA"):
        A.matmat(torch.zeros((6, 2), dtype=torch.float64))
    # matvec and @ send 2-D input to matmat (and its checks)
    with pytest.raises(ValueError, match="float64"):
        A.matvec(torch.zeros((6, 2), dtype=torch.float32))
    with pytest.raises(ValueError, match="float64"):
        A @ torch.zeros((6, 2), dtype=torch.int64)


def test_block_solvers_check_before_any_native_call(monkeypatch):
    import torch
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    A = _fake_csr(6)
    for solve in (ild.cg, ild.bicgstab):
        with pytest.raises(ValueError, match="float64"):
            solve(A, torch.zeros((6, 2), dtype=torch.float32))
        with pytest.raises(ValueError, match="rows"):
            solve(A, torch.zeros((7, 2), dtype=torch.float64))
        with pytest.raises(ValueError, match="contiguous"):
            solve(A, torch.zeros((2, 6), dtype=torch.float64).t())
        with pytest.raises(ValueError, match="CUDA"):
            solve(A, torch.zeros((6, 2), dtype=torch.float64))


def test_multilevel_kind_refuses_a_block(monkeypatch):
    import torch
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    A = _fake_csr(4)
    M = ild.DevicePreconditioner.__new__(ild.DevicePreconditioner)
    M.kind, M.n, M.pr = "ILUpp", 4, None
    for solve in (ild.cg, ild.bicgstab):
        with pytest.raises(NotImplementedError):
            solve(A, torch.zeros((4, 2), dtype=torch.float64), M)
