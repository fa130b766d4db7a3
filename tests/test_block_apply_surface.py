"""CPU tests of the block apply's surface (k right-hand sides per call): the C ABI exports it, the five single-factorisation classes route
P @ X through it, the multilevel and pivoting classes keep scipy's column loop, and the bindings check their buffers before any GPU
call."""
import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator

BLOCK_SYMBOLS = ("ilupp_hip_apply_block", "ilupp_hip_apply_block_device", "ilupp_hip_block_path")
FIVE = ("ILU0Preconditioner", "ILUTPreconditioner", "ILUCPreconditioner", "IChol0Preconditioner", "ICholTPreconditioner")
LOOPED = ("ILUppPreconditioner", "ILUTPPreconditioner", "ILUCPPreconditioner")


def test_library_exports_the_block_entries():
    from ilupp_amd import _native
    lib = _native.lib()
    for name in BLOCK_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _native.ABI_SYMBOLS, name


def test_five_classes_define_matmat():
    import ilupp_amd as ilupp
    for name in FIVE:
        cls = getattr(ilupp, name)
        assert cls._matmat is not LinearOperator._matmat, name
        assert cls._rmatmat is not LinearOperator._rmatmat, name


def test_out_of_scope_classes_keep_the_column_loop():
    import ilupp_amd as ilupp
    for name in LOOPED:
        cls = getattr(ilupp, name)
        assert cls._matmat is LinearOperator._matmat, name
        assert cls._rmatmat is LinearOperator._rmatmat, name


def test_bindings_have_apply_block():
    from ilupp_amd import _ilupp_hip as m
    from ilupp_amd import _native
    for member in ("apply_block", "apply_block_device", "block_path"):
        assert callable(getattr(_native.Preconditioner, member, None)), member
    for cls in (m.GenericLUPreconditioner, m.GenericLLTPreconditioner, m.ILUTPreconditioner, m.ILUCPreconditioner):
        assert hasattr(cls, "apply_block") and hasattr(cls, "apply_block_trans"), cls
    for cls in (m.ILUTPPreconditioner, m.ILUCPPreconditioner, m.MultilevelILUCDPPreconditioner):
        assert not hasattr(cls, "apply_block"), cls
    assert not hasattr(_native.MultilevelPreconditioner, "apply_block")
    assert not hasattr(_native.PivotedPreconditioner, "apply_block")


def test_ctypes_block_buffer_checks():
    """the checks run before the native call (the handle is never touched)"""
    from ilupp_amd import _native
    P = _native.Preconditioner(None)
    with pytest.raises(RuntimeError, match="Expected 2D array for b!"):
        P.apply_block(np.zeros(4))
    with pytest.raises(RuntimeError, match="Expected contiguous array for b!"):
        P.apply_block(np.zeros((4, 3), order="F"))
    with pytest.raises(RuntimeError, match=r"Expected d \(d\) array for b, got f!"):
        P.apply_block(np.zeros((4, 3), dtype=np.float32))
    ro = np.zeros((4, 3))
    ro.flags.writeable = False
    with pytest.raises(RuntimeError, match="b must be writable"):
        P.apply_block(ro)


def test_null_object_is_refused_by_the_library():
    from ilupp_amd import _native
    lib = _native.lib()
    X = np.zeros((4, 2))
    assert lib.ilupp_hip_apply_block(None, X.ctypes.data, 4, 2, 0) != 0
    assert lib.ilupp_hip_apply_block_device(None, X.ctypes.data, 4, 2, 0, 1) != 0
    assert lib.ilupp_hip_block_path(None) == b""


def test_device_multilevel_refuses_a_block():
    """the "ILUpp" kind of DevicePreconditioner: 2-D input is refused before any native call"""
    import torch
    import ilupp_amd.device as ild
    M = ild.DevicePreconditioner.__new__(ild.DevicePreconditioner)
    M.kind, M.n, M.pr = "ILUpp", 4, None
    with pytest.raises(NotImplementedError):
        M.apply_(torch.zeros((4, 2), dtype=torch.float64))
