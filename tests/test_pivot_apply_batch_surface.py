"""CPU tests of the batched apply of the two pivoting classes: the C ABI exports ilupp_hip_ilucp_apply_device, ilupp_hip_pivot_apply_batch_device
and ilupp_hip_pivot_apply_batch and refuses bad arguments before any HIP call; ilupp_amd.apply_batch checks its input before any native call;
the compiled shim offers the function; the classes the block apply leaves out still have scipy's column loop.  (A wrong vector length needs
a constructed member to compare with: the library's refusal of it is in tests/test_gpu_pivot_apply_batch.py, the Python layer's is here.)"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import LinearOperator

NEW_SYMBOLS = ("ilupp_hip_ilucp_apply_device", "ilupp_hip_pivot_apply_batch_device", "ilupp_hip_pivot_apply_batch")
LOOPED = ("ILUppPreconditioner", "ILUTPPreconditioner", "ILUCPPreconditioner")
INVALID = -1        # ILUPP_ERR_INVALID


def test_library_exports_the_three_entries():
    from ilupp_amd import _native
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _native.ABI_SYMBOLS, name


def test_library_refuses_bad_arguments_before_any_device_call():
    from ilupp_amd import _native
    lib = _native.lib()
    VP = ctypes.c_void_p
    x = np.ones(4)
    fake = VP(x.ctypes.data)             # stands in for a device pointer: never dereferenced by a refused call
    one_null = (VP * 1)()                # a member list whose only member is NULL
    off = (ctypes.c_int64 * 1)(0)
    X, N = (VP * 1)(x.ctypes.data), (ctypes.c_int64 * 1)(4)
    route = (ctypes.c_int32 * 1)()
    # the single device apply
    assert lib.ilupp_hip_ilucp_apply_device(None, fake, 4, 0, 1) == INVALID
    assert lib.ilupp_hip_last_error().decode() == "null preconditioner"
    # the device batch: null lists, a negative count, a null member
    f = lib.ilupp_hip_pivot_apply_batch_device
    for args in ((1, None, fake, off), (1, one_null, None, off), (1, one_null, fake, None), (-1, one_null, fake, off)):
        assert f(*args, 0, 1, route) == INVALID, args
        assert lib.ilupp_hip_last_error().decode() == "null argument"
    assert f(1, one_null, fake, off, 0, 1, route) == INVALID
    assert lib.ilupp_hip_last_error().decode() == "null preconditioner"
    assert f(0, one_null, fake, off, 0, 1, route) == 0                     # nothing to do: the device is not touched
    assert f(0, one_null, fake, off, 1, 0, None) == 0
    # the host batch
    g = lib.ilupp_hip_pivot_apply_batch
    for args in ((1, None, X, N), (1, one_null, None, N), (1, one_null, X, None), (-1, one_null, X, N)):
        assert g(*args, 0, route) == INVALID, args
        assert lib.ilupp_hip_last_error().decode() == "null argument"
    assert g(1, one_null, X, N, 0, route) == INVALID
    assert lib.ilupp_hip_last_error().decode() == "null preconditioner"
    assert g(0, one_null, X, N, 0, route) == 0
    assert g(0, one_null, X, N, 1, None) == 0
    assert np.array_equal(x, np.ones(4))


class _Boom:
    """stands in for the native library: any call fails the test"""
    def __getattr__(self, name):
        raise AssertionError("native call %s before the argument checks" % name)


def _unbuilt(cls, n):
    """an instance of a pivoting class of dimension n without a native object behind it"""
    P = cls.__new__(cls)
    P.pr = _Boom()
    LinearOperator.__init__(P, dtype=np.float64, shape=(n, n))
    return P


def test_apply_batch_checks_its_input_before_any_native_call(monkeypatch):
    import ilupp_amd as ilupp
    from ilupp_amd import _native
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    monkeypatch.setattr(_native, "pivot_apply_batch", lambda *a: (_ for _ in ()).throw(AssertionError("native call before the argument checks")))
    assert ilupp.apply_batch([], []) == []
    assert ilupp.apply_batch(iter(()), iter(()), transpose=True) == []
    P4, Q3 = _unbuilt(ilupp.ILUCPPreconditioner, 4), _unbuilt(ilupp.ILUTPPreconditioner, 3)
    with pytest.raises(TypeError, match="ILUCPPreconditioner / ILUTPPreconditioner"):
        ilupp.apply_batch([P4, _unbuilt(ilupp.ILUTPreconditioner, 4)], [np.ones(4), np.ones(4)])
    with pytest.raises(TypeError, match="ILUCPPreconditioner / ILUTPPreconditioner"):
        ilupp.apply_batch([sp.eye(4, format="csr")], [np.ones(4)])
    with pytest.raises(ValueError, match="2 preconditioners but 1 vectors"):
        ilupp.apply_batch([P4, Q3], [np.ones(4)])
    with pytest.raises(ValueError, match="vector of 4 elements for a preconditioner of dimension 3"):
        ilupp.apply_batch([P4, Q3], [np.ones(4), np.ones(4)])


def test_native_layer_has_the_entries():
    from ilupp_amd import _native
    assert callable(_native.pivot_apply_batch) and callable(_native.pivot_apply_batch_device)
    assert callable(_native.PivotedPreconditioner.apply_device)
    assert _native.pivot_apply_batch([], [], False) == []
    with pytest.raises(ValueError):
        _native.pivot_apply_batch([], [np.ones(2)], False)
    with pytest.raises(TypeError):
        _native.pivot_apply_batch([object()], [np.ones(2)], False)


def test_pybind_module_has_the_function():
    from ilupp_amd import _ilupp_hip as m
    assert callable(m.pivot_apply_batch)
    assert m.pivot_apply_batch([], [], False) == []
    with pytest.raises(ValueError):
        m.pivot_apply_batch([], [np.ones(2)], True)
    with pytest.raises(TypeError):
        m.pivot_apply_batch([object()], [np.ones(2)], False)


def test_looped_classes_keep_the_column_loop():
    import ilupp_amd as ilupp
    for name in LOOPED:
        cls = getattr(ilupp, name)
        assert cls._matmat is LinearOperator._matmat, name
        assert cls._rmatmat is LinearOperator._rmatmat, name
        assert not hasattr(cls, "apply_block"), name
