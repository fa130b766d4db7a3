"""CPU tests of the batched construction of the two pivoting classes: the C ABI exports ilupp_hip_ilucp_create_batch / ilupp_hip_ilutp_create_batch
and refuses bad arguments before any HIP call; ILUCPPreconditioner.batch / ILUTPPreconditioner.batch check their input before any native
call; the compiled shim offers the same two functions."""
import ctypes
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

NEW_SYMBOLS = ("ilupp_hip_ilucp_create_batch", "ilupp_hip_ilutp_create_batch")


def _classes():
    import ilupp_amd as ilupp
    return ilupp.ILUCPPreconditioner, ilupp.ILUTPPreconditioner


def test_library_exports_the_batch_entries():
    from ilupp_amd import _native
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _native.ABI_SYMBOLS, name


def test_classes_have_a_batch_classmethod():
    for cls in _classes():
        assert inspect.ismethod(cls.batch) and cls.batch.__self__ is cls
        assert str(inspect.signature(cls.batch)) == "(matrices, fill_in=100, threshold=0.1, piv_tol=0.1, mem_factor=10.0)"


class _Boom:
    """stands in for the native library: any call fails the test"""
    def __getattr__(self, name):
        raise AssertionError("native call %s before the argument checks" % name)


def test_batch_checks_its_input_before_any_native_call(monkeypatch):
    from ilupp_amd import _native
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    A = sp.eye(4, format="csr")
    for cls in _classes():
        assert cls.batch([]) == []
        assert cls.batch(iter(())) == []
        with pytest.raises(TypeError, match="a batch holds matrices of one format"):
            cls.batch([A, A.tocsc()])
        with pytest.raises(TypeError, match="A must be a csr_matrix or a csc_matrix"):
            cls.batch([A, sp.eye(4, format="coo")])
        with pytest.raises(ValueError, match="A must be a square matrix!"):
            cls.batch([A, sp.csr_matrix(np.ones((2, 3)))])


def test_pybind_module_has_both_batch_functions():
    from ilupp_amd import _ilupp_hip as m
    for name in ("ILUCPPreconditioner_batch", "ILUTPPreconditioner_batch"):
        assert callable(getattr(m, name)), name
    assert m.ILUCPPreconditioner_batch([], True, 100, 0.1, 0.1, -1, 10.0) == []
    assert m.ILUTPPreconditioner_batch([], False, 100, 0.1, 0.1, -1, 10.0) == []


def test_library_refuses_bad_arguments_before_any_device_call():
    from ilupp_amd import _native
    lib = _native.lib()
    VP = ctypes.c_void_p
    d, i, p = np.ones(2), np.arange(2, dtype=np.int32), np.arange(3, dtype=np.int32)
    D, I, P = (VP * 1)(d.ctypes.data), (VP * 1)(i.ctypes.data), (VP * 1)(p.ctypes.data)
    N = (ctypes.c_int32 * 1)(2)
    out, status = (VP * 1)(), (ctypes.c_int32 * 1)()
    tail = (1, 100, 0.1, 0.1, -1, 10.0)
    for name in NEW_SYMBOLS:
        f = getattr(lib, name)
        for args in ((1, None, I, P, N), (1, D, None, P, N), (1, D, I, None, N), (1, D, I, P, None), (-1, D, I, P, N)):
            assert f(*args, *tail, out, status) == -1, (name, args)            # ILUPP_ERR_INVALID
            assert lib.ilupp_hip_last_error().decode() == "null argument"
        assert f(1, D, I, P, N, *tail, None, status) == -1
        assert f(0, D, I, P, N, *tail, out, status) == 0                       # nothing to do: the device is not touched
        assert f(0, D, I, P, N, *tail, out, None) == 0
