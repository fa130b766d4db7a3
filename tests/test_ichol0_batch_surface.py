"""CPU tests of the batched IChol(0) surface: the C ABI exports and declares the five entries and refuses bad arguments before any HIP call;
ilupp_amd.device.ichol0_batch / ichol0_refactor_ / ichol0_refactor_batch_ check their input before any native call; empty batches return
empty lists; the host classmethod exists.  (The refusals that need a built member are in tests/test_gpu_ichol0_batch.py.)"""
import ctypes
import os

import numpy as np
import pytest

INVALID = -1        # ILUPP_ERR_INVALID
VP = ctypes.c_void_p
SYMBOLS = ("ilupp_hip_ichol0_refactor_device", "ilupp_hip_ichol0_refactor_batch_device", "ilupp_hip_ichol0_refactor_batch_max_n",
           "ilupp_hip_ichol0_create_batch", "ilupp_hip_ichol0_create_batch_device")


def test_library_exports_and_header_declares_the_entries():
    from ilupp_amd import _native
    lib = _native.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ilupp_hip.h")).read()
    for symbol in SYMBOLS:
        assert hasattr(lib, symbol)
        assert symbol in _native.ABI_SYMBOLS
        assert symbol + "(" in header
    for name in ("ichol0_refactor_batch_device", "ichol0_refactor_batch_max_n", "IChol0Preconditioner_batch", "IChol0Preconditioner_batch_device"):
        assert callable(getattr(_native, name)), name
    assert callable(_native.Preconditioner.ichol0_refactor_device)


def _member(n=4):
    """stands in for a handle: zeroed host memory whose third word is the dimension (see tests/test_refactor_batch_surface.py); kind 0 is
    an LU object, so a refused call reads of it only that it is no IChol(0) object"""
    m = (ctypes.c_int32 * 16384)()
    m[2] = n
    return m


def _args(**kw):
    x = np.ones(4)
    fake = VP(x.ctypes.data)
    member = _member()
    a = dict(count=1, members=(VP * 1)(ctypes.addressof(member)), data=(VP * 1)(fake), indices=(VP * 1)(fake), indptr=(VP * 1)(fake),
             nnz=(ctypes.c_int64 * 1)(4), status=fake, sync=1, route=(ctypes.c_int32 * 1)())
    a.update(kw)
    a["_keep"] = (x, member)
    return a


def _call(lib, a):
    order = ("count", "members", "data", "indices", "indptr", "nnz", "status", "sync", "route")
    return lib.ilupp_hip_ichol0_refactor_batch_device(*[a[k] for k in order])


def test_refactor_entries_refuse_bad_arguments_before_any_device_call():
    from ilupp_amd import _native
    lib = _native.lib()
    err = lambda: lib.ilupp_hip_last_error().decode()
    for name in ("members", "data", "indices", "indptr", "nnz", "status"):
        assert _call(lib, _args(**{name: None})) == INVALID, name
        assert err() == "null argument", name
    for name in ("data", "indices", "indptr"):
        assert _call(lib, _args(**{name: (VP * 1)()})) == INVALID, name
        assert err() == "null argument", name
    assert _call(lib, _args(count=-1)) == INVALID
    assert err() == "null argument"
    assert _call(lib, _args(members=(VP * 1)())) == INVALID
    assert err() == "null preconditioner"
    a = _args()
    two = (VP * 2)(a["members"][0], a["members"][0])
    lists = {k: (VP * 2)(a[k][0], a[k][0]) for k in ("data", "indices", "indptr")}
    b = _args(count=2, members=two, nnz=(ctypes.c_int64 * 2)(4, 4), route=(ctypes.c_int32 * 2)(), _keep2=a, **lists)
    assert _call(lib, b) == INVALID
    assert err() == "a preconditioner appears twice in the batch"
    a = _args()
    assert _call(lib, a) == INVALID
    assert err() == "member 0 of the batch: not an IChol(0) object"
    assert np.array_equal(a["_keep"][0], np.ones(4)) and a["route"][0] == 0          # a refused call writes nothing
    assert _call(lib, _args(count=0)) == 0
    assert _call(lib, _args(count=0, sync=0, route=None)) == 0
    # the single entry: null arguments, and zeroed memory is no IChol(0) object
    fake = a["data"][0]
    assert lib.ilupp_hip_ichol0_refactor_device(None, fake, fake, fake) == INVALID and err() == "null argument"
    assert lib.ilupp_hip_ichol0_refactor_device(a["members"][0], None, fake, fake) == INVALID and err() == "null argument"
    assert lib.ilupp_hip_ichol0_refactor_device(a["members"][0], fake, fake, fake) == INVALID and err() == "not an IChol(0) object"


def test_create_entries_refuse_bad_arguments_before_any_device_call():
    from ilupp_amd import _native
    lib = _native.lib()
    err = lambda: lib.ilupp_hip_last_error().decode()
    x = np.ones(4)
    one = (VP * 1)(VP(x.ctypes.data))
    n, nnz, out = (ctypes.c_int32 * 1)(4), (ctypes.c_int64 * 1)(4), (VP * 1)()
    assert lib.ilupp_hip_ichol0_create_batch(1, None, one, one, n, 1, out, None, None) == INVALID and err() == "null argument"
    assert lib.ilupp_hip_ichol0_create_batch(1, one, one, one, n, 1, None, None, None) == INVALID and err() == "null argument"
    assert lib.ilupp_hip_ichol0_create_batch(-1, one, one, one, n, 1, out, None, None) == INVALID and err() == "null argument"
    assert lib.ilupp_hip_ichol0_create_batch(1, (VP * 1)(), one, one, n, 1, out, None, None) == INVALID and err() == "null argument"
    assert lib.ilupp_hip_ichol0_create_batch_device(1, one, one, one, n, None, 1, out, None, None) == INVALID and err() == "null argument"
    assert lib.ilupp_hip_ichol0_create_batch_device(1, one, (VP * 1)(), one, n, nnz, 1, out, None, None) == INVALID and err() == "null argument"
    assert lib.ilupp_hip_ichol0_create_batch(0, one, one, one, n, 1, out, None, None) == 0
    assert lib.ilupp_hip_ichol0_create_batch_device(0, one, one, one, n, nnz, 1, out, None, None) == 0
    assert _native.IChol0Preconditioner_batch([], True) == [] and _native.IChol0Preconditioner_batch_device([], True) == []
    assert _native.ichol0_refactor_batch_device([], [], None) == []
    with pytest.raises(ValueError, match="1 preconditioners but 0 matrices"):
        _native.ichol0_refactor_batch_device([_native.Preconditioner(None)], [], None)


class _Boom:
    """stands in for the native library: any call fails the test"""
    def __getattr__(self, name):
        raise AssertionError("native call %s before the argument checks" % name)


def _boom(monkeypatch):
    from ilupp_amd import _native
    fail = lambda *a, **k: (_ for _ in ()).throw(AssertionError("native call before the argument checks"))
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    for name in ("ichol0_refactor_batch_device", "IChol0Preconditioner_batch_device", "IChol0Preconditioner_batch", "set_caller_stream"):
        monkeypatch.setattr(_native, name, fail)
    monkeypatch.setattr(_native.Preconditioner, "ichol0_refactor_device", fail)


def _fake_csr(n):
    import ilupp_amd.device as ild
    A = ild.DeviceCSR.__new__(ild.DeviceCSR)
    A.n, A.nnz, A.shape = n, 3 * n, (n, n)
    return A


def _unbuilt(kind, n):
    """a DevicePreconditioner of dimension n without a factorisation behind it"""
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    M = ild.DevicePreconditioner.__new__(ild.DevicePreconditioner)
    M.kind, M.n, M.shape = kind, n, (n, n)
    M.pr = _native.MultilevelPreconditioner.__new__(_native.MultilevelPreconditioner) if kind == "ILUpp" else _native.Preconditioner(None)
    return M


class IChol0Preconditioner:
    """stands in for the host class of that name: the native object and the shape"""
    def __init__(self, n):
        from ilupp_amd import _native
        self.pr, self.shape = _native.Preconditioner(None), (n, n)


class ILU0Preconditioner(IChol0Preconditioner):
    """... and for a host class of another kind"""


def _pivoting(n):
    from ilupp_amd import _native
    return _native.PivotedPreconditioner(None, n, True, rows=False)


def test_ichol0_refactor_batch_checks_before_any_native_call(monkeypatch):
    pytest.importorskip("torch")
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    _boom(monkeypatch)
    A4, A3, P4, P3, H4 = _fake_csr(4), _fake_csr(3), _unbuilt("IChol0", 4), _unbuilt("IChol0", 3), IChol0Preconditioner(4)
    with pytest.raises(TypeError, match="DeviceCSR"):
        ild.ichol0_refactor_batch_([P4], [object()])
    with pytest.raises(TypeError, match="DeviceCSR"):
        ild.ichol0_refactor_batch_([P4], [np.zeros(4)])
    for kind in ("ILU0", "ILUT", "ILUC", "ICholT"):
        with pytest.raises(TypeError, match="IChol0 kind only"):
            ild.ichol0_refactor_batch_([P4, _unbuilt(kind, 4)], [A4, A4])
    with pytest.raises(TypeError, match="IChol0 kind only"):
        ild.ichol0_refactor_batch_([ILU0Preconditioner(4)], [A4])
    with pytest.raises(TypeError, match="IChol0 kind only"):
        ild.ichol0_refactor_batch_([ild.FactorOperator(ILU0Preconditioner(4))], [A4])
    with pytest.raises(TypeError, match="IChol0 kind only"):
        ild.ichol0_refactor_batch_([_native.Preconditioner(None)], [A4])      # (a bare native object: nothing says it is an IChol(0) one)
    with pytest.raises(TypeError, match="ILUpp"):
        ild.ichol0_refactor_batch_([_unbuilt("ILUpp", 4)], [A4])
    with pytest.raises(TypeError, match="non-pivoting"):
        ild.ichol0_refactor_batch_([_pivoting(4)], [A4])
    with pytest.raises(TypeError):
        ild.ichol0_refactor_batch_([object()], [A4])
    for members, As in (([P4, P3], [A4]), ([P4], [A4, A3]), ([], [A4])):
        with pytest.raises(ValueError, match="preconditioners but . matrices"):
            ild.ichol0_refactor_batch_(members, As)
    with pytest.raises(ValueError, match="appears twice"):
        ild.ichol0_refactor_batch_([P4, P4], [A4, A4])
    with pytest.raises(ValueError, match="appears twice"):
        ild.ichol0_refactor_batch_([H4, ild.FactorOperator(H4)], [A4, A4])
    with pytest.raises(ValueError, match="member 1: the matrix has dimension 4, the preconditioner 3"):
        ild.ichol0_refactor_batch_([H4, P3], [A4, A4])
    with pytest.raises(ValueError, match="member 0: the matrix has dimension 3, the preconditioner 4"):
        ild.ichol0_refactor_batch_([ild.FactorOperator(H4)], [A3], check=False)
    # the empty batch: no native call
    assert ild.ichol0_refactor_batch_([], []) == []
    routes, status = ild.ichol0_refactor_batch_([], [], check=False)
    assert routes == [] and status.numel() == 0


def test_ichol0_refactor_checks_before_any_native_call(monkeypatch):
    pytest.importorskip("torch")
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    for kind in ("ILU0", "ILUT", "ILUC", "ICholT", "ILUpp"):
        with pytest.raises(NotImplementedError, match=kind):
            ild.ichol0_refactor_(_unbuilt(kind, 4), _fake_csr(4))
    with pytest.raises(NotImplementedError, match="ILU0"):
        ild.ichol0_refactor_(ILU0Preconditioner(4), _fake_csr(4))
    with pytest.raises(NotImplementedError, match="ILU0"):
        ild.ichol0_refactor_(ild.FactorOperator(ILU0Preconditioner(4)), _fake_csr(4))
    with pytest.raises(NotImplementedError, match="PivotedPreconditioner"):
        ild.ichol0_refactor_(_pivoting(4), _fake_csr(4))
    with pytest.raises(NotImplementedError, match="object"):
        ild.ichol0_refactor_(object(), _fake_csr(4))
    for M in (_unbuilt("IChol0", 4), IChol0Preconditioner(4), ild.FactorOperator(IChol0Preconditioner(4))):
        with pytest.raises(ValueError, match="the matrix has dimension 3, the preconditioner 4"):
            ild.ichol0_refactor_(M, _fake_csr(3))
        with pytest.raises(TypeError, match="DeviceCSR"):
            ild.ichol0_refactor_(M, np.zeros(4))


def test_ichol0_batch_checks_before_any_native_call(monkeypatch):
    pytest.importorskip("torch")
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    with pytest.raises(TypeError, match="DeviceCSR"):
        ild.ichol0_batch([_fake_csr(4), np.zeros((4, 4))])
    with pytest.raises(TypeError, match="DeviceCSR"):
        ild.ichol0_batch([object()])
    assert ild.ichol0_batch([]) == []
    assert ild.ichol0_batch(iter(())) == []
    # the host classmethod: there, empty, and one format per batch
    assert ilupp.IChol0Preconditioner.batch([]) == []
    import scipy.sparse as sp
    A = sp.identity(3, format="csr")
    with pytest.raises(TypeError, match="one format"):
        ilupp.IChol0Preconditioner.batch([A, A.tocsc()])
