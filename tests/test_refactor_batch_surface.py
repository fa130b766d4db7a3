"""CPU tests of the batched ILU(0) re-factorisation's surface: the C ABI exports ilupp_hip_ilu0_refactor_batch_device and
ilupp_hip_ilu0_refactor_batch_max_n, declares them in the header and refuses bad arguments before any HIP call;
ilupp_amd.device.refactor_batch_ and DevicePreconditioner.refactor_ check their input before any native call.  (The refusals that need a
built member -- a wrong nnz, a member of another class -- are in tests/test_gpu_refactor_batch.py; the C entry's refusal of a live
multilevel handle is plain_batch_args', which tests/test_gpu_cg_batch.py exercises through the entries that share it.)"""
import ctypes
import os

import numpy as np
import pytest

INVALID = -1        # ILUPP_ERR_INVALID
VP = ctypes.c_void_p
SYMBOLS = ("ilupp_hip_ilu0_refactor_batch_device", "ilupp_hip_ilu0_refactor_batch_max_n")


def test_library_exports_and_header_declares_the_entries():
    from ilupp_amd import _native
    lib = _native.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ilupp_hip.h")).read()
    for symbol in SYMBOLS:
        assert hasattr(lib, symbol)
        assert symbol in _native.ABI_SYMBOLS
        assert symbol + "(" in header
    assert callable(_native.ilu0_refactor_batch_device) and callable(_native.ilu0_refactor_batch_max_n)


def _member(n=4):
    """stands in for a handle: zeroed host memory whose third word is the dimension (kind, nnz_mode, n: the first members of the library's
    struct).  A refused call reads of it only what says what kind of object it is: kind and nnz_mode (0 = an LU object with the generic
    count), and sA.nb, the factor schedule's block count, whose 0 means "no ILU(0) analysis behind this".  The multilevel check looks
    the ADDRESS up in the set of live multilevel objects and reads nothing.  64 KB, far more than the struct, so that a field that moves
    still reads zeroed memory and the refusal, not the read, is what the test sees"""
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
    return lib.ilupp_hip_ilu0_refactor_batch_device(*[a[k] for k in order])


def test_entry_refuses_bad_arguments_before_any_device_call():
    from ilupp_amd import _native
    lib = _native.lib()
    err = lambda: lib.ilupp_hip_last_error().decode()
    for name in ("members", "data", "indices", "indptr", "nnz", "status"):
        assert _call(lib, _args(**{name: None})) == INVALID, name
        assert err() == "null argument", name
    for name in ("data", "indices", "indptr"):
        assert _call(lib, _args(**{name: (VP * 1)()})) == INVALID, name          # a member's matrix array is NULL
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
    # zeroed memory is no ILU(0) object (it has no factor schedule): named by its number
    assert _call(lib, _args()) == INVALID
    assert err() == "member 0 of the batch: not an ILU(0) object"
    # a refused call writes nothing
    a = _args()
    assert _call(lib, a) == INVALID
    assert np.array_equal(a["_keep"][0], np.ones(4)) and a["route"][0] == 0
    # nothing to do: the device is not touched
    assert _call(lib, _args(count=0)) == 0
    assert _call(lib, _args(count=0, sync=0, route=None)) == 0


class _Boom:
    """stands in for the native library: any call fails the test"""
    def __getattr__(self, name):
        raise AssertionError("native call %s before the argument checks" % name)


def _boom(monkeypatch):
    from ilupp_amd import _native
    fail = lambda *a, **k: (_ for _ in ()).throw(AssertionError("native call before the argument checks"))
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    for name in ("ilu0_refactor_batch_device", "set_caller_stream"):
        monkeypatch.setattr(_native, name, fail)
    monkeypatch.setattr(_native.Preconditioner, "refactor_device", fail)


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


class ILU0Preconditioner:
    """stands in for the host class of that name: the native object and the shape"""
    def __init__(self, n):
        from ilupp_amd import _native
        self.pr, self.shape = _native.Preconditioner(None), (n, n)


class IChol0Preconditioner(ILU0Preconditioner):
    """... and for a host class of another kind"""


def _pivoting(n):
    from ilupp_amd import _native
    return _native.PivotedPreconditioner(None, n, True, rows=False)


def test_refactor_batch_checks_before_any_native_call(monkeypatch):
    pytest.importorskip("torch")
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    _boom(monkeypatch)
    A4, A3, P4, P3, H4 = _fake_csr(4), _fake_csr(3), _unbuilt("ILU0", 4), _unbuilt("ILU0", 3), ILU0Preconditioner(4)
    with pytest.raises(TypeError, match="DeviceCSR"):
        ild.refactor_batch_([P4], [object()])
    with pytest.raises(TypeError, match="DeviceCSR"):
        ild.refactor_batch_([P4], [np.zeros(4)])
    for kind in ("ILUT", "ILUC", "IChol0", "ICholT"):
        with pytest.raises(TypeError, match="ILU0 kind only"):
            ild.refactor_batch_([P4, _unbuilt(kind, 4)], [A4, A4])
    with pytest.raises(TypeError, match="ILU0 kind only"):
        ild.refactor_batch_([IChol0Preconditioner(4)], [A4])
    with pytest.raises(TypeError, match="ILU0 kind only"):
        ild.refactor_batch_([ild.FactorOperator(IChol0Preconditioner(4))], [A4])
    with pytest.raises(TypeError, match="ILU0 kind only"):
        ild.refactor_batch_([_native.Preconditioner(None)], [A4])             # (a bare native object: nothing says it is an ILU(0) one)
    with pytest.raises(TypeError, match="ILUpp"):
        ild.refactor_batch_([_unbuilt("ILUpp", 4)], [A4])
    with pytest.raises(TypeError, match="non-pivoting"):
        ild.refactor_batch_([_pivoting(4)], [A4])
    with pytest.raises(TypeError):
        ild.refactor_batch_([object()], [A4])
    for members, As in (([P4, P3], [A4]), ([P4], [A4, A3]), ([], [A4])):
        with pytest.raises(ValueError, match="preconditioners but . matrices"):
            ild.refactor_batch_(members, As)
    with pytest.raises(ValueError, match="appears twice"):
        ild.refactor_batch_([P4, P4], [A4, A4])
    with pytest.raises(ValueError, match="appears twice"):
        ild.refactor_batch_([H4, ild.FactorOperator(H4)], [A4, A4])
    with pytest.raises(ValueError, match="member 1: the matrix has dimension 4, the preconditioner 3"):
        ild.refactor_batch_([H4, P3], [A4, A4])
    with pytest.raises(ValueError, match="member 0: the matrix has dimension 3, the preconditioner 4"):
        ild.refactor_batch_([ild.FactorOperator(H4)], [A3], check=False)
    # the empty batch: no native call
    assert ild.refactor_batch_([], []) == []
    routes, status = ild.refactor_batch_([], [], check=False)
    assert routes == [] and status.numel() == 0


def test_refactor_checks_before_any_native_call(monkeypatch):
    pytest.importorskip("torch")
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    for kind in ("ILUT", "ILUC", "IChol0", "ICholT", "ILUpp"):
        with pytest.raises(NotImplementedError, match="ILU0"):
            _unbuilt(kind, 4).refactor_(_fake_csr(4))
    with pytest.raises(ValueError, match="the matrix has dimension 3, the preconditioner 4"):
        _unbuilt("ILU0", 4).refactor_(_fake_csr(3))
    with pytest.raises(TypeError, match="DeviceCSR"):
        _unbuilt("ILU0", 4).refactor_(np.zeros(4))
