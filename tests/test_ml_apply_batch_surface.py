"""CPU tests of the batched apply of the multilevel ILU++ class: the C ABI exports ilupp_hip_ml_apply_batch_device, ilupp_hip_ml_apply_batch
and ilupp_hip_ml_apply_batch_max_n and refuses bad arguments before any HIP call; ilupp_amd.ml_apply_batch, ilupp_amd.device.ml_apply_batch_
and ilupp_amd.device.MultilevelOperator check their input before any native call; ilupp_amd.device.bicgstab_batch still refuses a bare
"ILUpp" DevicePreconditioner and takes a MultilevelOperator.  (What needs a built multilevel object -- a wrong vector length at the library, the
refusals the other batched entries keep -- is in tests/test_gpu_ml_apply_batch.py.)"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import LinearOperator

NEW_SYMBOLS = ("ilupp_hip_ml_apply_batch_device", "ilupp_hip_ml_apply_batch", "ilupp_hip_ml_apply_batch_max_n")
INVALID = -1        # ILUPP_ERR_INVALID


def test_library_exports_the_three_entries():
    from ilupp_amd import _native
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _native.ABI_SYMBOLS, name
    assert callable(_native.ml_apply_batch) and callable(_native.ml_apply_batch_device) and callable(_native.ml_apply_batch_max_n)


def test_library_refuses_bad_arguments_before_any_device_call():
    from ilupp_amd import _native
    lib = _native.lib()
    VP = ctypes.c_void_p
    x = np.ones(4)
    fake = VP(x.ctypes.data)             # stands in for a device pointer: never dereferenced by a refused call
    one_null = (VP * 1)()                # a member list whose only member is NULL
    stranger = (ctypes.c_int32 * 64)()   # zeroed host memory: not an object the library has built
    not_ml = (VP * 1)(ctypes.addressof(stranger))
    off = (ctypes.c_int64 * 1)(0)
    X, N = (VP * 1)(x.ctypes.data), (ctypes.c_int64 * 1)(4)
    route = (ctypes.c_int32 * 1)()
    # the device batch: null lists, a negative count, a null member, a handle that is no live multilevel object
    f = lib.ilupp_hip_ml_apply_batch_device
    for args in ((1, None, fake, off), (1, one_null, None, off), (1, one_null, fake, None), (-1, one_null, fake, off)):
        assert f(*args, 0, 1, route) == INVALID, args
        assert lib.ilupp_hip_last_error().decode() == "null argument"
    assert f(1, one_null, fake, off, 0, 1, route) == INVALID
    assert lib.ilupp_hip_last_error().decode() == "null preconditioner"
    assert f(1, not_ml, fake, off, 0, 1, route) == INVALID
    assert lib.ilupp_hip_last_error().decode() == "member 0 of the batch is not a multilevel preconditioner"
    assert f(0, one_null, fake, off, 0, 1, route) == 0                     # nothing to do: the device is not touched
    assert f(0, one_null, fake, off, 1, 0, None) == 0
    # the host batch
    g = lib.ilupp_hip_ml_apply_batch
    for args in ((1, None, X, N), (1, one_null, None, N), (1, one_null, X, None), (-1, one_null, X, N)):
        assert g(*args, 0, route) == INVALID, args
        assert lib.ilupp_hip_last_error().decode() == "null argument"
    assert g(1, one_null, X, N, 0, route) == INVALID
    assert lib.ilupp_hip_last_error().decode() == "null preconditioner"
    assert g(1, not_ml, X, N, 0, route) == INVALID
    assert lib.ilupp_hip_last_error().decode() == "member 0 of the batch is not a multilevel preconditioner"
    assert g(0, one_null, X, N, 0, route) == 0
    assert g(0, one_null, X, N, 1, None) == 0
    assert np.array_equal(x, np.ones(4)) and route[0] == 0


class _Boom:
    """stands in for the native library: any call fails the test"""
    def __getattr__(self, name):
        raise AssertionError("native call %s before the argument checks" % name)


def _boom(monkeypatch):
    from ilupp_amd import _native
    fail = lambda *a, **k: (_ for _ in ()).throw(AssertionError("native call before the argument checks"))
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    for name in ("ml_apply_batch", "ml_apply_batch_device", "bicgstab_batch_device", "bicgstab_batch_ml_device", "set_caller_stream"):
        monkeypatch.setattr(_native, name, fail)


def _native_ml(n):
    """a native multilevel object of dimension n without a factorisation behind it"""
    from ilupp_amd import _native
    pr = _native.MultilevelPreconditioner.__new__(_native.MultilevelPreconditioner)
    pr._h, pr._n = None, n
    return pr


def _unbuilt(n):
    """an ILUppPreconditioner of dimension n without a factorisation behind it"""
    import ilupp_amd as ilupp
    P = ilupp.ILUppPreconditioner.__new__(ilupp.ILUppPreconditioner)
    P.pr = _native_ml(n)
    LinearOperator.__init__(P, dtype=np.float64, shape=(n, n))
    return P


def _unbuilt_other(cls, n):
    P = cls.__new__(cls)
    P.pr = _Boom()
    LinearOperator.__init__(P, dtype=np.float64, shape=(n, n))
    return P


def _device(kind, n):
    """a DevicePreconditioner of dimension n without a factorisation behind it"""
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    M = ild.DevicePreconditioner.__new__(ild.DevicePreconditioner)
    M.kind, M.n, M.shape = kind, n, (n, n)
    M.pr = _native_ml(n) if kind == "ILUpp" else _native.Preconditioner(None)
    return M


def _fake_csr(n):
    import ilupp_amd.device as ild
    A = ild.DeviceCSR.__new__(ild.DeviceCSR)
    A.n, A.nnz, A.shape = n, 3 * n, (n, n)
    return A


def test_ml_apply_batch_checks_its_input_before_any_native_call(monkeypatch):
    import ilupp_amd as ilupp
    _boom(monkeypatch)
    assert ilupp.ml_apply_batch([], []) == []
    assert ilupp.ml_apply_batch(iter(()), iter(()), transpose=True) == []
    P4, Q3 = _unbuilt(4), _unbuilt(3)
    for bad in (_unbuilt_other(ilupp.ILUCPPreconditioner, 4), _unbuilt_other(ilupp.ILUCPreconditioner, 4), _unbuilt_other(ilupp.ILUppPreconditioner, 4),
                sp.eye(4, format="csr"), _native_ml(4), _device("ILUpp", 4), object()):
        with pytest.raises(TypeError, match="ILUppPreconditioner instances of the ctypes binding"):
            ilupp.ml_apply_batch([P4, bad], [np.ones(4), np.ones(4)])
    with pytest.raises(ValueError, match="2 preconditioners but 1 vectors"):
        ilupp.ml_apply_batch([P4, Q3], [np.ones(4)])
    with pytest.raises(ValueError, match="vector of 4 elements for a preconditioner of dimension 3"):
        ilupp.ml_apply_batch([P4, Q3], [np.ones(4), np.ones(4)])


def test_native_layer_checks_before_the_library():
    from ilupp_amd import _native
    assert _native.ml_apply_batch([], [], False) == []
    assert _native.ml_apply_batch_device([], 0, []) == []
    with pytest.raises(ValueError):
        _native.ml_apply_batch([], [np.ones(2)], False)
    with pytest.raises(ValueError):
        _native.ml_apply_batch_device([], 0, [0])
    for bad in (object(), _native.Preconditioner(None), _native.PivotedPreconditioner(None, 2, True)):
        with pytest.raises(TypeError, match="multilevel"):
            _native.ml_apply_batch([bad], [np.ones(2)], False)
        with pytest.raises(TypeError, match="multilevel"):
            _native.ml_apply_batch_device([bad], 0, [0])


def test_device_batch_checks_its_input_before_any_native_call(monkeypatch):
    torch = pytest.importorskip("torch")
    import ilupp_amd.device as ild
    _boom(monkeypatch)

    class OnDevice(torch.Tensor):
        is_cuda = True
    cpu = torch.zeros(8, dtype=torch.float64)                            # a CPU tensor: as far as a machine without a GPU gets
    x = cpu.as_subclass(OnDevice)                                        # ... and one that says it is on the device
    P4, D3 = _unbuilt(4), _device("ILUpp", 3)
    for bad in (cpu, x.to(torch.float32).as_subclass(OnDevice), torch.zeros((8, 1), dtype=torch.float64).as_subclass(OnDevice), np.zeros(8),
                torch.zeros(16, dtype=torch.float64).as_subclass(OnDevice)[::2]):
        with pytest.raises(ValueError, match="x: expected a contiguous 1-D torch.float64 CUDA tensor"):
            ild.ml_apply_batch_([P4, D3], bad, [0, 4])
    with pytest.raises(ValueError, match="2 preconditioners but 1 offsets"):
        ild.ml_apply_batch_([P4, D3], x, [0])
    for bad in (object(), _device("ILU0", 4), _device("ILUC", 4), ild.DevicePreconditioner.__new__(ild.DevicePreconditioner),
                _unbuilt_other(__import__("ilupp_amd").ILUCPPreconditioner, 4), np.eye(4), None):
        with pytest.raises(TypeError, match="ILUppPreconditioner instances of the ctypes binding, DevicePreconditioners of the \"ILUpp\" kind or MultilevelOperators"):
            ild.ml_apply_batch_([P4, bad], x, [0, 4])
    for offs in ([0, 6], [-1, 4], [5, 0]):
        with pytest.raises(ValueError, match="does not lie inside x"):
            ild.ml_apply_batch_([P4, ild.MultilevelOperator(D3)], x, offs)
    assert ild.ml_apply_batch_([], x, []) == []


def test_multilevel_operator_checks_before_any_native_call(monkeypatch):
    torch = pytest.importorskip("torch")
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    M = ild.MultilevelOperator(_unbuilt(4))
    assert (M.n, M.shape) == (4, (4, 4)) and M.kind != "ILUpp"
    D = ild.MultilevelOperator(_device("ILUpp", 3))
    assert D.n == 3 and D.kind == M.kind and D.pr is D.P.pr
    assert callable(M.matvec) and callable(M.sync) and callable(M.apply_)
    for bad in (sp.eye(4, format="csr"), object(), _device("ILU0", 4), _device("ICholT", 4), M, None,
                _unbuilt_other(__import__("ilupp_amd").ILUCPPreconditioner, 4)):
        with pytest.raises(TypeError, match="ILUppPreconditioner instance of the ctypes binding or a DevicePreconditioner of the \"ILUpp\" kind"):
            ild.MultilevelOperator(bad)
    with pytest.raises(NotImplementedError, match="one column at a time"):
        M.apply_(torch.zeros((4, 2), dtype=torch.float64))
    for bad in (torch.zeros(5, dtype=torch.float64), torch.zeros((3, 1), dtype=torch.float64), torch.zeros((4, 1, 1), dtype=torch.float64), np.zeros(4)):
        with pytest.raises(ValueError, match="shape"):
            M.apply_(bad)
    for bad in (torch.zeros(4, dtype=torch.float32), torch.zeros(4, dtype=torch.float64), torch.zeros((4, 1), dtype=torch.float64)):
        with pytest.raises(ValueError, match="contiguous torch.float64 CUDA tensor"):
            M.apply_(bad)
    # the block loops take the wrapper (its kind is not the one they refuse) and refuse the bare object
    ild._block_setup(_fake_csr(4), torch.zeros((4, 1), dtype=torch.float64).as_subclass(type("OnDevice", (torch.Tensor,), {"is_cuda": True})), M, None)
    with pytest.raises(NotImplementedError, match="multilevel"):
        ild._block_setup(_fake_csr(4), torch.zeros((4, 1), dtype=torch.float64), _device("ILUpp", 4), None)


def test_bicgstab_batch_takes_the_operator_and_refuses_the_bare_kind(monkeypatch):
    """a bare "ILUpp" DevicePreconditioner keeps its TypeError; a MultilevelOperator passes the type check (the call then fails on the
    tensor, which is not on a device: as far as a machine without a GPU gets) and its dimension is checked like every member's; a batch
    with a multilevel member reaches _native.bicgstab_batch_ml_device, one without reaches _native.bicgstab_batch_device as before"""
    torch = pytest.importorskip("torch")
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    _boom(monkeypatch)

    class OnDevice(torch.Tensor):
        is_cuda = True
    b = torch.zeros(8, dtype=torch.float64)
    A4, A3 = _fake_csr(4), _fake_csr(3)
    M4, M3, P4 = ild.MultilevelOperator(_unbuilt(4)), ild.MultilevelOperator(_device("ILUpp", 3)), _device("ILU0", 4)
    for bad in (_device("ILUpp", 4), _unbuilt(4), _native_ml(4)):
        with pytest.raises(TypeError, match="ILUCPPreconditioner / ILUTPPreconditioner"):
            ild.bicgstab_batch([A4, A4], b, [0, 4], [P4, bad])
        with pytest.raises(TypeError):
            ild.cg_batch([A4, A4], b, [0, 4], [P4, bad])
    with pytest.raises(TypeError):
        ild.cg_batch([A4], b, [0], [M4])                                          # (CG: the multilevel preconditioner is not symmetric)
    with pytest.raises(ValueError, match="b: expected a contiguous 1-D torch.float64 CUDA tensor"):
        ild.bicgstab_batch([A4, A3], b, [0, 4], [M4, M3])
    with pytest.raises(ValueError, match="b: expected a contiguous 1-D torch.float64 CUDA tensor"):
        ild.bicgstab_batch([A4, A3, A4], torch.zeros(12, dtype=torch.float64), [0, 4, 8], [M4, None, P4])
    bd = b.as_subclass(OnDevice)
    with pytest.raises(ValueError, match="member 1: the matrix has dimension 4, the preconditioner 3"):
        ild.bicgstab_batch([A4, A4], bd, [0, 4], [M4, M3])
    with pytest.raises(ValueError, match="does not lie inside b"):
        ild.bicgstab_batch([A4, A3], bd, [0, 6], [M4, M3])

    class Reached(Exception):
        pass
    calls = []

    def entry(name):
        def f(*a, **k):
            calls.append((name, a))
            raise Reached(name)
        return f
    monkeypatch.setattr(_native, "set_caller_stream", lambda *a, **k: None)
    monkeypatch.setattr(_native, "bicgstab_batch_device", entry("plain"))
    monkeypatch.setattr(_native, "bicgstab_batch_ml_device", entry("ml"))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: type("S", (), {"cuda_stream": 0})())
    for A in (A4, A3):
        A.data = A.indices = A.indptr = torch.zeros(1)
    P3 = _device("ILUT", 3)
    with pytest.raises(Reached, match="ml"):
        ild.bicgstab_batch([A4, A3], bd, [0, 4], [M4, P3])
    assert calls[0][1][0] == [M4.pr, P3.pr] and calls[0][1][1] == [4, 3]
    del calls[:]
    with pytest.raises(Reached, match="plain"):
        ild.bicgstab_batch([A4, A3], bd, [0, 4], [None, P3])
    assert [c[0] for c in calls] == ["plain"] and calls[0][1][0] == [None, P3.pr]
