"""CPU tests of the batched BiCGstab solve with members of every class: the C ABI exports ilupp_hip_bicgstab_batch_device and
ilupp_hip_bicgstab_batch_max_n and refuses bad arguments before any HIP call; ilupp_amd.device.bicgstab_batch checks a mixed batch before
any native call and sends every batch, one of pivoting members only included, to ilupp_hip_bicgstab_batch_device.  (The refusal of a multilevel
handle needs a built multilevel object: tests/test_gpu_bicgstab_batch.py.)"""
import ctypes

import numpy as np
import pytest

INVALID = -1        # ILUPP_ERR_INVALID
WRONG_SIZE = -2     # ILUPP_ERR_WRONG_SIZE
VP = ctypes.c_void_p
SYMBOLS = ("ilupp_hip_bicgstab_batch_device", "ilupp_hip_bicgstab_batch_max_n")


def test_library_exports_the_entries():
    from ilupp_amd import _native
    lib = _native.lib()
    for symbol in SYMBOLS:
        assert hasattr(lib, symbol), symbol
        assert symbol in _native.ABI_SYMBOLS, symbol
    assert callable(_native.bicgstab_batch_device) and callable(_native.bicgstab_batch_max_n)


def _plain(n=4):
    """stands in for a non-pivoting handle: zeroed host memory whose third word is the dimension (kind, nnz_mode, n: the first members of
    the library's struct) -- a refused call reads nothing else of it"""
    m = (ctypes.c_int32 * 1024)()
    m[2] = n
    return m


def _pivoted(n=4):
    """stands in for a pivoting handle: zeroed host memory whose first word is the dimension"""
    m = (ctypes.c_int32 * 128)()
    m[0] = n
    return m


def _args(**kw):
    """a call of one non-pivoting member that nothing is wrong with but what `kw` replaces; the other pointers stand in for device pointers
    and are never dereferenced by a refused call"""
    x = np.ones(4)
    fake = VP(x.ctypes.data)
    member = _plain()
    a = dict(count=1, plain=(VP * 1)(ctypes.addressof(member)), pivoted=None, n=(ctypes.c_int64 * 1)(4), data=(VP * 1)(fake),
             indices=(VP * 1)(fake), indptr=(VP * 1)(fake), nnz=(ctypes.c_int64 * 1)(4), b=fake, x0=None, x=fake,
             offsets=(ctypes.c_int64 * 1)(0), work=fake, work_doubles=28, maxiter=5, rtol=0.0, check_every=0, iterations=fake, flags=fake,
             rr=fake, init=fake, sync=1, route=(ctypes.c_int32 * 1)())
    a.update(kw)
    a["_keep"] = (x, member)
    return a


def _call(lib, a):
    order = ("count", "plain", "pivoted", "n", "data", "indices", "indptr", "nnz", "b", "x0", "x", "offsets", "work", "work_doubles", "maxiter",
             "rtol", "check_every", "iterations", "flags", "rr", "init", "sync", "route")
    return lib.ilupp_hip_bicgstab_batch_device(*[a[k] for k in order])


def _pair(a):
    """what makes a call of two members out of `a`: the second one's matrix, dimension, offset and route beside the first one's"""
    lists = {k: (VP * 2)(a[k][0], a[k][0]) for k in ("data", "indices", "indptr")}
    return dict(count=2, n=(ctypes.c_int64 * 2)(4, 4), nnz=(ctypes.c_int64 * 2)(4, 4), offsets=(ctypes.c_int64 * 2)(0, 4),
                route=(ctypes.c_int32 * 2)(), work_doubles=56, _keep2=a, **lists)


def test_library_refuses_bad_arguments_before_any_device_call():
    from ilupp_amd import _native
    lib = _native.lib()
    err = lambda: lib.ilupp_hip_last_error().decode()
    # null lists and pointers, a negative count (`plain` and `pivoted` may be null as a whole: a member is then without a preconditioner)
    for name in ("n", "data", "indices", "indptr", "nnz", "b", "x", "offsets", "work", "iterations", "flags", "rr", "init"):
        assert _call(lib, _args(**{name: None})) == INVALID, name
        assert err() == "null argument", name
    for name in ("data", "indices", "indptr"):
        assert _call(lib, _args(**{name: (VP * 1)()})) == INVALID, name            # a member's matrix array is NULL
        assert err() == "null argument", name
    assert _call(lib, _args(count=-1)) == INVALID
    assert err() == "null argument"
    # negative iteration counts
    for kw in (dict(maxiter=-1), dict(check_every=-1)):
        assert _call(lib, _args(**kw)) == INVALID, kw
        assert err() == "maxiter and check_every must not be negative", kw
    # a dimension that is not positive, with or without a preconditioner
    for kw in (dict(plain=None), dict(plain=(VP * 1)()), dict()):
        for n in (0, -3):
            assert _call(lib, _args(n=(ctypes.c_int64 * 1)(n), **kw)) == INVALID, (kw, n)
            assert err() == "matrix has size 0!", (kw, n)
    # a dimension that is not the member's, in either family
    assert _call(lib, _args(n=(ctypes.c_int64 * 1)(5), work_doubles=35)) == WRONG_SIZE
    assert err() == "matrix has wrong size for preconditioner!"
    pv = _pivoted(4)
    assert _call(lib, _args(plain=None, pivoted=(VP * 1)(ctypes.addressof(pv)), n=(ctypes.c_int64 * 1)(3))) == WRONG_SIZE
    assert err() == "matrix has wrong size for preconditioner!"
    # both families name a preconditioner for one member
    assert _call(lib, _args(pivoted=(VP * 1)(ctypes.addressof(pv)))) == INVALID
    assert "both" in err()
    # a handle named twice within either family (a member without a preconditioner may stand there any number of times)
    a = _args()
    assert _call(lib, _args(plain=(VP * 2)(a["plain"][0], a["plain"][0]), **_pair(a))) == INVALID
    assert err() == "a preconditioner appears twice in the batch"
    two = (VP * 2)(ctypes.addressof(pv), ctypes.addressof(pv))
    assert _call(lib, _args(plain=None, pivoted=two, **_pair(a))) == INVALID
    assert err() == "a preconditioner appears twice in the batch"
    assert _call(lib, _args(plain=(VP * 2)(a["plain"][0], None), pivoted=two, **_pair(a))) == INVALID       # (member 0 has both)
    none_twice = _pair(a)
    none_twice["work_doubles"] = 55
    assert _call(lib, _args(plain=None, pivoted=(VP * 2)(), **none_twice)) == INVALID
    assert err().startswith("workspace too small")
    # a workspace below 7 n doubles
    for w in (27, 0, -5):
        assert _call(lib, _args(work_doubles=w)) == INVALID, w
        assert err() == "workspace too small: 7 doubles per unknown of the batch", w
    # nothing to do: the device is not touched
    assert _call(lib, _args(count=0)) == 0
    assert _call(lib, _args(count=0, plain=None, pivoted=None, sync=0, route=None)) == 0
    # a refused call writes nothing
    a = _args(work_doubles=27)
    assert _call(lib, a) == INVALID
    assert np.array_equal(a["_keep"][0], np.ones(4)) and a["route"][0] == 0


class _Boom:
    """stands in for the native library: any call fails the test"""
    def __getattr__(self, name):
        raise AssertionError("native call %s before the argument checks" % name)


def _boom(monkeypatch):
    from ilupp_amd import _native
    fail = lambda *a, **k: (_ for _ in ()).throw(AssertionError("native call before the argument checks"))
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    for name in ("pivot_bicgstab_batch_device", "bicgstab_batch_device", "set_caller_stream"):
        monkeypatch.setattr(_native, name, fail)


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


def _pivoting(n, rows=False):
    from ilupp_amd import _native
    return _native.PivotedPreconditioner(None, n, True, rows=rows)


def test_mixed_batch_checks_before_any_native_call(monkeypatch):
    torch = pytest.importorskip("torch")
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    b = torch.zeros(8, dtype=torch.float64)                            # a CPU tensor: as far as a machine without a GPU gets
    A4, A3, V4, P4, P3, H4 = _fake_csr(4), _fake_csr(3), _pivoting(4), _unbuilt("ILU0", 4), _unbuilt("ILUT", 3), ILU0Preconditioner(4)
    with pytest.raises(TypeError, match="DeviceCSR"):
        ild.bicgstab_batch([A4, object()], b, [0, 4], [P4, None])
    # every bad member is named with the classes the function takes
    for bad in (object(), _unbuilt("ILUpp", 4), ild.DevicePreconditioner.__new__(ild.DevicePreconditioner), np.eye(4), "ILU0"):
        with pytest.raises(TypeError, match="ILUCPPreconditioner / ILUTPPreconditioner"):
            ild.bicgstab_batch([A4, A4], b, [0, 4], [P4, bad])
        with pytest.raises(TypeError, match="ILUCPPreconditioner / ILUTPPreconditioner"):
            ild.bicgstab_batch([A4, A4, A4], b, [0, 4, 8], [V4, None, bad])
    for As, offs, Ms in (([A4, A3], [0, 4], [P4]), ([A4], [0, 4], [V4, None]), ([A4, A3], [0], [None, P3])):
        with pytest.raises(ValueError, match="matrices, . preconditioners and . offsets"):
            ild.bicgstab_batch(As, b, offs, Ms)
    for bad in (b.to(torch.float32), b[:, None], np.zeros(8)):
        with pytest.raises(ValueError, match="b: expected"):
            ild.bicgstab_batch([A4, A3], bad, [0, 4], [P4, None])
    with pytest.raises(ValueError, match="b: expected a contiguous 1-D torch.float64 CUDA tensor"):
        ild.bicgstab_batch([A4, A3, A4], b, [0, 4, 4], [V4, P3, ild.FactorOperator(H4)])      # all else is right: not on the device
    with pytest.raises(ValueError, match="b: expected a contiguous 1-D torch.float64 CUDA tensor"):
        ild.bicgstab_batch([A4, A3], b, [0, 4], [None, None])


def test_dimension_and_slice_checks_of_a_mixed_batch(monkeypatch):
    """the checks behind the tensor checks need a tensor that says it is on the device: a CPU tensor of a subclass whose is_cuda is True
    does, and no native call is reached"""
    torch = pytest.importorskip("torch")
    import ilupp_amd.device as ild
    _boom(monkeypatch)

    class OnDevice(torch.Tensor):
        is_cuda = True
    b = torch.zeros(8, dtype=torch.float64).as_subclass(OnDevice)
    A4, A3, V4, P4, P3 = _fake_csr(4), _fake_csr(3), _pivoting(4), _unbuilt("ILU0", 4), _unbuilt("ILUT", 3)
    with pytest.raises(ValueError, match="member 1: the matrix has dimension 4, the preconditioner 3"):
        ild.bicgstab_batch([A4, A4], b, [0, 4], [None, P3])
    with pytest.raises(ValueError, match="member 2: the matrix has dimension 3, the preconditioner 4"):
        ild.bicgstab_batch([A4, A3, A3], b, [0, 4, 4], [P4, None, V4])
    with pytest.raises(ValueError, match="the matrix has dimension 3, the preconditioner 4"):
        ild.bicgstab_batch([A3], b, [0], [ild.FactorOperator(ILU0Preconditioner(4))])
    with pytest.raises(ValueError, match="does not lie inside b"):
        ild.bicgstab_batch([A4, A3], b, [0, 6], [P4, None])
    with pytest.raises(ValueError, match="does not lie inside b"):
        ild.bicgstab_batch([A4, A4], b, [-1, 4], [None, V4])
    with pytest.raises(ValueError, match="x0: expected shape"):
        ild.bicgstab_batch([A4], b, [0], [P4], x0=torch.zeros(7, dtype=torch.float64).as_subclass(OnDevice))


def test_every_batch_takes_the_one_entry(monkeypatch):
    """every batch, one of pivoting members only included, reaches _native.bicgstab_batch_device with the members' native objects and
    dimensions, and _native.pivot_bicgstab_batch_device is never called: the call is recorded and ended there (the tensors are CPU
    tensors that say they are on the device; nothing native runs)"""
    torch = pytest.importorskip("torch")
    import ilupp_amd.device as ild
    from ilupp_amd import _native

    class Reached(Exception):
        pass

    class OnDevice(torch.Tensor):
        is_cuda = True
    calls = []

    def entry(name):
        def f(*a, **k):
            calls.append((name, a))
            raise Reached(name)
        return f
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    monkeypatch.setattr(_native, "set_caller_stream", lambda *a, **k: None)
    monkeypatch.setattr(_native, "pivot_bicgstab_batch_device",
                        lambda *a, **k: (_ for _ in ()).throw(AssertionError("the pivot entry was called")))
    monkeypatch.setattr(_native, "bicgstab_batch_device", entry("all"))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: type("S", (), {"cuda_stream": 0})())
    b = torch.zeros(8, dtype=torch.float64).as_subclass(OnDevice)
    A4, A3, V4, V3, P3 = _fake_csr(4), _fake_csr(3), _pivoting(4), _pivoting(3, rows=True), _unbuilt("ILU0", 3)
    for A in (A4, A3):
        A.data = A.indices = A.indptr = torch.zeros(1)
    for Ms, natives in (([V4, ild.PivotedOperator(V3)], [V4, V3]), ([V4, P3], [V4, P3.pr]), ([V4, None], [V4, None]),
                        ([None, P3], [None, P3.pr])):
        del calls[:]
        with pytest.raises(Reached, match="all"):
            ild.bicgstab_batch([A4, A3], b, [0, 4], Ms)
        assert [c[0] for c in calls] == ["all"]
        assert calls[0][1][0] == natives and calls[0][1][1] == [4, 3]
