"""CPU tests of the batched apply and the batched CG solve of the non-pivoting classes: the C ABI exports ilupp_hip_apply_batch_device and
ilupp_hip_cg_batch_device and refuses bad arguments before any HIP call; ilupp_amd.device.FactorOperator, apply_batch_ and cg_batch check
their input before any native call.  (The refusal of a multilevel handle needs a built multilevel object, and the wrong-size refusal a
built member: tests/test_gpu_cg_batch.py.)"""
import ctypes

import numpy as np
import pytest

INVALID = -1        # ILUPP_ERR_INVALID
VP = ctypes.c_void_p


def test_library_exports_the_entries():
    from ilupp_amd import _native
    lib = _native.lib()
    for symbol in ("ilupp_hip_apply_batch_device", "ilupp_hip_cg_batch_device", "ilupp_hip_cg_batch_max_n"):
        assert hasattr(lib, symbol)
        assert symbol in _native.ABI_SYMBOLS
    assert callable(_native.apply_batch_device) and callable(_native.cg_batch_device) and callable(_native.cg_batch_max_n)


def _member(n=4):
    """stands in for a handle: zeroed host memory whose third word is the dimension (kind, nnz_mode, n: the first members of the library's
    struct) -- a refused call reads nothing else of it"""
    m = (ctypes.c_int32 * 1024)()
    m[2] = n
    return m


def _args(**kw):
    """a call of one member that nothing is wrong with but what `kw` replaces; the other pointers stand in for device pointers and are
    never dereferenced by a refused call"""
    x = np.ones(4)
    fake = VP(x.ctypes.data)
    member = _member()
    a = dict(count=1, members=(VP * 1)(ctypes.addressof(member)), n=(ctypes.c_int64 * 1)(4), data=(VP * 1)(fake), indices=(VP * 1)(fake),
             indptr=(VP * 1)(fake), nnz=(ctypes.c_int64 * 1)(4), b=fake, x0=None, x=fake, offsets=(ctypes.c_int64 * 1)(0), work=fake,
             work_doubles=20, maxiter=5, rtol=0.0, check_every=0, iterations=fake, flags=fake, rr=fake, bnorm=fake, sync=1,
             route=(ctypes.c_int32 * 1)())
    a.update(kw)
    a["_keep"] = (x, member)
    return a


def _cg(lib, a):
    order = ("count", "members", "n", "data", "indices", "indptr", "nnz", "b", "x0", "x", "offsets", "work", "work_doubles", "maxiter", "rtol",
             "check_every", "iterations", "flags", "rr", "bnorm", "sync", "route")
    return lib.ilupp_hip_cg_batch_device(*[a[k] for k in order])


def _apply(lib, a, transpose=0):
    return lib.ilupp_hip_apply_batch_device(a["count"], a["members"], a["x"], a["offsets"], transpose, a["sync"], a["route"])


def test_cg_entry_refuses_bad_arguments_before_any_device_call():
    from ilupp_amd import _native
    lib = _native.lib()
    err = lambda: lib.ilupp_hip_last_error().decode()
    # null lists and pointers, a negative count
    for name in ("members", "n", "data", "indices", "indptr", "nnz", "b", "x", "offsets", "work", "iterations", "flags", "rr", "bnorm"):
        assert _cg(lib, _args(**{name: None})) == INVALID, name
        assert err() == "null argument", name
    for name in ("data", "indices", "indptr"):
        assert _cg(lib, _args(**{name: (VP * 1)()})) == INVALID, name            # a member's matrix array is NULL
        assert err() == "null argument", name
    assert _cg(lib, _args(count=-1)) == INVALID
    assert err() == "null argument"
    # a member named twice (a NULL member -- no preconditioner -- may stand there any number of times: its refusal below is the workspace's)
    a = _args()
    two = (VP * 2)(a["members"][0], a["members"][0])
    lists = {k: (VP * 2)(a[k][0], a[k][0]) for k in ("data", "indices", "indptr")}
    pair = dict(count=2, n=(ctypes.c_int64 * 2)(4, 4), nnz=(ctypes.c_int64 * 2)(4, 4), offsets=(ctypes.c_int64 * 2)(0, 4), route=(ctypes.c_int32 * 2)(),
                _keep2=a, **lists)
    assert _cg(lib, _args(members=two, work_doubles=40, **pair)) == INVALID
    assert err() == "a preconditioner appears twice in the batch"
    assert _cg(lib, _args(members=(VP * 2)(), work_doubles=39, **pair)) == INVALID
    assert err().startswith("workspace too small")
    # negative iteration counts
    for kw in (dict(maxiter=-1), dict(check_every=-1)):
        assert _cg(lib, _args(**kw)) == INVALID, kw
        assert err() == "maxiter and check_every must not be negative", kw
    # a dimension that is not positive; a workspace below 5 n doubles
    assert _cg(lib, _args(members=(VP * 1)(), n=(ctypes.c_int64 * 1)(0))) == INVALID
    assert err() == "matrix has size 0!"
    for w in (19, 0, -5):
        assert _cg(lib, _args(work_doubles=w)) == INVALID, w
        assert err() == "workspace too small: 5 doubles per unknown of the batch", w
    # nothing to do: the device is not touched
    assert _cg(lib, _args(count=0)) == 0
    assert _cg(lib, _args(count=0, sync=0, route=None)) == 0
    # a refused call writes nothing
    a = _args(work_doubles=19)
    assert _cg(lib, a) == INVALID
    assert np.array_equal(a["_keep"][0], np.ones(4)) and a["route"][0] == 0


def test_apply_entry_refuses_bad_arguments_before_any_device_call():
    from ilupp_amd import _native
    lib = _native.lib()
    err = lambda: lib.ilupp_hip_last_error().decode()
    for name in ("members", "x", "offsets"):
        assert _apply(lib, _args(**{name: None})) == INVALID, name
        assert err() == "null argument", name
    assert _apply(lib, _args(count=-1)) == INVALID
    assert err() == "null argument"
    assert _apply(lib, _args(members=(VP * 1)())) == INVALID
    assert err() == "null preconditioner"
    a = _args()
    two = (VP * 2)(a["members"][0], a["members"][0])
    for transpose in (0, 1):
        b = _args(count=2, members=two, offsets=(ctypes.c_int64 * 2)(0, 4), route=(ctypes.c_int32 * 2)(), _keep2=a)
        assert _apply(lib, b, transpose) == INVALID
        assert err() == "a preconditioner appears twice in the batch"
        assert np.array_equal(b["_keep"][0], np.ones(4)) and list(b["route"]) == [0, 0]      # (nothing was written)
    assert _apply(lib, _args(count=0)) == 0
    assert _apply(lib, _args(count=0, sync=0, route=None)) == 0


class _Boom:
    """stands in for the native library: any call fails the test"""
    def __getattr__(self, name):
        raise AssertionError("native call %s before the argument checks" % name)


def _boom(monkeypatch):
    from ilupp_amd import _native
    fail = lambda *a, **k: (_ for _ in ()).throw(AssertionError("native call before the argument checks"))
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    for name in ("apply_batch_device", "cg_batch_device", "set_caller_stream"):
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


def _pivoting(n):
    from ilupp_amd import _native
    return _native.PivotedPreconditioner(None, n, True, rows=False)


def test_factor_operator_checks_before_any_native_call(monkeypatch):
    torch = pytest.importorskip("torch")
    import scipy.sparse as sp
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    M = ild.FactorOperator(ILU0Preconditioner(4))
    assert (M.kind, M.n, M.shape) == ("ILU0", 4, (4, 4))
    assert callable(M.matvec) and callable(M.sync) and callable(M.apply_)
    for other in (sp.eye(4, format="csr"), object(), _pivoting(4), _unbuilt("ILUpp", 4), _unbuilt("ILU0", 4), M):
        with pytest.raises(TypeError):
            ild.FactorOperator(other)
    with pytest.raises(ValueError, match="shape"):
        M.apply_(torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):
        M.apply_(torch.zeros((2, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="CUDA"):
        M.apply_(torch.zeros(4, dtype=torch.float64))                  # (a CPU tensor)
    with pytest.raises(ValueError, match="float64"):
        M.apply_(torch.zeros((4, 2), dtype=torch.float32))


def test_apply_batch_checks_before_any_native_call(monkeypatch):
    torch = pytest.importorskip("torch")
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    x = torch.zeros(8, dtype=torch.float64)                            # a CPU tensor: as far as a machine without a GPU gets
    P4, P3, H4 = _unbuilt("IChol0", 4), _unbuilt("ILUT", 3), ILU0Preconditioner(4)
    with pytest.raises(TypeError, match="ILUpp"):
        ild.apply_batch_([P4, _unbuilt("ILUpp", 4)], x, [0, 4])
    with pytest.raises(TypeError, match="non-pivoting"):
        ild.apply_batch_([_pivoting(4)], x, [0])
    with pytest.raises(TypeError, match="ILU0 / ILUT / ILUC / IChol0 / ICholT"):
        ild.apply_batch_([object()], x, [0])
    with pytest.raises(ValueError, match="2 preconditioners but 1 offsets"):
        ild.apply_batch_([P4, P3], x, [0])
    with pytest.raises(ValueError, match="does not lie inside x"):
        ild.apply_batch_([P4, ild.FactorOperator(H4), P3], x, [0, 4, 6])
    with pytest.raises(ValueError, match="does not lie inside x"):
        ild.apply_batch_([P4], x, [-1])
    for bad in (x.to(torch.float32), x[:, None], np.zeros(8)):
        with pytest.raises(ValueError, match="x: expected"):
            ild.apply_batch_([P4], bad, [0])
    with pytest.raises(ValueError, match="x: expected a contiguous 1-D torch.float64 CUDA tensor"):
        ild.apply_batch_([P4, H4], x, [0, 4])                          # all else is right: not on the device
    with pytest.raises(ValueError, match="CUDA"):
        ild.apply_batch_([], x, [])


def test_cg_batch_checks_before_any_native_call(monkeypatch):
    torch = pytest.importorskip("torch")
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    b = torch.zeros(8, dtype=torch.float64)                            # a CPU tensor
    A4, A3, P4, P3 = _fake_csr(4), _fake_csr(3), _unbuilt("IChol0", 4), _unbuilt("ILU0", 3)
    with pytest.raises(TypeError, match="DeviceCSR"):
        ild.cg_batch([object()], b, [0], [P4])
    with pytest.raises(TypeError, match="ILUpp"):
        ild.cg_batch([A4], b, [0], [_unbuilt("ILUpp", 4)])
    with pytest.raises(TypeError, match="non-pivoting"):
        ild.cg_batch([A4, A3], b, [0, 4], [None, _pivoting(3)])
    with pytest.raises(TypeError, match="ILU0 / ILUT / ILUC / IChol0 / ICholT"):
        ild.cg_batch([A4], b, [0], [object()])
    for As, offs, Ms in (([A4, A3], [0, 4], [P4]), ([A4], [0, 4], [P4, P3]), ([A4, A3], [0], [None, P3])):
        with pytest.raises(ValueError, match="matrices, . preconditioners and . offsets"):
            ild.cg_batch(As, b, offs, Ms)
    with pytest.raises(ValueError, match="does not lie inside b"):
        ild.cg_batch([A4, A3], b, [0, 6], [P4, None])
    with pytest.raises(ValueError, match="does not lie inside b"):
        ild.cg_batch([A4], b, [-1], [None])
    with pytest.raises(ValueError, match="member 1: the matrix has dimension 4, the preconditioner 3"):
        ild.cg_batch([A3, A4], b, [0, 4], [None, P3])
    with pytest.raises(ValueError, match="the matrix has dimension 3, the preconditioner 4"):
        ild.cg_batch([A3], b, [0], [ild.FactorOperator(ILU0Preconditioner(4))])
    for bad in (b.to(torch.float32), b[:, None], np.zeros(8)):
        with pytest.raises(ValueError, match="b: expected"):
            ild.cg_batch([A4], bad, [0], [P4])
    with pytest.raises(ValueError, match="x0: expected shape"):
        ild.cg_batch([A4], b, [0], [P4], x0=torch.zeros(7, dtype=torch.float64))
    with pytest.raises(ValueError, match="x0: expected a contiguous"):
        ild.cg_batch([A4], b, [0], [P4], x0=b.to(torch.float32))
    with pytest.raises(ValueError, match="b: expected a contiguous 1-D torch.float64 CUDA tensor"):
        ild.cg_batch([A4, A3], b, [0, 4], [P4, None])                      # all else is right: not on the device


def test_empty_lists_give_an_empty_result(monkeypatch):
    """the empty batch: no native call; cg_batch's result is b's shape, the stats are empty.  (b must be a CUDA tensor, so here the
    check that names it is as far as a machine without a GPU gets; with one, the GPU file runs the call.)"""
    torch = pytest.importorskip("torch")
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="CUDA"):
            ild.cg_batch([], torch.zeros(3, dtype=torch.float64), [], [], stats={})
        return
    b = torch.ones(3, dtype=torch.float64, device="cuda")
    st = {}
    x = ild.cg_batch([], b, [], [], stats=st)
    assert x.shape == b.shape and float(x.abs().sum()) == 0.0
    assert st["route"] == [] and all(st[k].numel() == 0 for k in ("iterations", "converged", "relres"))
    assert ild.apply_batch_([], b, []) == []
