"""CPU tests of the batched BiCGstab solve of the two pivoting classes: the C ABI exports ilupp_hip_pivot_bicgstab_batch_device and refuses
bad arguments before any HIP call; ilupp_amd.device.bicgstab_batch and PivotedOperator check their input before any native call.  (The
checks that need a CUDA tensor to get as far as they go -- a slice outside b, a matrix and a preconditioner of different dimensions, x0 of
another shape, the empty batch -- are in tests/test_gpu_pivot_bicgstab_batch.py.)"""
import ctypes

import numpy as np
import pytest

SYMBOL = "ilupp_hip_pivot_bicgstab_batch_device"
INVALID = -1        # ILUPP_ERR_INVALID
VP = ctypes.c_void_p


def test_library_exports_the_entry():
    from ilupp_amd import _native
    lib = _native.lib()
    assert hasattr(lib, SYMBOL)
    assert SYMBOL in _native.ABI_SYMBOLS
    assert callable(_native.pivot_bicgstab_batch_device)


def _args(**kw):
    """a call of one member that nothing is wrong with but what `kw` replaces.  The member stands in for a handle: zeroed host memory whose
    first word is the dimension (n = 4, the first member of the library's struct) -- a refused call reads nothing else of it; the other
    pointers stand in for device pointers and are never dereferenced by a refused call."""
    x = np.ones(4)
    fake = VP(x.ctypes.data)
    member = (ctypes.c_int32 * 128)()
    member[0] = 4
    a = dict(count=1, members=(VP * 1)(ctypes.addressof(member)), data=(VP * 1)(fake), indices=(VP * 1)(fake), indptr=(VP * 1)(fake),
             nnz=(ctypes.c_int64 * 1)(4), b=fake, x0=None, x=fake, offsets=(ctypes.c_int64 * 1)(0), work=fake, work_doubles=28, maxiter=5,
             rtol=0.0, check_every=0, iterations=fake, flags=fake, rr=fake, init=fake, sync=1, route=(ctypes.c_int32 * 1)())
    a.update(kw)
    a["_keep"] = (x, member)
    return a


def _call(lib, a):
    order = ("count", "members", "data", "indices", "indptr", "nnz", "b", "x0", "x", "offsets", "work", "work_doubles", "maxiter", "rtol",
             "check_every", "iterations", "flags", "rr", "init", "sync", "route")
    return lib.ilupp_hip_pivot_bicgstab_batch_device(*[a[k] for k in order])


def test_library_refuses_bad_arguments_before_any_device_call():
    from ilupp_amd import _native
    lib = _native.lib()
    err = lambda: lib.ilupp_hip_last_error().decode()
    # null lists and pointers, a negative count
    for name in ("members", "data", "indices", "indptr", "nnz", "b", "x", "offsets", "work", "iterations", "flags", "rr", "init"):
        a = _args(**{name: None})
        assert _call(lib, a) == INVALID, name
        assert err() == "null argument", name
    for name in ("data", "indices", "indptr"):
        assert _call(lib, _args(**{name: (VP * 1)()})) == INVALID, name            # a member's matrix array is NULL
        assert err() == "null argument", name
    assert _call(lib, _args(count=-1)) == INVALID
    assert err() == "null argument"
    # a null member, a member named twice
    assert _call(lib, _args(members=(VP * 1)())) == INVALID
    assert err() == "null preconditioner"
    a = _args()
    two = (VP * 2)(a["members"][0], a["members"][0])
    lists = {k: (VP * 2)(a[k][0], a[k][0]) for k in ("data", "indices", "indptr")}
    assert _call(lib, _args(count=2, members=two, nnz=(ctypes.c_int64 * 2)(4, 4), offsets=(ctypes.c_int64 * 2)(0, 4), work_doubles=56,
                            route=(ctypes.c_int32 * 2)(), _keep2=a, **lists)) == INVALID
    assert err() == "a preconditioner appears twice in the batch"
    # negative iteration counts
    for kw in (dict(maxiter=-1), dict(check_every=-1)):
        assert _call(lib, _args(**kw)) == INVALID, kw
        assert err() == "maxiter and check_every must not be negative", kw
    # a workspace below 7 n doubles
    for w in (27, 0, -5):
        assert _call(lib, _args(work_doubles=w)) == INVALID, w
        assert err().startswith("workspace too small"), w
    # nothing to do: the device is not touched
    assert _call(lib, _args(count=0)) == 0
    assert _call(lib, _args(count=0, sync=0, route=None)) == 0
    a = _args(work_doubles=27)
    assert _call(lib, a) == INVALID
    assert np.array_equal(a["_keep"][0], np.ones(4)) and a["route"][0] == 0         # (nothing was written)


class _Boom:
    """stands in for the native library: any call fails the test"""
    def __getattr__(self, name):
        raise AssertionError("native call %s before the argument checks" % name)


def _fake_csr(n):
    import ilupp_amd.device as ild
    A = ild.DeviceCSR.__new__(ild.DeviceCSR)
    A.n, A.nnz, A.shape = n, 3 * n, (n, n)
    return A


def _unbuilt(n, rows=False):
    """a native pivoting object of dimension n without a handle behind it"""
    from ilupp_amd import _native
    return _native.PivotedPreconditioner(None, n, True, rows=rows)


def _boom(monkeypatch):
    from ilupp_amd import _native
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    monkeypatch.setattr(_native, "pivot_bicgstab_batch_device", lambda *a, **k: (_ for _ in ()).throw(AssertionError("native call before the argument checks")))
    monkeypatch.setattr(_native, "set_caller_stream", lambda *a, **k: (_ for _ in ()).throw(AssertionError("native call before the argument checks")))


def test_pivoted_operator_checks_before_any_native_call(monkeypatch):
    torch = pytest.importorskip("torch")
    import scipy.sparse as sp
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    M = ild.PivotedOperator(_unbuilt(4))
    assert (M.kind, M.n, M.shape) == ("ILUCP", 4, (4, 4))
    assert ild.PivotedOperator(_unbuilt(3, rows=True)).kind == "ILUTP"
    assert callable(M.matvec) and callable(M.sync)
    with pytest.raises(TypeError, match="ILUCPPreconditioner / ILUTPPreconditioner"):
        ild.PivotedOperator(sp.eye(4, format="csr"))
    with pytest.raises(TypeError, match="ILUCPPreconditioner / ILUTPPreconditioner"):
        ild.PivotedOperator(object())
    with pytest.raises(NotImplementedError, match="one column at a time"):
        M.apply_(torch.zeros((4, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):
        M.apply_(torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="CUDA"):
        M.apply_(torch.zeros(4, dtype=torch.float64))                  # (a CPU tensor)
    with pytest.raises(ValueError, match="float64"):
        M.apply_(torch.zeros((4, 1), dtype=torch.float32))


def test_bicgstab_batch_checks_before_any_native_call(monkeypatch):
    torch = pytest.importorskip("torch")
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    b = torch.zeros(8, dtype=torch.float64)                            # a CPU tensor: as far as a machine without a GPU gets
    A4, A3, P4, P3 = _fake_csr(4), _fake_csr(3), _unbuilt(4), _unbuilt(3, rows=True)
    with pytest.raises(TypeError, match="DeviceCSR"):
        ild.bicgstab_batch([object()], b, [0], [P4])
    with pytest.raises(TypeError, match="ILUCPPreconditioner / ILUTPPreconditioner"):
        ild.bicgstab_batch([A4], b, [0], [object()])
    with pytest.raises(TypeError, match="ILUCPPreconditioner / ILUTPPreconditioner"):
        ild.bicgstab_batch([A4, A3], b, [0, 4], [P4, ild.DevicePreconditioner.__new__(ild.DevicePreconditioner)])
    for As, offs, Ms in (([A4, A3], [0, 4], [P4]), ([A4], [0, 4], [P4, P3]), ([A4, A3], [0], [P4, ild.PivotedOperator(P3)])):
        with pytest.raises(ValueError, match="matrices, . preconditioners and . offsets"):
            ild.bicgstab_batch(As, b, offs, Ms)
    with pytest.raises(ValueError, match="b: expected a contiguous 1-D torch.float64 CUDA tensor"):
        ild.bicgstab_batch([A4, A3], b, [0, 4], [P4, P3])                  # not on the device
    with pytest.raises(ValueError, match="b: expected"):
        ild.bicgstab_batch([A4], b.to(torch.float32), [0], [P4])
    with pytest.raises(ValueError, match="b: expected"):
        ild.bicgstab_batch([A4], b[:, None], [0], [P4])
    with pytest.raises(ValueError, match="b: expected"):
        ild.bicgstab_batch([A4], np.zeros(8), [0], [P4])
