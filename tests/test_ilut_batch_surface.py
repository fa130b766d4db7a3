"""CPU tests of the batched ILUT construction's surface: the C ABI exports ilupp_hip_ilut_create_batch and
ilupp_hip_ilut_create_batch_device, declares them in the header and refuses bad arguments before any HIP call;
ilupp_amd.ILUTPreconditioner.batch and ilupp_amd.device.ilut_batch check their input before any native call and wrap what the native
layer returns.  (What needs a GPU is in tests/test_gpu_ilut_batch.py.)"""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

INVALID = -1        # ILUPP_ERR_INVALID
VP = ctypes.c_void_p
SYMBOLS = ("ilupp_hip_ilut_create_batch", "ilupp_hip_ilut_create_batch_device")


def test_library_exports_and_header_declares_the_entries():
    from ilupp_amd import _native
    lib = _native.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ilupp_hip.h")).read()
    for symbol in SYMBOLS:
        assert hasattr(lib, symbol)
        assert symbol in _native.ABI_SYMBOLS
        assert symbol + "(" in header
        assert getattr(lib, symbol).argtypes is not None
    assert '"ilut:batch"' in header
    assert callable(_native.ILUTPreconditioner_batch) and callable(_native.ILUTPreconditioner_batch_device)


def test_entries_refuse_bad_arguments_before_any_device_call():
    from ilupp_amd import _native
    lib = _native.lib()
    err = lambda: lib.ilupp_hip_last_error().decode()
    x = np.ones(4)
    fake = VP(x.ctypes.data)
    one = lambda: (VP * 1)(fake)
    n1, nnz1 = (ctypes.c_int32 * 1)(4), (ctypes.c_int64 * 1)(4)
    out, status, route = (VP * 1)(), (ctypes.c_int32 * 1)(), (ctypes.c_int32 * 1)()
    host = dict(count=1, data=one(), indices=one(), indptr=one(), n=n1, is_csr=1, fill=10, tau=1e-4, out=out, status=status, route=route)
    dev = dict(host, nnz=nnz1)
    horder = ("count", "data", "indices", "indptr", "n", "is_csr", "fill", "tau", "out", "status", "route")
    dorder = ("count", "data", "indices", "indptr", "n", "nnz", "is_csr", "fill", "tau", "out", "status", "route")
    for fn, base, order, lists in ((lib.ilupp_hip_ilut_create_batch, host, horder, ("data", "indices", "indptr", "n", "out")),
                                   (lib.ilupp_hip_ilut_create_batch_device, dev, dorder, ("data", "indices", "indptr", "n", "nnz", "out"))):
        for name in lists:
            a = dict(base, **{name: None})
            assert fn(*[a[k] for k in order]) == INVALID, name
            assert err() == "null argument", name
        for name in ("data", "indices", "indptr"):
            a = dict(base, **{name: (VP * 1)()})                                # a member's matrix array is NULL
            assert fn(*[a[k] for k in order]) == INVALID, name
            assert err() == "null argument", name
        a = dict(base, count=-1)
        assert fn(*[a[k] for k in order]) == INVALID
        assert err() == "null argument"
        # nothing to do: the device is not touched; status and route may be NULL
        a = dict(base, count=0)
        assert fn(*[a[k] for k in order]) == 0
        a = dict(base, count=0, status=None, route=None)
        assert fn(*[a[k] for k in order]) == 0
    assert np.array_equal(x, np.ones(4)) and not out[0]


class _Boom:
    """stands in for the native library: any call fails the test"""
    def __getattr__(self, name):
        raise AssertionError("native call %s before the argument checks" % name)


def _boom(monkeypatch):
    from ilupp_amd import _native
    fail = lambda *a, **k: (_ for _ in ()).throw(AssertionError("native call before the argument checks"))
    monkeypatch.setattr(_native, "lib", lambda: _Boom())
    for name in ("ILUTPreconditioner_batch", "ILUTPreconditioner_batch_device", "ILUTPreconditioner_device", "ILU0Preconditioner_batch",
                 "ILU0Preconditioner_batch_device", "set_caller_stream"):
        monkeypatch.setattr(_native, name, fail)


def _fake_csr(n):
    import ilupp_amd.device as ild
    A = ild.DeviceCSR.__new__(ild.DeviceCSR)
    A.n, A.nnz, A.shape = n, 3 * n, (n, n)
    return A


def _tridiag(n, fmt):
    return sp.diags([np.full(n - 1, -1.0), np.full(n, 4.0), np.full(n - 1, -1.0)], [-1, 0, 1], format=fmt)


def test_device_entry_checks_before_any_native_call(monkeypatch):
    pytest.importorskip("torch")
    import ilupp_amd.device as ild
    _boom(monkeypatch)
    for bad in (object(), np.zeros(4), _tridiag(4, "csr")):
        with pytest.raises(TypeError, match="DeviceCSR"):
            ild.ilut_batch([_fake_csr(4), bad])
        with pytest.raises(TypeError, match="DeviceCSR"):
            ild.ilut_batch([bad], fill_in=10, threshold=1e-4)
    assert ild.ilut_batch([]) == []
    assert ild.ilut_batch(iter(()), fill_in=10, threshold=1e-4) == []
    # DevicePreconditioner.batch is what it was: ILU(0) only
    with pytest.raises(NotImplementedError, match="ILUT"):
        ild.DevicePreconditioner.batch("ILUT", [_fake_csr(4)])


def test_host_entry_checks_before_any_native_call(monkeypatch):
    import ilupp_amd as ilupp
    _boom(monkeypatch)
    with pytest.raises(TypeError, match="one format"):
        ilupp.ILUTPreconditioner.batch([_tridiag(4, "csr"), _tridiag(5, "csc")])
    with pytest.raises(TypeError, match="one format"):
        ilupp.ILUTPreconditioner.batch([_tridiag(4, "csc"), _tridiag(5, "csr"), _tridiag(6, "csc")], fill_in=10, threshold=1e-4)
    with pytest.raises(TypeError):
        ilupp.ILUTPreconditioner.batch([np.eye(3)])
    with pytest.raises(ValueError, match="square"):
        ilupp.ILUTPreconditioner.batch([sp.csr_matrix(np.ones((2, 3)))])
    assert ilupp.ILUTPreconditioner.batch([]) == []
    assert ilupp.ILUTPreconditioner.batch(iter(()), fill_in=10) == []


def test_instances_carry_what_the_constructor_sets(monkeypatch):
    """fakes in place of the library: the wrappers hand the matrices and the parameter set on in order and dress the native objects as
    the constructors do"""
    pytest.importorskip("torch")
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    seen = {}

    def host(ms, is_csr, fill_in, threshold):
        seen["host"] = ([tuple(np.asarray(a).shape[0] for a in m) for m in ms], is_csr, fill_in, threshold)
        return ["h%d" % k for k in range(len(ms))]

    def device(ms, is_csr, fill_in, threshold):
        seen["device"] = (list(ms), is_csr, fill_in, threshold)
        return ["d%d" % k for k in range(len(ms))]

    monkeypatch.setattr(_native, "ILUTPreconditioner_batch", host)
    monkeypatch.setattr(_native, "ILUTPreconditioner_batch_device", device)
    monkeypatch.setattr(ild, "_on_current_stream", lambda: seen.setdefault("ordered", True))      # (torch's current stream needs a GPU)
    for fmt, is_csr in (("csr", True), ("csc", False)):
        mats = [_tridiag(n, fmt) for n in (3, 5, 4)]
        Ps = ilupp.ILUTPreconditioner.batch(mats, fill_in=7, threshold=0.25)
        assert seen["host"] == ([(3 * n - 2, 3 * n - 2, n + 1) for n in (3, 5, 4)], is_csr, 7, 0.25)
        assert [type(P) for P in Ps] == [ilupp.ILUTPreconditioner] * 3
        assert [P.pr for P in Ps] == ["h0", "h1", "h2"]
        assert [P.shape for P in Ps] == [(3, 3), (5, 5), (4, 4)]
        assert all(P.dtype == np.float64 for P in Ps)
    ilupp.ILUTPreconditioner.batch([_tridiag(3, "csr")])
    assert seen["host"][2:] == (100, 0.1)                                # (the constructor's defaults)

    class _T:
        def __init__(self, a):
            self.a = a

        def data_ptr(self):
            return self.a

    As = []
    for k, n in enumerate((4, 7)):
        A = _fake_csr(n)
        A.data, A.indices, A.indptr = _T(100 + k), _T(200 + k), _T(300 + k)
        As.append(A)
    Ms = ild.ilut_batch(As, fill_in=10, threshold=1e-4)
    assert seen["device"] == ([(100, 200, 300, 4, 12), (101, 201, 301, 7, 21)], True, 10, 1e-4)
    assert seen["ordered"]                                               # (construction is ordered on torch's current stream)
    assert [type(M) for M in Ms] == [ild.DevicePreconditioner] * 2
    assert [(M.kind, M.n, M.shape, M.pr) for M in Ms] == [("ILUT", 4, (4, 4), "d0"), ("ILUT", 7, (7, 7), "d1")]
    ild.ilut_batch(As)
    assert seen["device"][2:] == (100, 0.1)
