"""CPU tests of the single-object entries of the C ABI: the twelve construction entries, the three multilevel constructions, the ten
apply entries and the sync / destroy entries refuse bad arguments before any HIP call, with the return code, the message and the order
of the checks the host layer documents (null output, then *out = NULL, then the matrix of size 0).  ctypes on the built library; the
pointers that stand in for arrays are never dereferenced by a refused call.  (The batched entries have their own files, test_*_surface.py;
a wrong vector length needs a constructed object: the GPU suites.)"""
import ctypes

import numpy as np
import pytest

INVALID = -1        # ILUPP_ERR_INVALID
VP = ctypes.c_void_p

# name -> the arguments between is_csr and out
HOST_CREATE = {
    "ilupp_hip_ilu0_create": (),
    "ilupp_hip_ilut_create": (10, 1e-2),
    "ilupp_hip_iluc_create": (10, 1e-2),
    "ilupp_hip_ichol0_create": (),
    "ilupp_hip_icholt_create": (10, 1e-2),
    "ilupp_hip_ilucp_create": (10, 1e-2, 0.0, -1, 10.0),
    "ilupp_hip_ilutp_create": (10, 1e-2, 0.0, -1, 10.0),
}
DEVICE_CREATE = {
    "ilupp_hip_ilu0_create_device": (),
    "ilupp_hip_ilut_create_device": (10, 1e-2),
    "ilupp_hip_iluc_create_device": (10, 1e-2),
    "ilupp_hip_ichol0_create_device": (),
    "ilupp_hip_icholt_create_device": (10, 1e-2),
}
CREATE = sorted({**HOST_CREATE, **DEVICE_CREATE}.items())


@pytest.fixture(scope="module")
def lib():
    from ilupp_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def fake():
    """stands in for a host or a device array"""
    x = np.ones(8)
    yield VP(x.ctypes.data)
    assert np.array_equal(x, np.ones(8))


def _last(lib):
    return lib.ilupp_hip_last_error().decode()


def test_the_lists_name_seven_host_and_five_device_constructions():
    assert len(HOST_CREATE) == 7 and len(DEVICE_CREATE) == 5 and len(CREATE) == 12


@pytest.mark.parametrize("name,extra", CREATE)
def test_construction_refuses_a_null_output(lib, fake, name, extra):
    assert getattr(lib, name)(fake, fake, fake, 4, 1, *extra, None) == INVALID
    assert _last(lib) == "null output"


@pytest.mark.parametrize("name,extra", CREATE)
def test_construction_refuses_a_matrix_of_size_zero_and_clears_the_output(lib, fake, name, extra):
    f = getattr(lib, name)
    for args in ((fake, fake, fake, 0), (fake, fake, None, 4)):      # n = 0; indptr = NULL
        out = VP(0xdead0)                                            # a non-null dummy: the refusal must have cleared it
        assert f(*args, 1, *extra, ctypes.byref(out)) == INVALID, args
        assert _last(lib) == "matrix has size 0!"
        assert out.value is None


def test_multilevel_constructions_refuse_null_arguments(lib, fake):
    from ilupp_amd import _native
    params = _native.MLParams()
    lib.ilupp_hip_ml_default_params(ctypes.byref(params))
    out = VP(0xdead0)
    for name in ("ilupp_hip_ml_create", "ilupp_hip_ml_create_device"):
        f = getattr(lib, name)
        assert f(fake, fake, fake, 4, 1, ctypes.byref(params), None) == INVALID, name
        assert _last(lib) == "null argument"
        assert f(fake, fake, fake, 4, 1, None, ctypes.byref(out)) == INVALID, name
        assert _last(lib) == "null argument"
    arrays, n = (VP * 1)(fake), (ctypes.c_int32 * 1)(4)
    outs, status = (VP * 1)(), (ctypes.c_int32 * 1)()
    g = lib.ilupp_hip_ml_create_batch
    assert g(1, arrays, arrays, arrays, n, 1, ctypes.byref(params), None, status) == INVALID
    assert _last(lib) == "null argument"
    assert g(1, arrays, arrays, arrays, n, 1, None, outs, status) == INVALID
    assert _last(lib) == "null argument"


APPLY = [
    ("ilupp_hip_apply", (8,)),
    ("ilupp_hip_apply_trans", (8,)),
    ("ilupp_hip_apply_device", (8, 0, 1)),
    ("ilupp_hip_apply_block", (8, 1, 0)),
    ("ilupp_hip_apply_block_device", (8, 1, 0, 1)),
    ("ilupp_hip_ml_apply", (8, 0)),
    ("ilupp_hip_ml_apply_device", (8, 0, 1)),
    ("ilupp_hip_ml_apply_part_device", (8, 0, 1, 1)),
    ("ilupp_hip_ilucp_apply", (8, 0)),
    ("ilupp_hip_ilucp_apply_device", (8, 0, 1)),
]


@pytest.mark.parametrize("name,rest", APPLY)
def test_apply_refuses_a_null_handle(lib, fake, name, rest):
    assert getattr(lib, name)(None, fake, *rest) == INVALID
    assert _last(lib) == "null preconditioner"


def test_sync_refuses_a_null_handle(lib):
    assert lib.ilupp_hip_sync(None) == INVALID
    assert lib.ilupp_hip_ml_sync(None) == INVALID


def test_destroy_of_a_null_handle_does_nothing(lib):
    for name in ("ilupp_hip_destroy", "ilupp_hip_ml_destroy", "ilupp_hip_ilucp_destroy"):
        assert getattr(lib, name)(None) is None
