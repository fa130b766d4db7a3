"""GPU tests of the parked plans (ilupp_amd/csrc/plan_cache.h, api.hip: plan_park / plan_adopt): a box-grid ILU(0) object that is destroyed
leaves the tables its analysis made from the grid's dimensions to the next object of the same shape, which runs the proof of the pattern
and the factor kernel and nothing of the table chain.  What is tested: an adopted object has the reference's bits, the built object's
tables and kernels; shapes of equal size and entry count but other dimensions do not meet; a matrix that only begins like the grid drops
the plan it was handed and gets the general path; objects that left the pristine state never hand on anything wrong; parked plans are
cache in the accounting; the switch turns all of it off.  Factors and applies are compared, as arrays, with the oracle's restatement of the
reference (ILU0.hpp:26-106, sparse_implementation.h:4040-4087), table digests with a child process that parks nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import matgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (64, 48, 40)               # 3 x 3 tiles, n = 122880
ODD = (40, 33, 50)                # n = 66000: no multiple of 256
TWINS = ((32, 64, 48), (64, 32, 48))      # n = 98304 and nnz = 7 n - 2 * 6656, both
COMPACT_L = "k_sptrsv_wv<1, false, false, true>"
ENTRIES = ("host", "device", "nnz")


def _unsym(d, seed):
    return d * (1.0 + 0.25 * np.random.default_rng(seed).random(d.shape[0]))


_patterns, _oracle = {}, {}


def _grid(dims, seed=7):
    if dims not in _patterns:
        _patterns[dims] = matgen.poisson3d(*dims)
    d, i, p = _patterns[dims]
    return (_unsym(d, seed), i, p)


def _want(a, key):
    """the oracle's L, U and apply(ones) for matrix a, computed once per key"""
    from oracle import oracle as O
    if key not in _oracle:
        d, i, p = a
        n = p.shape[0] - 1
        L, U = O.orc().ilu0((d, i, p, True))
        x = O.orc().trisolve(U, O.UPPER, O.ID, O.orc().trisolve(L, O.LOWER, O.ID, np.ones(n)))
        _oracle[key] = (L, U, x)
    return _oracle[key]


def _equals_oracle(P, a, key):
    """factors (values and index arrays) and apply(ones), array-equal"""
    L, U, xw = _want(a, key)
    (ld, li, lp, _, _, _), (ud, ui, up, _, _, _) = P.factors_info()
    for got, want in ((lp, L[2]), (li, L[1]), (up, U[2]), (ui, U[1]), (ld, L[0]), (ud, U[0])):
        assert np.array_equal(got, want)
    x = np.ones(xw.shape[0]); P.apply(x)
    assert np.array_equal(x, xw)


def _move_a_column(i, p, r):
    """row r with one off-diagonal column moved to the free place next to it (sorted, same count, diagonal kept)"""
    n = p.shape[0] - 1
    i = i.copy()
    row = i[p[r]:p[r + 1]]
    for j in range(row.shape[0]):
        nxt = row[j + 1] if j + 1 < row.shape[0] else n
        if row[j] != r and row[j] + 1 < nxt:
            row[j] += 1
            return i
    raise AssertionError("row %d has no column to move" % r)


_keep = []                        # device arrays of the matrices handed to the device entries (every call gets arrays of its own)


def _make(entry, a):
    """an ILU(0) object through the host entry, the plain device entry or the nnz= entry; the device arrays are new ones every time"""
    import torch
    from ilupp_amd import _native
    d, i, p = a
    if entry == "host":
        return _native.ILU0Preconditioner(d, i, p, True)
    t = tuple(torch.from_numpy(np.ascontiguousarray(v)).to(torch.device("cuda", 0)) for v in (d, i, p))
    torch.cuda.synchronize()
    _keep.append(t)
    n = p.shape[0] - 1
    if entry == "device":
        return _native.ILU0Preconditioner_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, True)
    return _native.ILU0Preconditioner_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, True, nnz=int(p[-1]))


@pytest.fixture(autouse=True)
def _clean():
    """every test starts and ends with nothing parked and no device arrays of its own"""
    import torch
    from ilupp_amd import _native
    _native.release_cached_memory()
    yield
    torch.cuda.synchronize()
    del _keep[:]
    _native.release_cached_memory()


def _stats():
    from ilupp_amd import _native
    return np.array(_native.plan_cache_stats(), dtype=np.int64)


def _names(P):
    return (P.path(), P.analysis_path(), tuple(P.kernel_names()))


_CHILD = r"""
import hashlib, sys
sys.path[:0] = [%r, %r]
import numpy as np, matgen
from ilupp_amd import _native
buf = np.empty(1 << 24, dtype=np.int32)
def line(P, n):
    t = hashlib.sha256()
    for which in range(13):
        cnt = int(_native.lib().ilupp_hip_debug_static_table(P._h, which, buf.ctypes.data, buf.shape[0]))
        assert 0 < cnt < buf.shape[0]
        t.update(buf[:cnt].tobytes())
    h = hashlib.sha256()
    for f in P.factors_info():
        for a in f[:3]:
            h.update(np.ascontiguousarray(a).tobytes())
    x = np.ones(n); P.apply(x); h.update(x.tobytes())
    return " ".join((t.hexdigest(), h.hexdigest(), P.path(), P.analysis_path(), ";".join(P.kernel_names())))
for dims in ((64, 48, 40), (40, 33, 50)):
    d, i, p = matgen.poisson3d(*dims)
    d = d * (1.0 + 0.25 * np.random.default_rng(7).random(d.shape[0]))
    n = p.shape[0] - 1
    P = _native.ILU0Preconditioner(d, i, p, True)
    print(line(P, n))
    del P
    P = _native.ILU0Preconditioner(d, i.copy(), p.copy(), True)
    print(line(P, n))
    del P
print("stats", *_native.plan_cache_stats())
"""


def _child(off):
    """a fresh process: per shape an object built in memory nobody has used, destroyed, and a second object -- adopted, unless the switch
    is set; a line of digests for each of the four, then the stats"""
    env = dict(os.environ)
    env.pop("ILUPP_NO_PLAN_CACHE", None)
    if off:
        env["ILUPP_NO_PLAN_CACHE"] = "1"
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=600,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 5 and lines[4].startswith("stats")
    return lines


@pytest.fixture(scope="module")
def child_off():
    return _child(True)


@pytest.fixture(scope="module")
def child_on():
    return _child(False)


def _tables(P):
    from ilupp_amd import _native
    buf = np.empty(1 << 24, dtype=np.int32)
    out = []
    for which in range(13):
        cnt = int(_native.lib().ilupp_hip_debug_static_table(P._h, which, buf.ctypes.data, buf.shape[0]))
        assert 0 < cnt < buf.shape[0], which
        out.append(buf[:cnt].copy())
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_adoption_gives_the_references_bits(entry):
    """(1) built with one value set, destroyed, constructed with another value set from arrays at another address: one adoption, the
    same path and kernels, the oracle's factors and apply, the built object's transposed apply"""
    a0, a1 = _grid(DIMS, 7), _grid(DIMS, 11)
    n = a0[2].shape[0] - 1
    s0 = _stats()
    B = _make(entry, a1)                             # (built: nothing is parked; its transposed apply excludes it from parking)
    xt = np.ones(n); B.apply_trans(xt)
    del B
    assert (_stats() - s0)[0] == 0
    P = _make(entry, a0)
    built = _names(P)
    assert built[0] == "ilu0:static-direct" and built[1] == "grid" and built[2][0] == "k_ilu0_wa<0, 4, 4>" and built[2][1] == COMPACT_L
    _equals_oracle(P, a0, (DIMS, 7))
    s1 = _stats()
    del P
    assert (_stats() - s1)[0] == 1
    Q = _make(entry, a1)
    s = _stats() - s1
    assert s[1] == 1 and s[0] == 0 and s[3] == 0     # one adoption, nothing parked any more, nothing dropped
    assert _names(Q) == built
    _equals_oracle(Q, a1, (DIMS, 11))
    yt = np.ones(n); Q.apply_trans(yt)
    assert np.array_equal(yt, xt)


@pytest.mark.parametrize("which", [0, 1], ids=["64x48x40", "40x33x50"])
def test_one_digest(which, child_on, child_off):
    """(2) tables 0 .. 12 of an adopted object: the digest of a freshly built object in a process that parks nothing (and the same
    factors, apply, path and kernels) -- both in processes of their own, where a built object's tables lie in memory nobody has used;
    and in this process, word for word, the tables of the object that left them"""
    assert child_on[4].split() == ["stats", "2", "2", "2", "0"]      # (per shape a miss, then an adoption; both second objects left a plan)
    assert child_on[2 * which + 1] == child_off[2 * which]
    assert child_on[2 * which] == child_off[2 * which]
    a = _grid((DIMS, ODD)[which])
    s0 = _stats()
    P = _make("host", a)
    built = _tables(P)
    del P
    P = _make("host", a)
    assert (_stats() - s0)[1] == 1
    for got, want in zip(_tables(P), built):
        assert np.array_equal(got, want)


def test_equal_n_and_nnz_other_dimensions():
    """(3) 32 x 64 x 48 parked, 64 x 32 x 48 constructed: a miss, the oracle's bits; then both plans lie side by side and each is adopted"""
    a, b = _grid(TWINS[0]), _grid(TWINS[1])
    assert a[2].shape == b[2].shape and a[2][-1] == b[2][-1] == 7 * 98304 - 2 * 6656
    s0 = _stats()
    P = _make("device", a)
    del P
    assert (_stats() - s0)[0] == 1
    s1 = _stats()
    Q = _make("device", b)
    s = _stats() - s1
    assert s[1] == 0 and s[2] == 1 and s[0] == 0     # no adoption: a miss; the other shape's plan stays parked
    assert Q.analysis_path() == "grid"
    _equals_oracle(Q, b, (TWINS[1], 7))
    del Q
    assert (_stats() - s0)[0] == 2
    s2 = _stats()
    for m, key in ((b, (TWINS[1], 7)), (a, (TWINS[0], 7))):
        R = _make("device", m)
        _equals_oracle(R, m, key)
        del R
    s = _stats() - s2
    assert s[1] == 2 and s[2] == 0 and s[0] == 0 and s[3] == 0


N = DIMS[0] * DIMS[1] * DIMS[2]


@pytest.mark.parametrize("r", [100, N - 2000], ids=["first-tile", "last-slice"])
def test_a_pattern_that_only_looks_like_the_grid(r):
    """(4) one moved column, met with a plan parked: the general path with the oracle's bits through the plain entry and through the
    nnz= entry of a remembered shape, the plan dropped and nothing of it live; a true grid afterwards builds and parks again"""
    from ilupp_amd import _native
    d, i, p = _grid(DIMS)
    bad = (d, _move_a_column(i, p, r), p)
    for m in ((d, i, p), bad):                       # (warm: whatever the first constructions of a process keep for good)
        P = _make("device", m); del P
    _native.release_cached_memory()
    lb0 = _native.live_blocks()
    s0 = _stats()
    P = _make("device", (d, i, p)); del P
    assert (_stats() - s0)[0] == 1
    Q = _make("device", bad)
    s = _stats() - s0
    assert s[1] == 1 and s[3] == 1 and s[0] == 0     # adopted, then dropped: nothing parked
    assert Q.analysis_path() == "general"
    _equals_oracle(Q, bad, (DIMS, 7, r))
    del Q
    assert _native.live_blocks() == lb0 and _stats()[0] == s0[0]
    # the nnz= entry: the true grid is remembered (and parks), the matrix that only looks like it recalls the shape and adopts
    P = _make("nnz", (d, i, p))
    assert P.analysis_path() == "grid"
    del P
    s1 = _stats()
    assert (s1 - s0)[0] == 1
    Q = _make("nnz", bad)
    s = _stats() - s1
    assert s[1] == 1 and s[3] == 1 and s[0] == -1
    assert Q.analysis_path() == "general"
    _equals_oracle(Q, bad, (DIMS, 7, r))
    del Q
    assert _native.live_blocks() == lb0
    P = _make("nnz", (d, i, p))
    assert _names(P)[:2] == ("ilu0:static-direct", "grid")
    _equals_oracle(P, (d, i, p), (DIMS, 7))
    s2 = _stats()
    del P
    assert (_stats() - s2)[0] == 1


@pytest.mark.parametrize("what", ["factors_info", "apply_trans", "refactor_device", "unwaited-apply"])
def test_objects_that_left_the_pristine_state(what):
    """(5) whatever the object before did -- and whether that excluded it from parking or was put back --, the next construction of
    the shape has the oracle's bits and runs the compact-L sweep"""
    import torch
    a0, a1 = _grid(DIMS, 7), _grid(DIMS, 11)
    n = a0[2].shape[0] - 1
    P = _make("device", a0)
    if what == "factors_info":
        P.factors_info()
    elif what == "apply_trans":
        x = np.ones(n); P.apply_trans(x)
    elif what == "refactor_device":
        t = tuple(torch.from_numpy(np.ascontiguousarray(v)).to(torch.device("cuda", 0)) for v in a1)
        torch.cuda.synchronize()
        _keep.append(t)
        P.refactor_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    else:
        v = torch.ones(n, dtype=torch.float64, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        _keep.append(v)
        P.apply_device(v.data_ptr(), n, sync=False)
    del P
    Q = _make("device", a1)
    assert Q.kernel_names()[1] == COMPACT_L and Q.analysis_path() == "grid"
    _equals_oracle(Q, a1, (DIMS, 11))


def test_accounting():
    """(6) a parked plan is cache: no live block, cached bytes; released with the cache; not parked under a limit of 0; two live objects
    of one shape leave at most the capacity, in either order of destruction"""
    from ilupp_amd import _native
    a = _grid(DIMS)
    P = _make("device", a); del P                    # (warm)
    _native.release_cached_memory()
    lb0, cb0 = _native.live_blocks(), _native.cached_bytes()
    s0 = _stats()
    assert s0[0] == 0
    P = _make("device", a)
    buf = np.empty(1 << 24, dtype=np.int32)
    table_bytes = sum(4 * int(_native.lib().ilupp_hip_debug_static_table(P._h, w, buf.ctypes.data, buf.shape[0])) for w in range(13))
    assert table_bytes > 0
    del P
    assert _stats()[0] == 1 and _native.live_blocks() == lb0
    cb1 = _native.cached_bytes()
    assert cb1 - cb0 >= table_bytes
    _native.release_cached_memory()
    assert _stats()[0] == 0 and _native.cached_bytes() < cb1 and _native.live_blocks() == lb0
    limit = int(os.environ.get("ILUPP_CACHE_LIMIT_MB") or 48 * 1024) << 20
    try:
        _native.set_cache_limit(0)
        P = _make("device", a); del P
        assert _stats()[0] == 0 and _native.cached_bytes() == 0 and _native.live_blocks() == lb0
    finally:
        _native.set_cache_limit(limit)
    for first in (0, 1):
        objs = [_make("device", a), _make("device", a)]
        assert _stats()[0] == 0
        del objs[first]
        del objs[0]
        assert 1 <= _stats()[0] <= 4 and _native.live_blocks() == lb0
        _native.release_cached_memory()


def test_switched_off(child_on, child_off):
    """(7) ILUPP_NO_PLAN_CACHE=1: nothing parked, adopted, missed or dropped, and the digests a process has with the cache at work"""
    assert child_off[4].split() == ["stats", "0", "0", "0", "0"]
    assert child_off[:4] == child_on[:4]
