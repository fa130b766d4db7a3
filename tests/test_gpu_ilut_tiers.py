"""The wave-parallel ILUT kernel (ilut_wp.hip: wp_row, wp_select, k_ilut_rows_wp<128, 512> / <256, 1024>, k_ilut_rows_wp_big) on the cases
of tests/ilut_cases.py: which tier, hop and selection path produced a result, not only the result.  Every case, as CSR and as the CSC
arrays of the transpose (the same row view through the other labelling), is compared bit for bit with the oracle -- index arrays,
pointers, values as uint64, apply and apply_trans, total_nnz -- and asserts the ROUTE: the counters of the ILUPP_DEBUG line of
ilut_rows_wp (rows that outgrew LDS by pool / U slots / kept list, rows that left the pool-in-LDS tier, status) and the presence of
the line of the largest capacity class, against ilut_ref.route() over the CPU model's per-row demands.  tests/test_ilut_ref.py shows on the
CPU that the model has the oracle's bits and that every case sits on the boundary it is named for; the table of what is pinned, and what
is not, is in tests/ilut_cases.py.

The switches that are read once per process (ILUPP_ILUT_WAVES, ILUPP_ILUT_NO_TIER2, ILUPP_ILUT_CAP) run in child processes, one after
the other, each under a time limit; after one that faulted, aborted or was killed at its limit none is started."""
import functools
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import scipy.sparse as sp

import golden_util as G
import ilut_cases as C
import ilut_ref as R
from capture_util import Env as _Env, Stderr as _Stderr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_RE_ROWS = re.compile(r"\[ilupp\] ilut_wp: (\d+) of (\d+) rows outgrew LDS \(pool (\d+), U slots (\d+), kept (\d+)\), (\d+) of them the "
                      r"pool-in-LDS tier too, status (-?\d+)")
_RE_BIG = re.compile(r"\[ilupp\] ilut_wp: largest capacity class, (\d+) waves, status (-?\d+)")
_SWITCHES = ("ILUPP_ILUT_WAVES", "ILUPP_ILUT_NO_TIER2", "ILUPP_ILUT_CAP", "ILUPP_ILUT_BIG", "ILUPP_DEBUG")

_dead = []          # the first child process that faulted, aborted or ran into its time limit: nothing is started after it


def seen_route(err):
    """(outgrew, pool, uslots, kept, left_tier2, status, big) of one construction's stderr, in the form of ilut_ref.route; the waves of
    the largest class, or 0"""
    rows, big = _RE_ROWS.findall(err), _RE_BIG.findall(err)
    assert len(rows) <= 1 and len(big) <= 1 and (rows or big), err[-2000:]
    if big:
        assert int(big[0][1]) == 0, err[-2000:]                     # (no case is refused by the largest class)
    first = tuple(int(rows[0][q]) for q in (0, 2, 3, 4, 5, 6)) if rows else (None,) * 6
    return first + (bool(big),), int(big[0][0]) if big else 0


def _inputs(name):
    A = C.matrix(name)
    T = A.T.tocsc(); T.sort_indices()
    return {"csr": A, "csc": T}


def measure(name, fmt, big=False):
    """what the device does with one orientation of a case: factors, both applies, total_nnz, the route seen, the seconds it took"""
    import ilupp_amd as ilupp
    c = C.CASES[name]
    M = _inputs(name)[fmt]
    t0 = time.perf_counter()
    with _Env(ILUPP_DEBUG="1", **({"ILUPP_ILUT_BIG": "1"} if big else {})), _Stderr() as cap:
        P = ilupp.ILUTPreconditioner(M, fill_in=c.p, threshold=c.tau)
    dt = time.perf_counter() - t0
    route, waves = seen_route(cap.err)
    out = {"route": np.array([-1 if v is None else int(v) for v in route], dtype=np.int64), "waves": np.array(waves), "seconds": np.array(dt),
           "total_nnz": np.array(P.total_nnz)}
    for tag, F in zip("LU", P.factors()):
        assert sp.isspmatrix_csr(F) == (fmt == "csr"), (name, fmt)
        out[tag + "_data"], out[tag + "_indices"], out[tag + "_indptr"] = F.data, F.indices, F.indptr
    b = G.rhs(M.shape[0])
    x = b.copy(); P.apply(x); out["x"] = x
    x = b.copy(); P.apply_trans(x); out["xt"] = x
    return out


@functools.lru_cache(maxsize=None)
def _expected(name, fmt):
    """the oracle's factors and applies of one orientation (computed once, left unchanged)"""
    from oracle import oracle as O
    orc = O.orc()
    c = C.CASES[name]
    M = _inputs(name)[fmt]
    Lo, Uo = orc.ilut((M.data.astype(np.float64), M.indices.astype(np.int32), M.indptr.astype(np.int32), fmt == "csr"), c.p, c.tau)
    b = G.rhs(M.shape[0])
    return Lo, Uo, orc.apply_lu(Lo, Uo, b, O.ID), orc.apply_lu(Lo, Uo, b, O.TRANSPOSE)


def _rows(name):
    return C.model(name)[2]


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def judge(name, fmt, m, what="default", **route_kw):
    Lo, Uo, xo, xto = _expected(name, fmt)
    tag = (name, fmt, what)
    for t, Fo in (("L", Lo), ("U", Uo)):
        assert np.array_equal(m[t + "_indptr"], Fo[2]) and np.array_equal(m[t + "_indices"], Fo[1]), tag + (t, "pattern")
        assert np.array_equal(_u64(m[t + "_data"]), _u64(Fo[0])), tag + (t, "values")
    assert np.array_equal(_u64(m["x"]), _u64(xo)), tag + ("apply",)
    assert np.array_equal(_u64(m["xt"]), _u64(xto)), tag + ("apply_trans",)
    n = Lo[2].shape[0] - 1
    assert int(m["total_nnz"]) == int(Lo[2][-1]) + int(Uo[2][-1]) - n, tag          # (preconditioner_implementation.h:1035-1039)
    seen = tuple(None if v < 0 else int(v) for v in m["route"][:6]) + (bool(m["route"][6]),)
    want, _ = R.route(_rows(name), n, C.CASES[name].p, **route_kw)
    assert seen == want, tag + ("route seen", seen, "predicted", want)
    if seen[0] is not None:
        assert seen[0] == seen[1] + seen[2] + seen[3], tag + (seen,)


@pytest.mark.parametrize("name", C.NAMES)
def test_case(name):
    c = C.CASES[name]
    for fmt in ("csr", "csc"):
        m = measure(name, fmt)
        print("%s %s: %.3f s, route %s, waves of the largest class %d" % (name, fmt, float(m["seconds"]), m["route"].tolist(), int(m["waves"])))
        judge(name, fmt, m)
        assert R.route(_rows(name), C.matrix(name).shape[0], c.p)[0] == c.route, name
    # (ILUPP_ILUT_BIG is read per call: the same factors from the largest class, whose line is then the only one)
    m = measure(name, "csr", big=True)
    print("%s csr, ILUPP_ILUT_BIG=1: %.3f s, %d waves" % (name, float(m["seconds"]), int(m["waves"])))
    judge(name, "csr", m, what="largest class forced", force_big=True)


def test_reuse_case_has_more_table_rows_than_waves():
    """with ILUPP_ILUT_WAVES=1 a launch has one wave per CU (ilut_wp.hip:1052-1054): fewer waves than `reuse` has table rows, each of
    which starts on the whole table AND looks columns up -- so some wave takes a second such row after a first, whichever rows it gets.
    The default launch (16 waves per CU) has a wave for every row of the case: there nothing follows anything"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = C.matrix("reuse").shape[0]
    assert cus < C.REUSE_ROWS and n <= 16 * cus, (cus, n)


# ---- the switches -------------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import test_gpu_ilut_tiers as T
out = {}
for name in sys.argv[2:]:
    for fmt in ("csr", "csc"):
        for k, v in T.measure(name, fmt).items():
            out[name + "/" + fmt + "/" + k] = v
np.savez(sys.argv[1], **out)
"""

SETTINGS = [("waves1", {"ILUPP_ILUT_WAVES": "1"}, C.REUSE_CASES, {}),
            ("no_tier2", {"ILUPP_ILUT_NO_TIER2": "1"}, C.TIER_CASES, {"tier2": False}),
            ("cap256", {"ILUPP_ILUT_CAP": "256"}, C.CAP256_CASES, {"cap256": True})]
CHILD_TIMEOUT = 120         # a guard, not an assertion: a child takes 1.2 s on an MI355X (profiles/r23_ilut_tiers.txt), most of it the imports


@pytest.mark.parametrize("setting,env,names,route_kw", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_switches(setting, env, names, route_kw, tmp_path):
    """ILUPP_ILUT_WAVES=1: one wave per CU, fewer than `reuse` has rows that start on the whole table of their wave and look columns up in
    it (test_reuse_case_has_more_table_rows_than_waves): some wave takes one after another, and a cell that wp_uh_clear left behind
    makes the later row take a miss for a hit (ilut_cases.reuse) -- the bits show it; ILUPP_ILUT_NO_TIER2=1: rows that outgrow LDS
    go to the global pieces at once, no row leaves tier 2; ILUPP_ILUT_CAP=256: the p <= 32 cases take the routes of the larger LDS class.
    The same bits every time"""
    if _dead:
        pytest.fail("not started: an earlier child process ended badly (%s)" % _dead[0])
    out = str(tmp_path / "measured.npz")
    e = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    e.update(env)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests")), out] + list(names), capture_output=True,
                           text=True, timeout=CHILD_TIMEOUT, env=e, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _dead.append("%s: time limit" % setting)
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stdout + r.stderr:
        _dead.append("%s: exit status %d" % (setting, r.returncode))
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    print("%s: child process %.1f s" % (setting, time.perf_counter() - t0))
    z = np.load(out)
    for name in names:
        for fmt in ("csr", "csc"):
            pre = name + "/" + fmt + "/"
            m = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
            judge(name, fmt, m, what=setting, **route_kw)
            if setting == "no_tier2":
                assert int(m["route"][4]) == 0, (name, fmt, m["route"])
