"""The CSR sweep family (sptrsv.hip: k_sptrsv_lc, k_sptrsv_desc, k_sptrsv, k_sptrsv_rows; sptrsv_lm.hip: k_sptrsv_lm) against the CPU model of
tests/sweep_ref.py, on the cases of tests/sweep_cases.py: the factors are the oracle's, three rounds of apply and apply_trans (every sweep
leaves its right-hand-side buffer all-sentinel for the next) and one round on a right-hand side with -0.0, +-inf and NaN have the BITS of
the float64 model (NaNs by position), and every slot ran on the route (info[6]) and the kernel (info[7]) the model names.

Which case pins what (every figure that puts a case there is asserted on the CPU in tests/test_sweep_ref.py; "-up" is the transposed matrix):
  k_sptrsv_lc<FWD_LAST_ASC>     slot 0 of rows16, dense8, chain*, cycle16, handoff*, imports*, lanes*, lines4x192, chol0-band; slot 3 of cholt-band
  k_sptrsv_lc<BWD_FIRST_ASC>    slot 1 of dense8-up, chain*-up, cycle16-up, handoff*-up, imports512-up, lines4x192-up; slot 0 of cholt-band
  k_sptrsv_lc<BWD_FIRST_DESC>   slot 3 of dense8, chain*, cycle16, handoff*, imports512, lanes*, lines4x192, chol0-band
  k_sptrsv_desc<FWD_LAST_ASC>   slot 0 of rows17, dense7, nnz15, one, handoff*-desc, imports65-desc, arrow; slot 2 of their "-up"
  k_sptrsv_desc<BWD_FIRST_ASC>  slot 1 of rows16-up, rows17-up, rows1_16-up, tail*-up, imports1-up .. imports65-up (the transposed pattern: rows of 23 ..
                                262 entries, 256 foreign producers)
  k_sptrsv_desc<BWD_FIRST_DESC> slot 3 of rows16, rows17, rows1_16, tail*, dense7, one, imports1 .. imports65 (the same transposed patterns)
  k_sptrsv<all three>           chain32769 and chain32769-up: B = 32 769 is not compact, and the other factor (B = 1) goes with it (joint)
  k_sptrsv_rows<FWD_LAST_ASC>, <BWD_FIRST_ASC>   cholt-indefinite (route 5, a process with ILUPP_REFERENCE_NANS=1)
  k_sptrsv_lm                   the diagonal factors of every case with nnz >= 16, lines4x192-short, ghost20 ...: RECORDED in sweep_cases.py
  the rule 0 < longest row <= 16, nnz >= 16, n >= 8: rows16 / rows17, rows1_16, dense7 / dense8, nnz15 / nnz16, one
  window loads at the array ends: rows16 (first row short, last long), rows1_16 (last short), tail3, tail6, their "-up" (first row long); cycle16 (the
  last lane owns 2 rows)        entry and right-hand-side rings: chain15 .. chain100, cycle16
  hand-off between lanes of a workgroup: handoff1 .. handoff40 (k_sptrsv_lc, ring of 4) / their "-desc" (k_sptrsv_desc, ring of 8): a lane reads
  its neighbour 1 .. 43 rows back.  What these pin is the RESULT on both sides of the ring -- a tag that matches, an older one (wait), a newer
  one (the entry was recycled: the unknown is fetched from memory) --, NOT the depth: with kXD = 2 every case still passes, and must, since
  the depth only decides how often the ring is hit (profiles/r21_sweep_kernels.txt).  The own previous row: every chain*, handoff*, cycle16
  imports: imports1, 63, 64, 65, 512 (4, 5, 9 foreign unknowns per row); a ghost producer with a chain of 20: ghost20 under ILUPP_NO_PACKED
  nb = 511, 512, 513: lanes*;   the tiled placement: lines4x192;   kl up to 0x7fff: chain32768 under ILUPP_NO_PACKED
NOT pinned here: route 4, hence k_sptrsv_rows<BWD_FIRST_DESC>.  No such case can be built from a valid factor at any n: lvl_order and
lvl_build (sptrsv_lvl.hip) decline only a schedule of the wrong direction, a numbering pass that ran into its time limit, or a dependency
that does not come earlier in the order (k_lvl_fill's `wrong`) -- a pattern that is not triangular, which no case may feed.  Route 4 stays
with the model's rule (sweep_ref.long_rows) alone.  Nor k_sptrsv_small: sweep() never reaches it, it serves the levels of multilevel
objects, which have their own tests.
A degenerate object's rows without entries give NaN (k_sptrsv_rows divides by NaN there; the reference reads past the row): the model says
the same, the oracle does not, so that case is compared with the model alone.
No right-hand side and no factor carries the sentinel's bit pattern (such a vector ends in the kernels' bounded timeout)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import golden_util as G
import sweep_cases as C
import sweep_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_dead = []          # the first child process that faulted, aborted or ran into its time limit: nothing is started after it


def _oracle():
    from oracle import oracle as O
    return O.ref() if O.ref_available() else O.orc()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _special_rhs(n):
    b = G.rhs(n)
    b[n // 7] = -0.0; b[n // 5] = np.inf; b[n // 3] = -np.inf; b[n // 2] = np.nan
    return b


def _same_bits_nan_in_place(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def measure(name):
    """what the device does with a case, as arrays: the factors, three rounds of both applies, the special round, route and kernel of the
    four slots"""
    import ilupp_amd as ilupp
    P = C.make(ilupp, name)
    out = {}
    for tag, F in zip("LU", P.factors()):
        out[tag + "_data"], out[tag + "_indices"], out[tag + "_indptr"] = F.data, F.indices, F.indptr
        out[tag + "_is_csr"] = np.array(int(sp.isspmatrix_csr(F)))
    n = C.matrix(name).shape[0]
    b, s = G.rhs(n), _special_rhs(n)
    for rep in range(3):
        for tag, f in (("id", P.apply), ("tr", P.apply_trans)):
            x = b.copy(); f(x)
            out["x_%s_%d" % (tag, rep)] = x
    for tag, f in (("id", P.apply), ("tr", P.apply_trans)):
        x = s.copy(); f(x)
        out["s_" + tag] = x
    out["routes"] = np.array([P.pr.level_order(slot)[1][6:8] for slot in range(4)], dtype=np.int64)
    return out


@functools.lru_cache(maxsize=None)
def _model(name):
    """the oracle's factors of a case and the float64 model's four vectors (computed once, shared by every setting)"""
    cls, L, U = C.factors(_oracle(), name)
    csr = C.info(name)[2] == "csr"
    n = L.shape[0]
    b, s = G.rhs(n), _special_rhs(n)
    return cls, L, U, {(v, tr): R.apply(cls, L, U, csr, tr == "tr", rhs) for v, rhs in (("x", b), ("s", s)) for tr in ("id", "tr")}


def expected_routes(name, setting):
    """[(route, kernel)] of the four slots: sweep_ref's prediction, and sweep_cases' record where the model answers LM_OR_CSR"""
    cls, L, U, _ = _model(name)
    if name in C.RECORDED_STATIC and setting != "no_packed":
        return [(R.ROUTE_STATIC, 0) if s in R.stored(cls, L, U) else (0, 0) for s in range(4)]
    e = R.expected_routes(cls, L, U, degenerate=name == C.DEGENERATE, no_packed=setting == "no_packed", no_tiles=setting == "no_tiles",
                          tile_tz=2 if setting == "tile_tz" else None)
    out = []
    for slot in range(4):
        route, kernel = e.get(slot, (0, 0))
        if route == R.LM_OR_CSR:
            rec = C.RECORDED.get(name, {})
            assert slot in rec, ("no record for a slot the model cannot decide", name, slot)
            route, kernel = (R.ROUTE_LEVEL_MAJOR, 0) if rec[slot] == R.ROUTE_LEVEL_MAJOR else kernel
        assert route != R.LEVEL_OR_ROWS, ("a case of this module has long rows and n >= 1024", name, slot)
        out.append((route, kernel))
    return out


def judge(name, m, setting="default"):
    cls, L, U, want = _model(name)
    fac = lambda F: (F.data, F.indices, F.indptr, sp.isspmatrix_csr(F))
    for tag, F in (("L", L), ("U", U)):
        if F is not None:
            got = (m[tag + "_data"], m[tag + "_indices"], m[tag + "_indptr"], bool(int(m[tag + "_is_csr"])))
            assert G.mat_equal(got, fac(F)), (name, setting, "factor", tag)
    for tr in ("id", "tr"):
        for rep in range(3):
            assert _same_bits_nan_in_place(m["x_%s_%d" % (tr, rep)], want["x", tr]), (name, setting, tr, "round", rep)
        assert _same_bits_nan_in_place(m["s_" + tr], want["s", tr]), (name, setting, tr, "special right-hand side")
    routes = [tuple(int(v) for v in row) for row in m["routes"]]
    assert routes == expected_routes(name, setting), (name, setting, routes, expected_routes(name, setting))


@pytest.mark.parametrize("name", C.NAMES)
def test_case(name):
    judge(name, measure(name))


# ---- the switches -------------------------------------------------------------------------------------------------------------------------
# (each is read once per process: one fresh interpreter per setting runs the whole table and writes what it measured to a file; the children
# run one after the other, each under a time limit; after one that faulted, aborted or was killed at its limit none is started: _dead)
_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import test_gpu_sweep_kernels as T
out = {}
for name in sys.argv[2:]:
    for k, v in T.measure(name).items():
        out[name + "/" + k] = v
np.savez(sys.argv[1], **out)
"""

SETTINGS = [("no_packed", {"ILUPP_NO_PACKED": "1"}, C.NAMES), ("no_tiles", {"ILUPP_NO_TILES": "1"}, C.NAMES),
            ("tile_tz", {"ILUPP_TILE_TZ": "2"}, C.NAMES), ("reference_nans", {"ILUPP_REFERENCE_NANS": "1"}, (C.DEGENERATE,))]


@pytest.mark.parametrize("setting,env,names", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_switches(setting, env, names, tmp_path):
    """ILUPP_NO_PACKED=1 sends every level-major candidate to the descriptor kernels (all routes predicted then); ILUPP_NO_TILES=1 and
    ILUPP_TILE_TZ=2 (patches of 2 lines instead of 64: lines4x192) move blocks between workgroups; ILUPP_REFERENCE_NANS=1 lets the indefinite
    ICholT case through: the same bits every time"""
    if _dead:
        pytest.fail("not started: an earlier child process ended badly (%s)" % _dead[0])
    out = str(tmp_path / "measured.npz")
    e = {k: v for k, v in os.environ.items() if k not in ("ILUPP_NO_PACKED", "ILUPP_NO_TILES", "ILUPP_TILE_TZ", "ILUPP_REFERENCE_NANS")}
    e.update(env)
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests")), out] + list(names), capture_output=True,
                           text=True, timeout=300, env=e, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _dead.append("%s: time limit" % setting)
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stdout + r.stderr:
        _dead.append("%s: exit status %d" % (setting, r.returncode))
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    z = np.load(out)
    for name in names:
        judge(name, {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}, setting)
