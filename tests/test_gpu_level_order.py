"""The level-order family (sptrsv_lvl.hip, sptrsm_lvl.hip, ilu0_lvl.hip) against the CPU model of tests/level_ref.py: the NUMBERING (a
wrong one still gives the right bits, only slower or through a silent fall to another kernel), the ROUTE every sweep took, and the bits at
the structural edges of every kernel instantiation.  What the device did is read through ilupp_hip_debug_level_order (perm, levels, window
and block of the sweep, how the order was numbered, the kernel family of the last sweep over the slot).

Which case pins what (every figure that puts a case there is asserted on the CPU in tests/test_level_ref.py):
  k_sptrsv_lvl<4, 256>    nine48, nine200x7, nine8x300, holes42, nine256         k_sptrsv_lvl<4, 1024>    dense9; counts' U (one level, no entry)
  k_sptrsv_lvl<8, 256>    dense14_small; ILUT / ILUC factors                      k_sptrsv_lvl<8, 1024>    dense14
  k_sptrsv_lvl<16, 256>   box27_41, box27_3x26x27, dense64x16, counts' L          k_sptrsv_lvl<16, 1024>   dense24
  window refills at W, W + 1, 2 W entries, LDS and memory dependencies in one row: counts;  a tail workgroup: every n but dense64x16's
  k_lvl_levels<0, .>      U^T / L^T slots (forward sweeps of apply_trans), the left factor of ILUC, L of the LL^T classes
  k_lvl_levels<1, .>      every U slot and backward sweep                          k_lvl_levels<2, .>       which = 4 (the factor order), W = 4 / 8 / 16:
                                                                                   nine48 / dense14 / box27_41
  lines longer / shorter than the level pass' ring of 16: nine48, nine200x7 / nine8x300 (W = 4), box27_3x26x27 (W = 16)
  k_ilu0_lvl's pivot batches of 16: dense64x16 (every count 0 .. 63, rows of 64 entries), counts (0, 15, 16, 17, 31, 32, 33, 63)
  info[3] = 0 (given)     slot 0 of every "ilu0:level-order" object               info[3] = 1 (natural)    every case with n < 65 536, box27_41
  info[3] = 2 (relaxed)   holes42, nine256; box27_41 under ILUPP_LVL_RELAX_ALL    info[3] = 3 (given up)   ILUPP_LVL_RELAX_BATCHES = 0 and 1
Batches of 32 relaxation passes observed on an MI355X: holes42 (124 levels) 4, nine256 (768 levels) 23 or 24 -- the count moves with the
order in which the hardware runs the rows of an in-place pass, so only its bounds are asserted --, box27_41 under ILUPP_LVL_RELAX_ALL (281
levels) 8 or 9.  With ILUPP_LVL_RELAX_BATCHES=1 neither holes42 nor nine256 has converged after its 32 passes: both are "given up".

Two cases are NOT where one might expect them, by the code's stated rules, and are pinned as they are:
  nine3x700   fewer than 8 entries per row and 1 401 levels of one or two rows: the factor order is numbered and dropped ("deep AND wide",
              csr_and_level_fallbacks), the object is "ilu0:csr" and sweeps on the descriptor kernels; no level order exists.  Its mode-2
              numbering (W = 4, lines of 3 rows) does run, but is thrown away before the entry can read it: it is NOT compared with the
              model on the device.  The short-line natural pass that is compared is nine8x300's (lines of 8, W = 4, all three modes) and
              box27_3x26x27's (lines of 3, W = 16); lines of fewer than 8 rows with W = 4 have no case on a level-order object, since a
              9-point grid that narrow has fewer than 8 entries per row.
  counts      U is the diagonal alone.  Slot 1 (Uc, an "ilu0:level-order" object has no descriptors) sweeps in level order: one level, no
              off-diagonal entry.  Its transposed copy (slot 2) has descriptors, packs into level-major records and sweeps there.
A right-hand side never carries the kernels' marker payloads (sptrsv_small.hip: such a vector ends in a timeout)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import golden_util as G
import level_ref as R
from test_gpu_level_sweeps import _applies, _fac, _oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_expected = {}
_dead = []          # the first child process that faulted, aborted or ran into its time limit: nothing is started after it


def _slot_expectation(key, T, upper, given):
    """R.expected_slot(T), computed once per (case, class, format, sweep) and kept with the pattern it was computed from: a later caller
    that brings another matrix under the same key fails here instead of reading somebody else's numbers"""
    T = T.tocsr()
    mark = (G.sha(T.indptr.astype(np.int64)), G.sha(T.indices.astype(np.int64)), upper, given)
    if key not in _expected:
        _expected[key] = (mark, R.expected_slot(T, upper, given))
    assert _expected[key][0] == mark, ("another pattern under the same key", key)
    return _expected[key][1]


@functools.lru_cache(maxsize=None)
def _factor_expectation(name, fmt):
    A = R.matrix(name)
    return R.expected_factor_order(A if fmt == "csr" else A.T.tocsr())          # (CSC input: the row-major view is A^T)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _special_rhs(n):
    b = G.rhs(n)
    b[n // 7] = -0.0; b[n // 5] = np.inf; b[n // 3] = -np.inf; b[n // 2] = np.nan
    return b


def _same_bits_nan_in_place(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _check_slots(P, key, cls, L, U, csr_input, given0, other_route=()):
    """every slot both applies used: perm, levels, window, block, numbering route and W as the model says, and the sweep ran in level order.
    other_route: {(transpose, slot): route} for sweeps that legitimately run elsewhere (no level order exists for them)"""
    for transpose in (False, True):
        for k, (slot, T) in enumerate(R.plan(cls, L, U, csr_input, transpose)):
            perm, info = P.pr.level_order(slot)
            tag = (key, transpose, slot, info.tolist())
            if (transpose, slot) in dict(other_route):
                assert perm is None and info[6] == dict(other_route)[(transpose, slot)], tag
                continue
            e = _slot_expectation((key, transpose, k), T, k == 1, given0 and slot == 0)
            assert perm is not None and perm.dtype == np.int32 and np.array_equal(perm, e["perm"]), tag
            assert info[0] == e["nlevels"] and info[1] == e["w"] and info[2] == e["block"], (tag, e["nlevels"], e["w"], e["block"])
            assert info[3] == e["how"] and info[5] == e["natural_w"], (tag, e["how"], e["natural_w"])
            assert (1 <= info[4] <= 64) if e["how"] == R.RELAXED else info[4] == 0, tag
            assert info[6] == R.ROUTE_LEVEL_ORDER and info[7] == 0, tag


def _lu_case(P, key, cls, M, is_csr, Lo, Uo, given0, other_route=()):
    """factors, three rounds of both applies, the special right-hand side, then the numbering of every slot they used"""
    O, ref = _oracle()
    n = M.shape[0]
    L, U = P.factors()
    assert G.mat_equal(_fac(L), Lo) and G.mat_equal(_fac(U), Uo)
    b = G.rhs(n)
    _applies(P, ref.apply_lu(Lo, Uo, b, O.ID), ref.apply_lu(Lo, Uo, b, O.TRANSPOSE), b)
    s = _special_rhs(n)
    for f, use in ((P.apply, O.ID), (P.apply_trans, O.TRANSPOSE)):
        x = s.copy(); f(x)
        assert _same_bits_nan_in_place(x, ref.apply_lu(Lo, Uo, s, use)), (key, use)
    _check_slots(P, key, cls, L, U, is_csr, given0, other_route)


ILU0_CASES = [(name, "csr") for name in ("holes42", "nine256", "box27_41", "nine48", "nine200x7", "nine8x300", "box27_3x26x27", "dense64x16", "dense9", "dense14",
                                         "dense24", "dense14_small", "counts")] + [("nine48", "csc"), ("dense14_small", "csc")]


@pytest.mark.parametrize("name,fmt", ILU0_CASES, ids=["%s-%s" % c for c in ILU0_CASES])
def test_ilu0(name, fmt):
    import ilupp_amd as ilupp
    O, ref = _oracle()
    A = R.matrix(name)
    M = A if fmt == "csr" else A.tocsc()
    P = ilupp.ILU0Preconditioner(M)
    assert P.pr.path() == "ilu0:level-order"
    Lo, Uo = ref.ilu0((M.data, M.indices, M.indptr, fmt == "csr"))
    # (counts: the transposed copy of the diagonal U sweeps on its level-major records -- the module docstring)
    other = {(True, 2): R.ROUTE_LEVEL_MAJOR} if name == "counts" else {}
    _lu_case(P, (name, fmt, "ilu0"), "lu", M, fmt == "csr", Lo, Uo, True, tuple(other.items()))
    e = _factor_expectation(name, fmt)
    perm, info = P.pr.level_order(4)
    assert perm is not None and np.array_equal(perm, e["perm"]), (name, info.tolist())
    assert info[0] == e["nlevels"] and info[3] == e["how"] and info[5] == e["natural_w"] and info[6] == 0, (name, info.tolist(), e["how"], e["natural_w"])
    assert (1 <= info[4] <= 64) if e["how"] == R.RELAXED else info[4] == 0, (name, info.tolist())
    assert P.pr.level_order(5)[0] is None and P.pr.level_order(-1)[0] is None


@pytest.mark.parametrize("name", ["below_floor", "nine3x700"])
def test_objects_without_a_level_order(name):
    """n = 1 023 (below the floor of 1 024) and the 3 x 700 grid (deep, not wide): no order exists for any `which`, no sweep runs in level order
    -- both applies ran on the descriptor kernels, info[7] says on which of the two --, and the bits are the reference's all the same"""
    import ilupp_amd as ilupp
    O, ref = _oracle()
    A = R.matrix(name)
    n = A.shape[0]
    P = ilupp.ILU0Preconditioner(A)
    assert P.pr.path() == "ilu0:csr"
    Lo, Uo = ref.ilu0((A.data, A.indices, A.indptr, True))
    L, U = P.factors()
    assert G.mat_equal(_fac(L), Lo) and G.mat_equal(_fac(U), Uo)
    assert all(P.pr.level_order(s)[1][6] == 0 for s in range(4))                      # nothing swept yet
    b = G.rhs(n)
    _applies(P, ref.apply_lu(Lo, Uo, b, O.ID), ref.apply_lu(Lo, Uo, b, O.TRANSPOSE), b)
    # (info[7], the kernel inside the descriptor family: rows and columns of up to 64 entries sweep on k_sptrsv_desc (2), of at most 9 on
    # k_sptrsv_lc (1) -- sptrsv()'s rule, pinned at its edges by test_gpu_sweep_kernels.py)
    kernel = 2 if name == "below_floor" else 1
    for which in range(5):
        perm, info = P.pr.level_order(which)
        assert perm is None and not info[:6].any() and info[7] == (kernel if which < 4 else 0), (which, info.tolist())
        assert info[6] == (R.ROUTE_DESCRIPTORS if which < 4 else 0), (which, info.tolist())


OTHER_LU = [(cls, name, fmt) for cls in ("ilut", "iluc") for name in ("nine48", "holes42", "dense14_small") for fmt in ("csr", "csc")]


@pytest.mark.parametrize("cls,name,fmt", OTHER_LU, ids=["-".join(c) for c in OTHER_LU])
def test_ilut_iluc(cls, name, fmt):
    import ilupp_amd as ilupp
    O, ref = _oracle()
    A = R.matrix(name)
    M = A if fmt == "csr" else A.tocsc()
    fill, tau = 8, 1e-3
    P = (ilupp.ILUTPreconditioner if cls == "ilut" else ilupp.ILUCPreconditioner)(M, fill_in=fill, threshold=tau)
    Lo, Uo = (ref.ilut if cls == "ilut" else ref.iluc)((M.data, M.indices, M.indptr, fmt == "csr"), fill, tau)
    _lu_case(P, (name, fmt, cls), "lu" if cls == "ilut" else "iluc", M, fmt == "csr", Lo, Uo, False)
    assert P.pr.level_order(4)[0] is None


@pytest.mark.parametrize("name", ["sym_nine48", "sym_box27_13"])
@pytest.mark.parametrize("cls", ["ichol0", "icholt"])
def test_ichol(cls, name):
    import ilupp_amd as ilupp
    O, ref = _oracle()
    A = R.matrix(name)
    n = A.shape[0]
    M = (A.data, A.indices, A.indptr, True)
    if cls == "ichol0":
        P, Lo = ilupp.IChol0Preconditioner(A), ref.ichol0(M)
    else:
        P, Lo = ilupp.ICholTPreconditioner(A, add_fill_in=5, threshold=1e-3), ref.icholt(M, 5, 1e-3)
    (L,) = P.factors()
    assert G.mat_equal(_fac(L), Lo) and np.isfinite(Lo[0]).all()
    b = G.rhs(n)
    want = ref.apply_llt(Lo, b, O.ID)
    _applies(P, want, want, b)
    s = _special_rhs(n)
    for f in (P.apply, P.apply_trans):
        x = s.copy(); f(x)
        assert _same_bits_nan_in_place(x, ref.apply_llt(Lo, s, O.ID)), (cls, name)
    _check_slots(P, (name, cls), cls, L, None, True, False)


@pytest.mark.parametrize("name,ks", [("counts", (1, 16, 17)), ("dense24", (1, 16, 17)), ("holes42", (17,))])
def test_block_apply(name, ks):
    """k = 16 is one full chunk of sptrsm_lvl, 17 a full chunk and a chunk of one; a single column is the plain apply ("block:columns", as
    test_gpu_block_apply asserts).  (holes42: 1 and 16 are test_gpu_block_apply's on the 64^3 mesh with holes.)  Every column has the bits
    of its single apply, which test_ilu0 compares with the reference's"""
    import ilupp_amd as ilupp
    A = R.matrix(name)
    n = A.shape[0]
    P = ilupp.ILU0Preconditioner(A)
    X = np.random.default_rng(3).standard_normal((n, max(ks)))
    X[:, 0] = G.rhs(n)
    X[n // 3, min(3, X.shape[1] - 1)] = np.nan
    single = np.column_stack([P @ X[:, j] for j in range(X.shape[1])])
    single_t = np.column_stack([P.T @ X[:, j] for j in range(X.shape[1])])
    for k in ks:
        Y = P.matmat(X[:, :k].copy())                      # (scipy sends an (n, 1) block of P @ X to matvec, matmat never)
        assert P.pr.block_path() == ("block:level" if k > 1 else "block:columns"), k
        assert np.array_equal(_bits(Y), _bits(single[:, :k])), k
        Yt = P.T.matmat(X[:, :k].copy())
        # (counts' transposed apply is no pair of level-ordered sweeps -- the module docstring --: column by column)
        assert P.pr.block_path() == ("block:level" if k > 1 and name != "counts" else "block:columns"), k
        assert np.array_equal(_bits(Yt), _bits(single_t[:, :k])), k


# ---- the three numbering routes agree ------------------------------------------------------------------------------------------------
# (the switches are read once per process: one fresh interpreter per setting, one after the other, each under a time limit; after a child
# that faulted, aborted or was killed at its limit no further child is started: _dead)
_ROUTE_MATRICES = ("holes42", "nine256", "box27_41")
_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import golden_util as G, level_ref as R
import ilupp_amd as ilupp
out = {}
for name in %r:
    A = R.matrix(name)
    P = ilupp.ILU0Preconditioner(A)
    assert P.pr.path() == "ilu0:level-order"
    for f in (P.apply, P.apply_trans):
        x = G.rhs(A.shape[0]); f(x)
        out["%%s/x%%d" %% (name, f == P.apply_trans)] = x
    for which in range(5):
        perm, info = P.pr.level_order(which)
        out["%%s/%%d/info" %% (name, which)] = info
        if perm is not None:
            out["%%s/%%d/perm" %% (name, which)] = perm
np.savez(sys.argv[1], **out)
"""

SETTINGS = [("default", {}), ("no_relax", {"ILUPP_LVL_NO_RELAX": "1"}), ("relax_all", {"ILUPP_LVL_RELAX_ALL": "1"}),
            ("batches_0", {"ILUPP_LVL_RELAX_BATCHES": "0"}), ("batches_1", {"ILUPP_LVL_RELAX_BATCHES": "1"})]


def _how_under(setting, how):
    """(info[3], batches as (lo, hi)) the model's `how` becomes under a switch"""
    if how == R.GIVEN:
        return R.GIVEN, (0, 0)
    if setting == "no_relax":
        return R.NATURAL, (0, 0)
    if setting == "relax_all":
        return R.RELAXED, (1, 64)                          # (all three matrices have n >= 65 536)
    if how == R.RELAXED and setting in ("batches_0", "batches_1"):
        b = int(setting[-1])
        return R.GIVEN_UP, (b, b)
    return how, ((1, 64) if how == R.RELAXED else (0, 0))


@functools.lru_cache(maxsize=None)
def _default_vectors(name):
    O, ref = _oracle()
    A = R.matrix(name)
    Lo, Uo = ref.ilu0((A.data, A.indices, A.indptr, True))
    b = G.rhs(A.shape[0])
    return ref.apply_lu(Lo, Uo, b, O.ID), ref.apply_lu(Lo, Uo, b, O.TRANSPOSE)


@pytest.mark.parametrize("setting,env", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_numbering_routes_agree(setting, env, tmp_path):
    """the natural-order pass, the relaxation, and the natural pass behind a relaxation that was given up (after no pass at all, and after 32
    passes had written into the level array): the same order, the same levels, the same bits; and the route the switch asks for ran.
    Batches observed on an MI355X: default holes42 4, nine256 23 or 24; relax_all box27_41 8 or 9; batches_1: holes42 and nine256 both given
    up after their one batch (124 and 768 levels take more than 32 in-place passes)"""
    if _dead:
        pytest.fail("not started: an earlier child process ended badly (%s)" % _dead[0])
    out = str(tmp_path / "orders.npz")
    e = {k: v for k, v in os.environ.items() if not k.startswith("ILUPP_LVL_")}
    e.update(env)
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), _ROUTE_MATRICES), out], capture_output=True, text=True,
                           timeout=300, env=e, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _dead.append("%s: time limit" % setting)
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stdout + r.stderr:
        _dead.append("%s: exit status %d" % (setting, r.returncode))
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    z = np.load(out)
    for name in _ROUTE_MATRICES:
        A = R.matrix(name)
        lo = R.lower_part(A)
        up = R.lower_part(A.T.tocsr()).T.tocsr()
        for j, want in enumerate(_default_vectors(name)):
            assert np.array_equal(z["%s/x%d" % (name, j)], want), (setting, name, j)
        for transpose in (False, True):
            for k, (slot, T) in enumerate(R.plan("lu", lo, up, True, transpose)):      # (ILU(0): the factors have A's pattern, test_ilu0)
                e = _slot_expectation(((name, "csr", "ilu0"), transpose, k), T, k == 1, slot == 0)
                info = z["%s/%d/info" % (name, slot)]
                tag = (setting, name, slot, info.tolist())
                assert np.array_equal(z["%s/%d/perm" % (name, slot)], e["perm"]), tag
                how, (blo, bhi) = _how_under(setting, e["how"])
                assert info[0] == e["nlevels"] and info[1] == e["w"] and info[2] == e["block"] and info[6] == R.ROUTE_LEVEL_ORDER, tag
                assert info[3] == how and blo <= info[4] <= bhi, (tag, how, blo, bhi)
                assert info[5] == (R.window(R.offdiag_per_row(T)) if how in (R.NATURAL, R.GIVEN_UP) else 0), tag
        e = _factor_expectation(name, "csr")
        info = z["%s/4/info" % name]
        how, (blo, bhi) = _how_under(setting, e["how"])
        assert np.array_equal(z["%s/4/perm" % name], e["perm"]) and info[0] == e["nlevels"], (setting, name, info.tolist())
        assert info[3] == how and blo <= info[4] <= bhi, (setting, name, info.tolist(), how)
        assert info[5] == (R.window(R.factor_per_row(A)) if how in (R.NATURAL, R.GIVEN_UP) else 0), (setting, name, info.tolist())
    if setting == "batches_1":
        assert z["nine256/4/info"][3] == R.GIVEN_UP and z["nine256/1/info"][3] == R.GIVEN_UP
    if setting == "relax_all":
        assert z["box27_41/4/info"][3] == R.RELAXED and z["box27_41/1/info"][3] == R.RELAXED
