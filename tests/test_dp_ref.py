"""The CPU model of the chain with pivoting (tests/dp_ref.py) against the oracle and the reference, and the cases of tests/dp_cases.py
against the records that put them on their boundaries -- all without a GPU:
* on every case the model's levels have the oracle's bits: L, U, D, both permutations and their inverses, the zero-pivot count, and
  through the next level (whose matrix it is) the Schur complement; the real reference too where oracle/_ref is built; and on a fuzz
  sample with the parameter families the model takes;
* every case's pin holds on the model's records;
* the cases discriminate: a model that forgets the dead marks at the hand-over, one that resumes with the LDS flavour's stale
  ctrl[6] / ctrl[7] / ctrl[11], one that applies a clashing chunk of bucket moves at once, one that lets the first copy of a doubled
  index stand -- each gives other bits;
* lv_hash is injective below 2 586, so no index set of the sizes kept to elsewhere can probe twice, let alone wrap (dp_cases: NOT pinned);
* it prints the largest znnz, wnnz and probe length seen."""
import numpy as np
import pytest
import scipy.sparse as sp

import dp_cases as C
import dp_ref as R
import ml_cases
from oracle import oracle as O


def _same_levels(levels, Q, tag):
    assert len(levels) == Q.levels(), tag + (len(levels), Q.levels())
    for k, lev in enumerate(levels):
        q = Q.level(k)
        assert lev.zero_pivots == q["zero_pivots"], tag + (k, "zero pivots")
        for j, (x, y) in enumerate(zip(R.level_arrays(lev), ml_cases.level_arrays(q))):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), tag + (k, j)


def _differs(a, b):
    return any(np.asarray(x).tobytes() != np.asarray(y).tobytes() for x, y in zip(R.level_arrays(a[0]), R.level_arrays(b[0])))


@pytest.mark.parametrize("name", C.NAMES)
def test_model_has_the_oracles_bits(name):
    levels = C.model(name)
    for fmt in ("csr", "csc"):
        ptr, idx, val = C.arrays(name, fmt)
        _same_levels(levels, O.orc().ml((val, idx, ptr, fmt == "csr"), C.params(name, O)), (name, fmt, "oracle"))
        assert len(R.multilevel(ptr, idx, val, fmt == "csr", C.params(name, O))) == len(levels)
    if O.ref_available():
        ptr, idx, val = C.arrays(name, "csr")
        _same_levels(levels, O.ref().ml((val, idx, ptr, True), C.params(name, O)), (name, "reference"))


@pytest.mark.parametrize("name", C.NAMES)
def test_case_is_on_its_boundary(name):
    levels = C.model(name)
    assert bool(C.CASES[name].pin(levels)), (name, C.stops(levels), C.largest(levels), R.launches(levels), R.launches(levels, store=C.STORE))
    n = C.rows(name)[0].shape[0] - 1
    assert n <= 2200 or name == "probe_wrap"


def test_the_largest_figures(capsys):
    f = {"znnz": 0, "wnnz": 0, "probe": 0, "wrapped": []}
    for name in C.NAMES:
        g = R.figures(C.model(name))
        f.update(znnz=max(f["znnz"], g["znnz"]), wnnz=max(f["wnnz"], g["wnnz"]), probe=max(f["probe"], g["probe"]))
        if g["wrapped"]:
            f["wrapped"].append(name)
    with capsys.disabled():
        print("\nlargest znnz %(znnz)d, wnnz %(wnnz)d, probe %(probe)d slots; a probe wraps in %(wrapped)s" % f)
    assert f["znnz"] == f["wnnz"] == R.LV_CAP + 1 and f["wrapped"] == ["probe_wrap"]


def test_every_hand_over_point_from_both_sides():
    """each of the eight places: a case that fits with 2 048 and one that hands over with 2 049; hand-overs at step 0, later, and in the Schur phase"""
    for point in R.POINTS:
        assert any(C.at_point(C.model(nm), point) == R.LV_CAP and not C.stops(C.model(nm)) for nm in C.NAMES), point
        assert any((0, point) == s[::2][:2] for nm in C.NAMES for s in C.stops(C.model(nm)) if s[0] == 0), point
    all_stops = [s for nm in C.NAMES for s in C.stops(C.model(nm)) if s[0] == 0]
    assert any(s[1] == 0 for s in all_stops) and any(s[1] >= 100 for s in all_stops) and any(not s[3] for s in all_stops)
    seq = R.launches(C.model(C.STOP_HANDOVER_STOP), store=C.STORE)
    kinds = [(f, s) for _, f, s, _ in seq]
    i = kinds.index(("LDS", 4))
    assert any(f == "LDS" and s in (1, 2, 3) for f, s in kinds[:i]) and any(f == "memory" and s in (1, 2, 3) for f, s in kinds[i:]), seq


def test_lv_hash_and_the_probe():
    assert R.lv_hash(1) == 0x9E3779B1 >> 20 and R.lv_hash(2586) == R.lv_hash(2) == 966
    assert len({R.lv_hash(c) for c in range(2586)}) == 2586                   # injective: every probe below n = 2 586 is one slot long
    assert R.probe_stats(range(2200)) == (1, False)
    assert R.probe_stats([377, 1974, 3571, 987, 2584, 4558]) == (6, True)     # slots 4 091 .. 4 095, then 4 091 again: on to slot 0
    assert R.probe_stats([2, 2586]) == (2, False)


# ---- the cases discriminate ----------------------------------------------------------------------------------------------------------------
def _variant(name, **kw):
    ptr, idx, val = C.rows(name)
    return R.multilevel(ptr, idx, val, True, C.params(name, O), **kw)


def test_forgotten_dead_marks_give_other_bits():
    """handover/marks: the memory flavour decides liveness by zrec / wrec slot -2; without the marks the LDS flavour leaves, column 1 comes
    back into row 3 of U and row 1 into column 3 of L"""
    base, lost = C.model("handover/marks"), _variant("handover/marks", forget_dead_at=2)
    assert _differs(base, lost) and len(lost[0].U[0]) == len(base[0].U[0]) + 1 and len(lost[0].L[0]) == len(base[0].L[0]) + 1


def test_a_stale_resume_gives_other_bits():
    """handover/marks under small stores: the launch that follows the memory flavour's first store stop begins at step 3; had the stop
    written ctrl[6] = ctrl[7] = 0 like the LDS flavour's, column 5 of the large row would still answer and row 3 of U would lose it"""
    seq = R.launches(C.model("handover/marks"), store=C.STORE)
    at = [k for (_, f, s, k) in seq if f == "memory" and s in (1, 2, 3)][0]
    base, stale = C.model("handover/marks"), _variant("handover/marks", stale_restart_at=at)
    assert at == 3 and _differs(base, stale) and len(stale[0].U[0]) == len(base[0].U[0]) - 1


def test_a_clash_chunk_applied_at_once_gives_another_permutation():
    """window/rows2_epr: rows 5 and 50 move in one chunk, and 50 is the boundary row of 5's move.  (Inside ONE bucket the group sort that
    follows makes any order of the moves come out the same -- moves/clash is such a chunk --, so the case that shows it needs the
    window's end.)"""
    assert C.model("window/rows2_epr")[0].records[0]["moves"] == ["clash"]
    base, once = C.model("window/rows2_epr"), _variant("window/rows2_epr", moves_at_once=True)
    assert not np.array_equal(base[0].perm_rows, once[0].perm_rows)
    assert not _differs(C.model("moves/once_2chunks"), _variant("moves/once_2chunks", moves_at_once=True))      # (the parallel form is right for "once")


@pytest.mark.parametrize("name", ["twice/row_63_64", "twice/col_63_64"])
def test_the_first_copy_gives_other_bits(name):
    assert _differs(C.model(name), _variant(name, first_copy=True))


# ---- breadth: the model on random matrices -------------------------------------------------------------------------------------------------
def test_fuzz_against_the_oracle():
    rng = np.random.default_rng(4242)
    seen = 0
    for it in range(80):
        n = int(rng.integers(3, 120))
        A = (sp.random(n, n, min(1.0, rng.uniform(2, 8) / n), random_state=rng, data_rvs=lambda k: rng.standard_normal(k))
             + sp.eye(n) * float(rng.choice([0.0, 0.5, 3.0]))).asformat("csr" if it % 2 else "csc")
        A.sort_indices()
        a = (A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32), bool(it % 2))
        knobs = ml_cases.pivoting(piv_tol=float(rng.choice([1.0, 0.5, 0.1, 0.0])), PERMUTE_ROWS=int(rng.integers(0, 4)), TOTAL_PIV=int(rng.integers(0, 3)),
                                  BEGIN_TOTAL_PIV=bool(rng.integers(0, 2)), FINAL_ROW_CRIT=int(rng.integers(-1, 10)),
                                  MIN_ELIM_FACTOR=float(rng.choice([0.0, 0.3, 0.5])), SMALL_PIVOT_TERMINATES=bool(rng.integers(0, 2)),
                                  MOVE_LEVEL_FACTOR=float(rng.choice([0.5, 2.0])))
        if rng.integers(0, 3) == 0:
            knobs["fill_in"] = int(rng.integers(1, 8))
        if rng.integers(0, 3) == 0:
            knobs.update(USE_STANDARD_DROPPING=bool(rng.integers(0, 2)), USE_PIVOT_DROPPING=bool(rng.integers(0, 2)), USE_ERR_PROP_DROPPING2=bool(rng.integers(0, 2)),
                         COMBINE_FACTOR=int(rng.integers(0, 4)))
        thr = float(rng.choice([0.0, 1e-3, 1e-2, 0.1, 1.0]))
        P = ml_cases.oracle_params(O, thr, (), knobs)
        if R.refuses(P):
            continue
        _same_levels(R.multilevel(a[2], a[1], a[0], a[3], P), O.orc().ml(a, P), (it, n, thr, tuple(sorted(knobs.items()))))
        seen += 1
    assert seen >= 60


def test_what_the_model_refuses():
    for knobs, pre in ((dict(USE_INVERSE_DROPPING=True), ()), (dict(USE_WEIGHTED_DROPPING=True), ()), (dict(USE_WEIGHTED_DROPPING2=True), ()), ({}, ("PQ_ORDERING",))):
        P = ml_cases.oracle_params(O, 0.1, pre, ml_cases.pivoting(**knobs))
        assert R.refuses(P)
        with pytest.raises(NotImplementedError):
            R.multilevel([0, 1], [0], [1.0], True, P)
