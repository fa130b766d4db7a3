"""The two chain kernels of the factorisation with pivoting (ilupp_amd/csrc/pilucdp.hip: k_pilucdp_lds with its working vectors in LDS,
k_pilucdp with them in memory) and the hand-over between them, on the cases of tests/dp_cases.py: every case sits on one boundary of a
kernel, which tests/test_dp_ref.py proves on the CPU from the model's records.  Here every case is built through
_native.MultilevelILUCDPPreconditioner under ILUPP_DEBUG, as CSR and as CSC, in four modes -- as dispatched, in the memory flavour from
the first step (ILUPP_NO_DPLDS), and with small stores (ILUPP_DP_STORE) from either start -- and in every mode
* all arrays of all levels, apply and apply_trans equal the oracle's as bytes (a NaN is compared by its bits too), and
* the `pilucdp: n .., launch .. (vectors in LDS | vectors in memory; ..): status S at step K` lines equal the sequence the model predicts.
A batch puts a member that hands over between two that do not.  The breadth tests run the memory flavour under every parameter family
the model refuses: the golden vectors of the real reference (tests/golden/mlp.npz) and a fuzz sample against the oracle."""
import functools
import hashlib
import os
import re
import time

import numpy as np
import pytest
import scipy.sparse as sp

import dp_cases as C
import dp_ref as R
import ml_cases
from capture_util import Env, Stderr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_LINE = re.compile(r"\[ilupp\] pilucdp: n (\d+), launch (\d+) \(vectors in (LDS|memory); stores of [^)]*\): status (-?\d+) at step (\d+)")
# mode -> (environment, the ILUPP_DP_STORE the model is told, whether the first launch keeps its vectors in LDS)
MODES = {"dispatched": ({}, None, True),
         "memory": ({"ILUPP_NO_DPLDS": "1"}, None, False),
         "stores": ({"ILUPP_DP_STORE": str(C.STORE)}, C.STORE, True),
         "stores_memory": ({"ILUPP_DP_STORE": str(C.STORE), "ILUPP_NO_DPLDS": "1"}, C.STORE, False)}
FORMATS = ("csr", "csc")


def _engine_params(name):
    import ilupp_amd as ilupp
    c = C.CASES[name]
    return ml_cases.engine_params(ilupp, c.threshold, (), c.knobs)


def _measure(P, n):
    b = ml_cases.rhs(n)
    x = b.copy(); P.apply(x)
    xt = b.copy(); P.apply_trans(xt)
    return dict(levels=[ml_cases.level_arrays(P.level(k)) for k in range(P.levels())], x=x, xt=xt, total_nnz=P.total_nnz)


@functools.lru_cache(maxsize=None)
def _expected(name, fmt):
    """the oracle's object of one orientation with both applies (computed once, left unchanged)"""
    from oracle import oracle as O
    ptr, idx, val = C.arrays(name, fmt)
    Q = O.orc().ml((val, idx, ptr, fmt == "csr"), C.params(name, O))
    b = ml_cases.rhs(ptr.shape[0] - 1)
    return dict(levels=[ml_cases.level_arrays(Q.level(k)) for k in range(Q.levels())], x=Q.apply(b), xt=Q.apply(b, O.TRANSPOSE), total_nnz=Q.total_nnz())


def _same_bytes(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _judge(got, want, tag):
    assert len(got["levels"]) == len(want["levels"]) and got["total_nnz"] == want["total_nnz"], tag
    for k, (a, b) in enumerate(zip(got["levels"], want["levels"])):
        for q, (x, y) in enumerate(zip(a, b)):
            assert _same_bytes(x, y), tag + ("level", k, "array", q)
    assert _same_bytes(got["x"], want["x"]), tag + ("apply",)
    assert _same_bytes(got["xt"], want["xt"]), tag + ("apply_trans",)


def _build(name, fmt, env):
    """the object of one orientation built alone under ILUPP_DEBUG: what it holds, and the launches it logged"""
    from ilupp_amd import _native
    ptr, idx, val = C.arrays(name, fmt)
    with Env(ILUPP_DEBUG="1", **env), Stderr() as cap:
        out = _measure(_native.MultilevelILUCDPPreconditioner(val, idx, ptr, fmt == "csr", _engine_params(name)), ptr.shape[0] - 1)
    seq, nxt = [], 0
    for n, launch, where, status, step in _LINE.findall(cap.err):
        assert int(launch) in (0, nxt), (name, fmt, cap.err[-2000:])           # (a level's launches are numbered from 0)
        nxt = int(launch) + 1
        seq.append((int(n), where, int(status), int(step)))
    return out, seq


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", C.NAMES)
def test_case(name, mode):
    env, store, start_lds = MODES[mode]
    predicted = R.launches(C.model(name), store=store, start_lds=start_lds)
    for fmt in FORMATS:
        t0 = time.perf_counter()
        got, seq = _build(name, fmt, env)
        print("%s %s %s: %.3f s, %d launches" % (name, mode, fmt, time.perf_counter() - t0, len(seq)))
        _judge(got, _expected(name, fmt), (name, mode, fmt))
        assert seq == predicted, (name, mode, fmt, "launches seen", seq, "predicted", predicted)


def test_a_store_stop_on_both_sides_of_a_hand_over():
    """the sequence test_case has just compared for C.STOP_HANDOVER_STOP holds a stop for a store with the vectors in LDS, the hand-over,
    and a stop for a store with the vectors in memory: ctrl[1..5], ctrl[8..10] and dctrl cross the first, znnz / wnnz / prev_pivot
    (ctrl[6], ctrl[7], ctrl[11]) the second"""
    got, seq = _build(C.STOP_HANDOVER_STOP, "csr", MODES["stores"][0])
    kinds = [(w, s) for _, w, s, _ in seq]
    i = kinds.index(("LDS", 4))
    assert any(w == "LDS" and s in (1, 2, 3) for w, s in kinds[:i]) and any(w == "memory" and s in (1, 2, 3) for w, s in kinds[i:]), seq
    _judge(got, _expected(C.STOP_HANDOVER_STOP, "csr"), (C.STOP_HANDOVER_STOP, "stores"))


@pytest.mark.parametrize("fmt", FORMATS)
def test_members_of_a_batch(fmt):
    """ILUppPreconditioner.batch: a member that hands over (its launches with the vectors in memory bypass the combined launch) between
    two that do not, and one that hands over in the middle of its level; every member is the object built alone and the oracle's"""
    import ilupp_amd as ilupp
    names = ["row_load/2048_step0", "row_load/2049_step0", "col_load_own/2048", "u_sub_other/2049", "l_sub/2048", "row_load/2049_mid", "twice/row_63_64"]
    assert len({(C.CASES[nm].threshold, tuple(sorted(C.CASES[nm].knobs.items()))) for nm in names}) == 1
    assert [bool(C.stops(C.model(nm))) for nm in names[:3]] == [False, True, False]
    kind = sp.csr_matrix if fmt == "csr" else sp.csc_matrix
    mats = []
    for nm in names:
        ptr, idx, val = C.arrays(nm, fmt)
        mats.append(kind((val.copy(), idx.copy(), ptr.copy()), shape=(ptr.shape[0] - 1,) * 2))
    with Env(ILUPP_DEBUG="1"), Stderr() as cap:
        B = ilupp.ILUppPreconditioner.batch(mats, params=_engine_params(names[0]))
    assert len(B) == len(names)
    seen = [(int(n), w, int(s), int(k)) for n, _, w, s, k in _LINE.findall(cap.err)]
    for nm, Pb in zip(names, B):
        n = C.rows(nm)[0].shape[0] - 1
        got = _measure(Pb.pr, n)
        _judge(got, _expected(nm, fmt), (nm, fmt, "member of the batch"))
        _judge(got, _build(nm, fmt, {})[0], (nm, fmt, "member against the object built alone"))
        for launch in R.launches(C.model(nm)):
            if launch[1] == "memory" or launch[2] == 4:
                assert launch in seen, (nm, fmt, launch, seen)


# ---- breadth: the memory flavour under the parameter families the model refuses -----------------------------------------------------------
def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", [n for n, _ in ml_cases.matrices()])
def test_reference_vectors_with_the_vectors_in_memory(name, fmt):
    """tests/golden/mlp.npz (the real reference on ml_cases.PIVOT_PARAMS: inverse-based and weighted dropping, bounded fill, every window)
    with k_pilucdp from the first step"""
    import ilupp_amd as ilupp
    from ilupp_amd import _native
    gold = np.load(os.path.join(HERE, "golden", "mlp.npz"))
    key = "%s_%s" % (name, fmt)
    a = (gold[key + "/data"], gold[key + "/indices"], gold[key + "/indptr"], fmt == "csr")
    b = ml_cases.rhs(a[2].shape[0] - 1)
    for tag, thr, pre, knobs in ml_cases.PIVOT_PARAMS:
        k2 = "%s/%s" % (key, tag)
        with Env(ILUPP_DEBUG="1", ILUPP_NO_DPLDS="1"), Stderr() as cap:
            P = _native.MultilevelILUCDPPreconditioner(a[0], a[1], a[2], a[3], ml_cases.engine_params(ilupp, thr, pre, knobs))
        where = set(w for _, _, w, _, _ in _LINE.findall(cap.err))
        assert where == {"memory"}, (k2, where)
        info = gold[k2 + "/info"]
        assert P.levels() == info[0] and P.total_nnz == info[1], k2
        for k in range(P.levels()):
            assert np.array_equal(_digest(ml_cases.level_arrays(P.level(k))), gold[k2 + "/levels_sha"][k]), (k2, k)
        x = b.copy(); P.apply(x)
        assert np.array_equal(x, gold[k2 + "/apply"], equal_nan=True), k2
        x = b.copy(); P.apply_trans(x)
        assert np.array_equal(x, gold[k2 + "/apply_trans"], equal_nan=True), k2


RECURRENCES = {"inverse": dict(USE_INVERSE_DROPPING=True), "weighted": dict(USE_WEIGHTED_DROPPING=True, INIT_WEIGHTS_LU=0.5),
               "weighted2_inverse_sum": dict(USE_WEIGHTED_DROPPING2=True, USE_INVERSE_DROPPING=True, COMBINE_FACTOR=1)}


@pytest.mark.parametrize("rule", list(RECURRENCES))
def test_hand_over_under_the_rules_that_are_recurrences(rule):
    """inverse-based and weighted dropping keep running products and sums over all steps (DpArgs inv / wts): they cross the hand-over and
    the resume in global memory.  The model refuses these rules, so only the bits are compared, with the oracle, and the log must show
    the hand-over; small stores add a resume on either side of it"""
    import ilupp_amd as ilupp
    from ilupp_amd import _native
    from oracle import oracle as O
    for name in ("row_load/2049_mid", "l_sub/2049", "u_sub_other/2049", "schur/l_sub_2049", "handover/marks"):
        c = C.CASES[name]
        kn = dict(c.knobs)
        kn.update(RECURRENCES[rule])
        ptr, idx, val = C.arrays(name, "csr")
        n = ptr.shape[0] - 1
        Q = O.orc().ml((val, idx, ptr, True), ml_cases.oracle_params(O, c.threshold, (), kn))
        b = ml_cases.rhs(n)
        want = dict(levels=[ml_cases.level_arrays(Q.level(k)) for k in range(Q.levels())], x=Q.apply(b), xt=Q.apply(b, O.TRANSPOSE), total_nnz=Q.total_nnz())
        for env in ({}, {"ILUPP_DP_STORE": str(C.STORE)}):
            with Env(ILUPP_DEBUG="1", **env), Stderr() as cap:
                got = _measure(_native.MultilevelILUCDPPreconditioner(val, idx, ptr, True, ml_cases.engine_params(ilupp, c.threshold, (), kn)), n)
            kinds = [(w, int(s)) for _, _, w, s, _ in _LINE.findall(cap.err)]
            assert ("LDS", 4) in kinds and ("memory", 0) in kinds, (name, rule, env, kinds)
            assert not env or any(w == "memory" and s in (1, 2, 3) for w, s in kinds), (name, rule, kinds)
            _judge(got, want, (name, rule, tuple(env)))


def test_fuzz_with_the_vectors_in_memory():
    """random matrices and parameters (every dropping rule, preprocessing, windows, level ends) against the oracle, k_pilucdp from the first
    step, every second one with small stores as well"""
    import ilupp_amd as ilupp
    from ilupp_amd import _native
    from oracle import oracle as O
    rng = np.random.default_rng(20240611)
    seen = 0
    for it in range(40):
        n = int(rng.integers(3, 300))
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
        family = int(rng.integers(0, 4))
        if family == 1:
            knobs.update(USE_STANDARD_DROPPING=bool(rng.integers(0, 2)), USE_PIVOT_DROPPING=bool(rng.integers(0, 2)), USE_ERR_PROP_DROPPING2=bool(rng.integers(0, 2)),
                         COMBINE_FACTOR=int(rng.integers(0, 4)))
        elif family == 2:
            knobs.update(USE_WEIGHTED_DROPPING=bool(rng.integers(0, 2)), USE_WEIGHTED_DROPPING2=bool(rng.integers(0, 2)),
                         WEIGHT_WEIGHTED_DROP=float(rng.choice([1.0, 0.2])), INIT_WEIGHTS_LU=float(rng.choice([1.0, 0.5, 2.0])))
        elif family == 3:
            knobs.update(USE_INVERSE_DROPPING=True, USE_ERR_PROP_DROPPING=bool(rng.integers(0, 2)), WEIGHT_INVERSE_DROP=float(rng.choice([1.0, 0.3, 3.0])))
        pre = [("PQ_ORDERING",), ("MAX_WEIGHTED_MATCHING_ORDERING",), ("NORMALIZE_COLUMNS", "NORMALIZE_ROWS", "PQ_ORDERING"), ("SPARSE_FIRST_ORDERING",), ()][int(rng.integers(0, 5))]
        thr = float(rng.choice([0.0, 1e-3, 1e-2, 0.1, 1.0]))
        ep = ml_cases.engine_params(ilupp, thr, pre, knobs)
        if ep._uses_partial_iluc():
            continue
        Q = O.orc().ml(a, ml_cases.oracle_params(O, thr, pre, knobs))
        b = ml_cases.rhs(n)
        want = dict(levels=[ml_cases.level_arrays(Q.level(k)) for k in range(Q.levels())], x=Q.apply(b), xt=Q.apply(b, O.TRANSPOSE), total_nnz=Q.total_nnz())
        env = {"ILUPP_NO_DPLDS": "1"}
        if it % 4 < 2:
            env["ILUPP_DP_STORE"] = "20"
        with Env(ILUPP_DEBUG="1", **env), Stderr() as cap:
            got = _measure(_native.MultilevelILUCDPPreconditioner(a[0], a[1], a[2], a[3], ep), n)
        assert set(w for _, _, w, _, _ in _LINE.findall(cap.err)) == {"memory"}, (it, cap.err[-1000:])
        tag = (it, n, pre, thr, tuple(sorted(knobs.items())))
        assert len(got["levels"]) == len(want["levels"]) and got["total_nnz"] == want["total_nnz"], tag
        for k, (u, v) in enumerate(zip(got["levels"], want["levels"])):
            for q, (x, y) in enumerate(zip(u, v)):
                assert np.array_equal(x, y, equal_nan=(np.asarray(x).dtype.kind == "f")), tag + (k, q)
        assert np.array_equal(got["x"], want["x"], equal_nan=True) and np.array_equal(got["xt"], want["xt"], equal_nan=True), tag
        seen += 1
    assert seen >= 25
