"""The CPU model of the two pivoting chains (tests/pivot_ref.py) against the oracle, the oracle against the reference, and the cases of
tests/pivot_cases.py against the figures that put them on their boundaries -- all without a GPU:
* the model has the oracle's bits on every case and on the fuzz distribution of test_gpu_ilucp.py / test_gpu_ilutp.py (index and pointer
  arrays, values as uint64, the permutation, the zero-pivot count, the error code);
* every case's pin holds: the model's records show what the case's name says;
* the ordered sums are discriminating (the reversed and the pairwise sum of the same 65 / 129 terms have other bits and decide the tested
  entry the other way) and so are the columns stored twice (the copies swapped: other bits from the oracle);
* the oracle agrees with the reference on every case, factors and both applies (ref_replay.ref(): oracle/_ref where it is built, else
  the digests of tests/golden/ref_live.npz);
* the working row of ILUTP never holds more than n + 1 slots, a quarter of its capacity at the most (status 12 is not reachable)."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import ml_cases
import pivot_cases as C
import pivot_ref as R
import ref_replay
from oracle import oracle as O


_LONG = R.tp_cap(2)            # the slots of ILUTP's working row at n = 2: 256


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle_cls(kind):
    return O.ILUTP if kind == "tp" else O.ILUCP


def _same_as_model(m, build, tag):
    """`build()` gives the oracle's object or raises its error: the model predicted either, bit for bit"""
    try:
        Q = build()
    except O.OracleError as e:
        assert m.err == e.code, tag + ("error", m.err, e.code)
        return None
    assert m.err == R.OK, tag + ("the model raises", m.err, "in", m.err_at)
    assert np.array_equal(m.perm, Q.perm) and m.zero_pivots == Q.zero_pivots, tag
    for t, got, want in (("L", m.L, Q.L), ("U", m.U, Q.U)):
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]), tag + (t, "pattern")
        assert np.array_equal(_u64(got[0]), _u64(want[0])), tag + (t, "values")
    return Q


@pytest.mark.parametrize("name", C.NAMES)
def test_model_has_the_oracles_bits(name):
    c = C.CASES[name]
    ptr, idx, val = C.arrays(name)
    m = C.model(name)
    for is_csr in (True, False):            # (one set of arrays under both labels: the same factorisation of the major-order view)
        Q = _same_as_model(m, lambda: _oracle_cls(c.kind)(O.orc(), (val, idx, ptr, is_csr), **c.params), (name, is_csr))
        if Q is not None:                   # every stored row of U keeps its pivot, so both solves are defined
            assert np.all(np.diff(Q.U[2]) >= 1) and np.all(np.diff(Q.L[2]) >= 1), name


@pytest.mark.parametrize("name", C.NAMES)
def test_case_is_on_its_boundary(name):
    m = C.model(name)
    f = R.route(m.records)
    assert bool(C.CASES[name].pin(m, f, m.records)), (name, m.err, m.err_at, m.err_store, dict(f))
    if m.err != R.OK:
        assert len(m.records) == m.err_at + 1 and (m.err_store in ("L", "U")) == (m.err == R.ERR_MEMORY), name


@pytest.mark.parametrize("name", C.NAMES)
def test_oracle_agrees_with_the_reference(name):
    c = C.CASES[name]
    ptr, idx, val = C.arrays(name)
    ref = ref_replay.ref()
    b = ml_cases.rhs(ptr.shape[0] - 1)
    for is_csr in (True, False):
        a = (val, idx, ptr, is_csr)
        try:
            Q = (ref.ILUTP if c.kind == "tp" else ref.ILUCP)(a, **c.params)
        except O.OracleError as e:
            with pytest.raises(O.OracleError) as e2:
                _oracle_cls(c.kind)(O.orc(), a, **c.params)
            assert e2.value.code == e.code, (name, is_csr)
            continue
        P = _oracle_cls(c.kind)(O.orc(), a, **c.params)
        assert np.array_equal(P.perm, Q.perm), (name, is_csr)
        for x, y in zip(P.L + P.U, Q.L + Q.U):
            assert np.array_equal(_u64(x), _u64(y)) if x.dtype.kind == "f" else np.array_equal(x, y), (name, is_csr)
        for use in (O.ID, O.TRANSPOSE):
            assert np.array_equal(P.apply(b, use), Q.apply(b, use), equal_nan=True), (name, is_csr, use)


def _fuzz(seed=4242, count=70):
    """the matrices and parameters of test_fuzz_against_the_oracle (test_gpu_ilucp.py, test_gpu_ilutp.py)"""
    rng = np.random.default_rng(seed)
    for it in range(count):
        n = int(rng.integers(2, 400))
        A = (sp.random(n, n, min(1.0, rng.uniform(2, 9) / n), random_state=rng, data_rvs=lambda k: rng.standard_normal(k))
             + sp.eye(n) * float(rng.choice([0.0, 0.3, 3.0]))).asformat("csr" if it % 2 else "csc")
        A.sort_indices()
        kw = dict(fill_in=int(rng.choice([1, 2, 5, 100])), threshold=float(rng.choice([0.0, 1e-3, 0.1, 0.5])), piv_tol=float(rng.choice([0.0, 0.1, 1.0])),
                  rp=int(rng.choice([-1, 0, n // 2])), mem_factor=float(rng.choice([10.0, 10.0, 1.0])))
        yield it, (A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32), bool(it % 2)), kw


@functools.lru_cache(maxsize=None)
def _fuzz_models(kind):
    """the model's results on the fuzz sample, (it, input, parameters, result) each: computed once, whichever test asks first"""
    return [(it, a, kw, (R.ilutp if kind == "tp" else R.ilucp)(a[2], a[1], a[0], **kw)) for it, a, kw in _fuzz()]


@pytest.mark.parametrize("kind", ["tp", "cp"])
def test_model_on_the_fuzz_distribution(kind):
    errors = 0
    for it, a, kw, m in _fuzz_models(kind):
        errors += m.err != R.OK
        _same_as_model(m, lambda: _oracle_cls(kind)(O.orc(), a, **kw), (kind, it))
    assert errors >= 3, errors


@pytest.mark.parametrize("name", sorted(C.ORDERS))
def test_the_order_of_the_sum_decides(name):
    count, terms_of, a, dec = C.ORDERS[name]
    m = C.model(name)
    terms = terms_of(m.records)
    assert len(terms) == count
    seq, rev, pair = C.sums(terms)
    assert len({_u64(x).item() for x in (seq, rev)}) == 2 and _u64(pair).item() != _u64(seq).item(), (name, seq.hex(), rev.hex(), pair.hex())
    tau = C.CASES[name].params["threshold"]
    mine = dec(a, tau * math.sqrt(seq))
    assert dec(a, tau * math.sqrt(rev)) != mine and dec(a, tau * math.sqrt(pair)) != mine, name
    # and the model (so the oracle: test_model_has_the_oracles_bits) decided as the ordered sum says
    if name.startswith("tp/unorm"):
        assert (1 in m.U[1][m.U[2][0]:m.U[2][1]]) == mine, name                     # column 1 of the U row of row 0
    elif name.startswith("tp/"):
        assert (0 in m.records[-1]["dropped_cols"]) == mine, name                   # column 0 of the last row
    elif "wnorm" in name:
        assert (1 in m.L[1][m.L[2][0]:m.L[2][1]]) == mine, name                     # row 1 of the L column of step 0
    else:
        assert (1 in m.U[1][m.U[2][0]:m.U[2][1]]) == mine, name                     # column 1 of the U row of step 0


@pytest.mark.parametrize("name", sorted(C.SWAPS))
def test_swapped_copies_give_other_bits(name):
    """a column stored twice keeps its LAST value: exchanging the values of two copies changes the oracle's factors"""
    c = C.CASES[name]
    ptr, idx, val = C.arrays(name)
    start = ptr[len(ptr) - 2] if c.kind == "tp" else ptr[0]            # the row (ILUTP: the last) or slice (ILUCP: slice 0) with the copies
    i, j = (start + q for q in C.SWAPS[name])
    assert idx[i] == idx[j] and val[i] != val[j], name
    swapped = val.copy()
    swapped[i], swapped[j] = val[j], val[i]
    P = _oracle_cls(c.kind)(O.orc(), (val, idx, ptr, True), **c.params)
    Q = _oracle_cls(c.kind)(O.orc(), (swapped, idx, ptr, True), **c.params)
    assert not all(x.shape == y.shape and np.array_equal(_u64(x), _u64(y)) for x, y in ((P.L[0], Q.L[0]), (P.U[0], Q.U[0]))), name


def test_the_long_row_is_dropped_by_the_norm_of_all_copies():
    """dup_long256 / 257: the 128 copies of column 0 all count in the left norm, which drops the value that is kept (the last copy); with
    one copy alone nothing is dropped"""
    for name in ("tp/dup_long256", "tp/dup_long257"):
        assert C.model(name).records[1]["drops"] == 1
    ptr, idx, val = C.slices(2, {0: [(0, 2.0), (1, 1.0)], 1: [(0, 1.5), (1, 4.0)]})
    assert R.ilutp(ptr, idx, val, **C.CASES["tp/dup_long256"].params).records[1]["drops"] == 0


def test_mem_factor_is_truncated():
    """mem19: 1.9 reserves 1 x nnz and fails as overL does; 2 x nnz holds the factors"""
    ptr, idx, val = C.arrays("tp/mem19")
    assert C.model("tp/mem19").err == R.ERR_MEMORY
    assert R.ilutp(ptr, idx, val, **dict(C.CASES["tp/mem19"].params, mem_factor=2.0)).err == R.OK


def test_status_12_is_not_reachable(capsys):
    """the largest ns the model ever saw against the capacity of the working row: a column has one slot (a dropped one never comes
    back), the inserted pivot one more"""
    seen = [(max(r["ns"] for r in m.records), R.tp_cap(a[2].shape[0] - 1), a[2].shape[0] - 1) for it, a, kw, m in _fuzz_models("tp")]
    for name in C.NAMES:
        if name.startswith("tp/"):
            n = C.arrays(name)[0].shape[0] - 1
            seen.append((max(r["ns"] for r in C.model(name).records), R.tp_cap(n), n))
    worst = max(seen, key=lambda t: t[0] / t[1])
    with capsys.disabled():
        print("\nILUTP working row: largest ns / cap = %d / %d (n = %d) over %d runs" % (worst + (len(seen),)))
    assert all(ns <= n + 1 for ns, cap, n in seen) and worst[0] / worst[1] <= 0.25, worst


def test_the_list_covers_the_boundaries():
    """every figure of the issue's list is reached by some case"""
    tp = [R.route(C.model(n).records) for n in C.NAMES if n.startswith("tp/")]
    cp = [R.route(C.model(n).records) for n in C.NAMES if n.startswith("cp/")]

    def union(fs, key):
        out = set()
        for f in fs:
            out.update(f[key])
        return out
    assert {1, 63, 64, 65, 128, 129, _LONG, _LONG + 1} <= {f["max_stored"] for f in tp}
    assert {0, 1, 63, 64, 65, 129} <= union(tp, "ulens") and {64, 65, 66, 129, 130} <= union(tp, "min_search_ns")
    assert {0, 64, 65} <= union(tp, "cL") and {0, 64, 65} <= union(tp, "cU") and {0, 1, 63, 64} <= union(tp, "cutL") and union(tp, "cutU")
    assert any(f["zp_new"] for f in tp) and any(f["zp_reuse"] for f in tp) and any(f["second"] for f in tp) and any(f["nonfinite"] for f in tp)
    assert {C.model(n).err for n in C.NAMES if n.startswith("tp/")} == {R.OK, R.ERR_ZERO_PIVOT, R.ERR_MEMORY}
    assert {(C.model(n).err_store) for n in C.NAMES} == {None, "L", "U"}
    assert {0, 1, 64, 65, 129} <= union(cp, "nrow") and {1, 64, 65, 129} <= union(cp, "zsub_lens") and 131 in union(cp, "wsub_lens")
    # (no ("kept", 1): the kept branch always returns its pivot, so no second pass follows it or becomes it -- pivot_cases.py, not pinned)
    assert {("pivoting", 0), ("pivoting", 1), ("kept", 0), ("neither", 0), ("neither", 1)} == union(cp, "branches")
    tied = [s for n in C.NAMES if n.startswith("tp/") for r in C.model(n).records for s in r["selects"] if s["cutU"] and s["key_before_cut"] == s["max_key"]]
    assert any(len(s["max_ties"]) >= 2 for s in tied)                      # equal maxima on both sides of offU
    assert {0, 1, 63, 64, 65, 128, 129} <= union(cp, "nL") and {0, 65, 66} <= union(cp, "col_len") and 0 in union(cp, "cutL")
    assert max(f["col_dups"] for f in cp) == 2 and max(f["filtered"] for f in cp) >= 65 and any(f["nonfinite"] for f in cp)

