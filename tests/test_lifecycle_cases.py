"""Preconditions of the apply-state lifecycle tests (test_gpu_apply_lifecycle.py), on the CPU: a test that compares with the oracle's
result for the CURRENT value set sees a stale copy only if the value sets give different answers -- so they must, in every row; the
sequences must be what they claim; and the expected result must be a function of the current value set and the operation alone."""
import numpy as np
import pytest

import lifecycle_cases as LC

REFACTOR_CASES = [c for c in LC.CASES if c.refactor]


@pytest.mark.parametrize("case", REFACTOR_CASES, ids=[c.name for c in REFACTOR_CASES])
def test_value_sets_differ_in_every_row(case):
    """every pair of value sets, both directions, every right-hand side of the pool: the oracle's applies share no finite row's bits
    (the NaN column is exempt: NaN spreads the same way whatever the values are); the factors differ too (F)"""
    assert case.sets == LC.K_SETS and case.matrix[2].shape[0] - 1 == case.n
    finite = [j for j in range(LC.POOL) if j != LC.NAN_COL]
    cols = [LC.oracle_columns(case, k) for k in range(case.sets)]
    for k in range(case.sets):
        for j in range(k + 1, case.sets):
            assert not np.array_equal(LC.values(case, k), LC.values(case, j))
            for direction in (0, 1):
                a, b = cols[k][direction][:, finite], cols[j][direction][:, finite]
                assert np.isfinite(a).all() and np.isfinite(b).all(), (case.name, k, j, direction)
                same = LC.bits(a) == LC.bits(b)
                assert not same.any(), (case.name, k, j, direction, np.argwhere(same)[:5].tolist())
            for fk, fj in zip(LC.oracle_factors(case, k), LC.oracle_factors(case, j)):
                assert np.array_equal(fk[1], fj[1]) and np.array_equal(fk[2], fj[2])          # one pattern
                assert not np.array_equal(fk[0], fj[0])
    # ... hence no operation's expected result can be mistaken for another set's, and diagnose names the right one
    for op in case.alphabet:
        for idx, want in enumerate(LC.expected(case, 1, op)):
            if op in ("C", "Ct") and idx == 1:
                continue                                                                     # (the twin never changes)
            assert LC.diagnose(case, 0, op, idx, want) == "equals the result under value set 1: a stale copy of v1"
            assert LC.diagnose(case, 1, op, idx, want) == "equals the result under no other value set"


def test_pool_and_value_sets():
    case = LC.BY_NAME["batch_member"]
    X = LC.rhs_pool(case.n)
    assert X.shape == (case.n, LC.POOL) and np.isnan(X[case.n // 3, LC.NAN_COL]) and np.isnan(X).sum() == 1
    assert not X.flags.writeable and not LC.values(case, 1).flags.writeable and not LC.oracle_columns(case, 0)[0].flags.writeable
    v0 = LC.values(case, 0)
    assert np.array_equal(v0, case.matrix[0])
    for k in (1, 2):
        r = LC.values(case, k) / v0
        assert (r >= 1.0).all() and (r < 1.25 + 1e-12).all()
    assert LC.B3_COLS[-1] == LC.NAN_COL
    with pytest.raises(AssertionError):
        LC.values(LC.BY_NAME["ilut"], 1)                       # a kind without R has the given set alone


def test_alphabets_and_fixed_sequences():
    for case in LC.CASES:
        assert ("R" in case.alphabet) == (case.kind == "ILU0")
        assert ("C" in case.alphabet) == ("Ct" in case.alphabet) == (case.n <= LC.BATCH_CAP_N)
        seqs = LC.fixed_sequences(case)
        assert len(set(seqs.values())) == len(seqs) and all(seqs.values())
        for num, toks in seqs.items():
            assert set(toks) <= set(case.alphabet)
            # the case's sequence is the issue's with the operations it lacks left out, in order
            assert toks == tuple(t for t in LC.parse(LC.FIXED[num]) if t in case.alphabet)
        assert (6 in seqs) == case.small
        if case.refactor:
            assert sorted(seqs) == [n for n in sorted(LC.FIXED) if n != 6 or case.small]
            assert all(seqs[n] == LC.parse(LC.FIXED[n]) for n in seqs)
    with pytest.raises(ValueError):
        LC.parse("a x")


def test_random_sequences_are_deterministic_and_respect_the_alphabet(monkeypatch):
    monkeypatch.delenv("ILUPP_FUZZ_OFFSET", raising=False)
    seen = set()
    for case in LC.CASES:
        seqs = LC.random_sequences(case)
        assert seqs == LC.random_sequences(case) and len(seqs) == 2
        for s in seqs:
            assert len(s) == LC.SEQ_LEN and set(s) <= set(case.alphabet) and s.count("R") <= LC.MAX_R
            seen.add((case.name, s))
    assert len(seen) == 2 * len(LC.CASES)
    # the cap on R holds where R is all there is to draw more of, and the seed decides everything
    for seed in range(50):
        s = LC.random_sequence(("a", "R"), seed)
        assert s.count("R") <= LC.MAX_R and s == LC.random_sequence(("a", "R"), seed)
    assert len({LC.random_sequence(LC.OPS, seed) for seed in range(20)}) > 1
    assert any(s.count("R") == LC.MAX_R for s in (LC.random_sequence(("a", "R"), seed) for seed in range(50)))
    # ILUPP_FUZZ_OFFSET shifts the seeds
    case = LC.CASES[0]
    base = LC.random_sequences(case)
    monkeypatch.setenv("ILUPP_FUZZ_OFFSET", "1")
    assert LC.random_sequences(case)[0] == base[1] and LC.random_sequences(case) != base


def test_expected_depends_on_the_current_set_and_the_operation_alone():
    case = LC.BY_NAME["batch_member"]
    # two histories that end on the same value set: every operation's expected result is the same, bit for bit
    m1, m2 = LC.Model(case), LC.Model(case)
    for op in LC.parse("a t R B9 C"):
        m1.step(op)
    for op in LC.parse("R R F AA R Bt3 R T"):
        m2.step(op)
    assert m1.cur == m2.cur == 1
    for op in case.alphabet:
        if op == "R":
            continue
        e1, e2 = m1.step(op), m2.step(op)
        assert len(e1) == len(e2) and all(LC.same_bits(x, y) for x, y in zip(e1, e2)), op
        assert all(LC.same_bits(x, y) for x, y in zip(e1, LC.expected(case, 1, op)))
    # R moves to the next set, cyclically; nothing else moves
    m = LC.Model(case)
    order = []
    for op in LC.parse("a R t R B3 R F R"):
        m.step(op)
        order.append(m.cur)
    assert order == [0, 1, 1, 2, 2, 0, 0, 1]
    # the results are the oracle's applies of the pool's columns on the factors of that set, per operation
    from oracle import oracle as O
    L, U = LC.oracle_factors(case, 2)
    X = LC.rhs_pool(case.n)
    assert LC.same_bits(LC.expected(case, 2, "a")[0], O.orc().apply_lu(L, U, X[:, 0], O.ID))
    assert LC.same_bits(LC.expected(case, 2, "T")[0], O.orc().apply_lu(L, U, X[:, 1], O.TRANSPOSE))
    assert LC.same_bits(LC.expected(case, 2, "TA")[1], O.orc().apply_lu(L, U, X[:, 2], O.ID))
    assert LC.same_bits(LC.expected(case, 2, "Bt3")[0][:, 2], O.orc().apply_lu(L, U, X[:, LC.NAN_COL], O.TRANSPOSE))
    assert LC.expected(case, 2, "B9")[0].shape == (case.n, 9) and LC.expected(case, 2, "R") == []
    assert LC.same_bits(LC.expected(case, 2, "F")[1], U[0])
