"""GPU tests of the batched construction of the two pivoting classes (ILUCPPreconditioner.batch / ILUTPPreconditioner.batch over
ilupp_hip_ilucp_create_batch / ilupp_hip_ilutp_create_batch: the chains of the members in one launch, one workgroup each -- k_ilucp_batch,
k_ilutp_batch through the combiner of pilucdp.hip).  Every member is the object the constructor builds alone, bit for bit: against the
single builds, against tests/golden/ilucp.npz / ilutp.npz and against the oracle; with more members than workers; with a member that
fails; and the chains do run side by side (one combined launch time for all members, a batch of 16 in well under 16 times one)."""
import gc
import os
import time

import numpy as np
import pytest
import scipy.sparse as sp

import matgen
import ml_cases as C

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(100, 0.1, 0.1), (100, 0.0, 0.0), (3, 1e-3, 1.0), (8, 1e-2, 0.5), (1, 0.1, 0.1)]          # = test_gpu_ilucp.py / test_gpu_ilutp.py
NAMES = ["laplace2d", "random", "rdd_300", "weak_200", "offdiag_150"]
KINDS = ["ilucp", "ilutp"]
# test 6: at n = 12000 one construction takes 0.18 s (ILUCP) / 0.10 s (ILUTP), under the 0.5 s cap, and the chain kernel is 0.99 of it;
# 16 side by side took 0.21 / 0.12 s (profiles/r09_pivot_batch.txt).  The test asserts the cap, the share and the bound.
N_SIDE = 12000


def _cls(kind):
    import ilupp_amd as ilupp
    return ilupp.ILUCPPreconditioner if kind == "ilucp" else ilupp.ILUTPPreconditioner


def _native_batch(kind):
    from ilupp_amd import _native
    return _native.ILUCPPreconditioner_batch if kind == "ilucp" else _native.ILUTPPreconditioner_batch


def _oracle_cls(kind):
    from oracle import oracle as O
    return O.ILUCP if kind == "ilucp" else O.ILUTP


def _random(n, seed, fmt, diag=3.0):
    rng = np.random.default_rng(seed)
    A = (sp.random(n, n, min(1.0, 6.0 / n), random_state=rng, data_rvs=lambda k: rng.standard_normal(k)) + sp.eye(n) * diag).asformat(fmt)
    A.sort_indices()
    return A


def _dd(n, seed, fmt="csr"):
    return sp.csr_matrix(matgen.random_dd(n, 8, 25.0, seed), shape=(n, n)).asformat(fmt)


def _same_native(pb, p1, tag):
    """two native objects: factors, permutation, counts and both solves equal bit for bit"""
    Lb, Ub, permb = pb.raw()
    L1, U1, perm1 = p1.raw()
    for x, y in zip(Lb + Ub, L1 + U1):
        assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), tag
    assert np.array_equal(permb, perm1), tag
    assert pb.total_nnz == p1.total_nnz and pb.zero_pivots == p1.zero_pivots, tag
    b = C.rhs(permb.shape[0])
    for solve in ("apply", "apply_trans"):
        x = b.copy(); getattr(pb, solve)(x)
        y = b.copy(); getattr(p1, solve)(y)
        assert np.array_equal(x, y, equal_nan=True), (tag, solve)


def _same(Pb, P1, tag):
    """two instances of a pivoting class: the native objects, and the Python surface on top of them"""
    _same_native(Pb.pr, P1.pr, tag)
    assert type(Pb) is type(P1) and Pb.shape == P1.shape and Pb.dtype == P1.dtype and repr(Pb) == repr(P1), tag
    b = C.rhs(Pb.shape[0])
    assert np.array_equal(Pb @ b, P1 @ b, equal_nan=True) and np.array_equal(Pb.T @ b, P1.T @ b, equal_nan=True), tag
    for fb, f1 in zip(Pb.factors(), P1.factors()):
        assert fb.format == f1.format and np.array_equal(fb.indptr, f1.indptr) and np.array_equal(fb.indices, f1.indices), tag
        assert np.array_equal(fb.data, f1.data, equal_nan=True), tag
    for qb, q1 in zip(Pb.permutations(), P1.permutations()):
        assert (qb is None and q1 is None) or np.array_equal(qb, q1), tag


# ---- 1. the same objects as built alone, bit for bit ----
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("kind", KINDS)
def test_members_are_the_objects_built_alone(kind, fmt):
    """the five matrices of the golden file (n = 150 - 400) + an n = 2 and an n = 65 (one past a wave) random matrix in ONE batch, every
    parameter set of CASES: raw() (L, U, perm), total_nnz, zero_pivots, apply, apply_trans equal to the single build's, and the golden
    matrices' members equal to the reference's arrays"""
    cls = _cls(kind)
    gold = np.load(os.path.join(HERE, "golden", "%s.npz" % kind))
    kindm = sp.csr_matrix if fmt == "csr" else sp.csc_matrix
    mats = []
    for name in NAMES:
        key = "%s_%s" % (name, fmt)
        n = gold[key + "/indptr"].shape[0] - 1
        mats.append(kindm((gold[key + "/data"].copy(), gold[key + "/indices"].copy(), gold[key + "/indptr"].copy()), shape=(n, n)))
    mats += [_random(2, 71, fmt), _random(65, 72, fmt)]
    for fill, thr, tol in CASES:
        B = cls.batch(mats, fill_in=fill, threshold=thr, piv_tol=tol)
        assert len(B) == len(mats)
        for k, (A, Pb) in enumerate(zip(mats, B)):
            tag = (kind, fmt, k, fill, thr, tol)
            _same(Pb, cls(A, fill_in=fill, threshold=thr, piv_tol=tol), tag)
            if k < len(NAMES):
                g = "%s_%s/f%d_t%g_p%g" % (NAMES[k], fmt, fill, thr, tol)
                L, U, perm = Pb.pr.raw()
                for nm, arr in zip(("L_data", "L_indices", "L_indptr", "U_data", "U_indices", "U_indptr"), L + U):
                    assert np.array_equal(arr, gold[g + "/" + nm], equal_nan=(arr.dtype.kind == "f")), (tag, nm)
                assert np.array_equal(perm, gold[g + "/perm"]), tag
                b = C.rhs(A.shape[0])
                x = b.copy(); Pb.apply(x)
                assert np.array_equal(x, gold[g + "/apply"], equal_nan=True), tag
                x = b.copy(); Pb.apply_trans(x)
                assert np.array_equal(x, gold[g + "/apply_trans"], equal_nan=True), tag


# ---- 2. more members than workers ----
@pytest.mark.parametrize("kind", KINDS)
def test_more_members_than_workers(kind, monkeypatch):
    """8 matrices of mixed size on 3 workers: several combined launches, workers that leave at different times"""
    monkeypatch.setenv("ILUPP_BATCH_WORKERS", "3")
    cls = _cls(kind)
    mats = [_random(n, 300 + k, "csr", diag=(0.3 if k % 3 == 0 else 3.0)) for k, n in enumerate([300, 40, 129, 64, 250, 41, 191, 77])]
    B = cls.batch(mats, threshold=1e-2, piv_tol=0.5)
    assert len(B) == 8
    for k, (A, Pb) in enumerate(zip(mats, B)):
        _same(Pb, cls(A, threshold=1e-2, piv_tol=0.5), (kind, k))


# ---- 3. fuzz against the oracle ----
@pytest.mark.parametrize("kind", KINDS)
def test_fuzz_against_the_oracle(kind):
    """24 random matrices drawn the way test_fuzz_against_the_oracle of test_gpu_ilucp.py / test_gpu_ilutp.py draws them, dealt into SIX
    batches (three of CSR, three of CSC input) of four members of mixed size; every batch has one parameter set drawn from the same
    choices (the row from which every step pivots: none, the first, or half of the batch's smallest n).  Members equal the oracle's
    factors, permutation, apply and apply_trans; a batch with members the oracle refuses raises the first one's error by its number,
    and the batch without them builds"""
    from oracle import oracle as O
    off = int(os.environ.get("ILUPP_FUZZ_OFFSET", "0"))
    rng = np.random.default_rng(9191 + off)
    dealt = [[] for _ in range(6)]
    for it in range(24):
        n = int(rng.integers(2, 400))
        A = (sp.random(n, n, min(1.0, rng.uniform(2, 9) / n), random_state=rng, data_rvs=lambda k: rng.standard_normal(k))
             + sp.eye(n) * float(rng.choice([0.0, 0.3, 3.0]))).asformat("csr" if it % 2 else "csc")
        A.sort_indices()
        dealt[it % 6].append((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32), bool(it % 2)))
    groups = {}
    for g, members in enumerate(dealt):
        assert len(members) == 4 and len({m[3] for m in members}) == 1
        nmin = min(m[2].shape[0] - 1 for m in members)
        kw = (int(rng.choice([1, 2, 5, 100])), float(rng.choice([0.0, 1e-3, 0.1, 0.5])), float(rng.choice([0.0, 0.1, 1.0])),
              int(rng.choice([-1, 0, nmin // 2])), float(rng.choice([10.0, 10.0, 1.0])))
        groups[(kw, members[0][3], g)] = members
    message = "Insufficient memory reserved" if kind == "ilucp" else "memory reserved was insufficient|zero pivot"
    for ((fill, thr, tol, rp, mem), is_csr, _), members in groups.items():
        tag = (kind, fill, thr, tol, rp, mem, is_csr)
        want, good = [], []
        for a in members:
            try:
                want.append(_oracle_cls(kind)(O.orc(), a, fill_in=fill, threshold=thr, piv_tol=tol, rp=rp, mem_factor=mem))
                good.append(a)
            except O.OracleError as e:
                assert e.code in (O.ERR_MEMORY, O.ERR_ZERO_PIVOT)
                want.append(None)
        if len(good) < len(members):
            first = want.index(None)
            with pytest.raises(RuntimeError, match=r"matrix %d of the batch: .*(%s)" % (first, message)):
                _native_batch(kind)([m[:3] for m in members], is_csr, fill, thr, tol, rp, mem)
        B = _native_batch(kind)([m[:3] for m in good], is_csr, fill, thr, tol, rp, mem)
        assert len(B) == len(good)
        for P, Q in zip(B, [q for q in want if q is not None]):
            L, U, perm = P.raw()
            assert np.array_equal(perm, Q.perm), tag
            for x, y in zip(L + U, Q.L + Q.U):
                assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), tag
            assert P.total_nnz == len(Q.L[0]) + len(Q.U[0]) and P.zero_pivots == Q.zero_pivots
            b = C.rhs(perm.shape[0])
            x = b.copy(); P.apply(x)
            assert np.array_equal(x, Q.apply(b), equal_nan=True), tag
            x = b.copy(); P.apply_trans(x)
            assert np.array_equal(x, Q.apply(b, O.TRANSPOSE), equal_nan=True), tag


# ---- 4. a failing member ----
def _sorted_by_the_oracle(kind, kw):
    """random matrices until the oracle has built two and refused one with ERR_MEMORY under `kw` (on the CPU)"""
    from oracle import oracle as O
    rng = np.random.default_rng(77)
    ok, bad = [], None
    for _ in range(200):
        n = int(rng.integers(40, 200))
        A = (sp.random(n, n, min(1.0, rng.uniform(2, 9) / n), random_state=rng, data_rvs=lambda k: rng.standard_normal(k))
             + sp.eye(n) * float(rng.choice([0.0, 0.3, 3.0]))).tocsr()
        A.sort_indices()
        try:
            _oracle_cls(kind)(O.orc(), (A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32), True), **kw)
            if len(ok) < 2:
                ok.append(A)
        except O.OracleError as e:
            if e.code == O.ERR_MEMORY and bad is None:
                bad = A
        if len(ok) == 2 and bad is not None:
            return ok, bad
    raise AssertionError("no matrix that overflows its reservation")


def _fails_alone_and_in_the_middle(kind, ok, bad, message, **kw):
    """`bad` raises `message` when built alone; as the middle member of a batch of three it is reported by its number with that message,
    nothing of the batch stays allocated, and the batch without it gives the single builds"""
    from ilupp_amd import _native
    cls = _cls(kind)
    with pytest.raises(RuntimeError, match=message):
        cls(bad, **kw)
    gc.collect()
    before = _native.live_blocks()
    with pytest.raises(RuntimeError, match=r"matrix 1 of the batch: .*%s.*\(matrix 1 of the batch, status -?\d+\)" % message):
        cls.batch([ok[0], bad, ok[1]], **kw)
    gc.collect()
    assert _native.live_blocks() == before
    B = cls.batch(ok, **kw)
    for k, (A, Pb) in enumerate(zip(ok, B)):
        _same(Pb, cls(A, **kw), (kind, k))


@pytest.mark.parametrize("kind", KINDS)
def test_a_member_that_overflows_its_reservation(kind):
    kw = dict(fill_in=100, threshold=0.1, piv_tol=0.0, mem_factor=1.0)       # (at this threshold the oracle builds some matrices in 1 x nnz and refuses others)
    ok, bad = _sorted_by_the_oracle(kind, dict(kw, rp=-1))
    _fails_alone_and_in_the_middle(kind, ok, bad, "Insufficient memory reserved" if kind == "ilucp" else "memory reserved was insufficient", **kw)


def test_ilutp_member_with_a_zero_pivot():
    """a stored zero on the diagonal of row 7 that a negative pivot tolerance keeps as the pivot: the reference's "encountered zero pivot"."""
    from oracle import oracle as O
    bad = _dd(60, 5)
    bad.sort_indices()
    row = slice(bad.indptr[7], bad.indptr[8])
    bad.data[row][bad.indices[row] == 7] = 0.0
    kw = dict(fill_in=100, threshold=0.1, piv_tol=-0.5, mem_factor=10.0)
    with pytest.raises(O.OracleError) as e:
        O.ILUTP(O.orc(), (bad.data, bad.indices.astype(np.int32), bad.indptr.astype(np.int32), True), rp=-1, **kw)
    assert e.value.code == O.ERR_ZERO_PIVOT
    _fails_alone_and_in_the_middle("ilutp", [_dd(80, 6), _dd(45, 7)], bad, "ILUTP2: encountered zero pivot", **kw)


# ---- 5. side by side, deterministically ----
@pytest.mark.parametrize("kind", KINDS)
def test_sixteen_chains_share_one_launch(kind, monkeypatch):
    """16 members of equal n, as many workers: ONE combined launch, whose time every member reports as its kernel_ms -- and which is less
    than the 16 single chains one after the other"""
    monkeypatch.delenv("ILUPP_BATCH_WORKERS", raising=False)
    cls = _cls(kind)
    mats = [_dd(1500, 900 + k) for k in range(16)]
    cls(mats[0])                                                                    # (warm: pool, code objects)
    B = cls.batch(mats)
    times = [P.pr.kernel_ms for P in B]
    alone = [cls(A).pr.kernel_ms for A in mats]
    print("%s n 1500: combined launch %.3f ms, the 16 single chains %.3f ms in all" % (kind, times[0], sum(alone)))
    assert len(set(times)) == 1 and times[0] > 0.0, times
    assert times[0] < sum(alone), (times[0], alone)
    _same(B[3], cls(mats[3]), (kind, 3))


# ---- 6. side by side, in wall time ----
@pytest.mark.parametrize("kind", KINDS)
def test_sixteen_constructions_in_the_time_of_a_few(kind, monkeypatch):
    """the form and margin of the multilevel test (test_gpu_mlp.py): 16 equal-size matrices, t_batch < 4 t_one, t_one a warm single
    construction in the same process -- at an n where the chain is at least 0.8 of one construction (asserted below)"""
    monkeypatch.delenv("ILUPP_BATCH_WORKERS", raising=False)
    cls = _cls(kind)
    big = [_dd(N_SIDE, 500 + k) for k in range(16)]
    cls(big[0])                                                                     # (warm: pool, code objects)
    t0 = time.perf_counter(); one = cls(big[0]); t_one = time.perf_counter() - t0
    t0 = time.perf_counter(); B = cls.batch(big); t_batch = time.perf_counter() - t0
    print("%s n %d: t_one %.4f s (kernel %.2f ms), t_batch(16) %.4f s (kernel %.2f ms)" % (kind, N_SIDE, t_one, one.pr.kernel_ms, t_batch, B[0].pr.kernel_ms))
    assert t_one < 0.5, t_one
    assert one.pr.kernel_ms >= 0.8 * 1e3 * t_one, (one.pr.kernel_ms, t_one)        # (the chain dominates: what runs side by side is what is timed)
    _same_native(B[0].pr, one.pr, kind)
    assert t_batch < 4.0 * t_one, (t_batch, t_one)
