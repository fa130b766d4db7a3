"""GPU tests of the batched apply of the two pivoting classes (ilupp_amd.apply_batch / ilupp_amd.device.pivot_apply_batch_ over
ilupp_hip_pivot_apply_batch / ilupp_hip_pivot_apply_batch_device: one launch of k_pivot_apply_batch, one workgroup per member with the
permutation and both sweeps inside it) and of the single device apply (ilupp_hip_ilucp_apply_device).  Every result is the single
apply's, bit for bit: against tests/golden/ilucp.npz / ilutp.npz, against P @ b, across the LDS cap and its fallback, with more members
than CUs, with both hand-overs between the sweeps, on device tensors between a producer and a consumer, next to a member full of NaN;
and sixteen members side by side take less time than the loop over them."""
import ctypes
import os
import time

import numpy as np
import pytest
import scipy.sparse as sp

import matgen
import ml_cases as C

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(100, 0.1, 0.1), (100, 0.0, 0.0), (3, 1e-3, 1.0), (8, 1e-2, 0.5), (1, 0.1, 0.1)]          # = test_gpu_pivot_batch.py
NAMES = ["laplace2d", "random", "rdd_300", "weak_200", "offdiag_150"]
KINDS = ["ilucp", "ilutp"]
N_SIDE = 12000                                                                                     # = test_gpu_pivot_batch.py


def _cls(kind):
    import ilupp_amd as ilupp
    return ilupp.ILUCPPreconditioner if kind == "ilucp" else ilupp.ILUTPPreconditioner


def _random(n, seed, fmt, diag=3.0):
    rng = np.random.default_rng(seed)
    A = (sp.random(n, n, min(1.0, 6.0 / n), random_state=rng, data_rvs=lambda k: rng.standard_normal(k)) + sp.eye(n) * diag).asformat(fmt)
    A.sort_indices()
    return A


def _dd(n, seed, fmt="csr"):
    return sp.csr_matrix(matgen.random_dd(n, 8, 25.0, seed), shape=(n, n)).asformat(fmt)


def _band(n, seed):
    """rows of 2 - 3 entries: a random tridiagonal matrix with a heavy diagonal (its construction is a short chain per row)"""
    rng = np.random.default_rng(seed)
    A = sp.diags([rng.standard_normal(n - 1), 4.0 + rng.random(n), rng.standard_normal(n - 1)], [-1, 0, 1], format="csr")
    A.sort_indices()
    return A


def _routes(B, rhs, transpose):
    """the routes the native call reports for these members (on copies of the right-hand sides)"""
    from ilupp_amd import _native
    return _native.pivot_apply_batch([P.pr for P in B], [b.copy() for b in rhs], transpose)


def _check_against_the_loop(B, rhs, tag):
    """apply_batch in both directions equals P @ b / P.T @ b of every member; returns the two result lists"""
    import ilupp_amd as ilupp
    keep = [b.copy() for b in rhs]
    Y, YT = ilupp.apply_batch(B, rhs), ilupp.apply_batch(B, rhs, transpose=True)
    assert len(Y) == len(B) and len(YT) == len(B)
    for k, (P, b) in enumerate(zip(B, rhs)):
        assert np.array_equal(b, keep[k], equal_nan=True), (tag, k)                # (the inputs are not modified)
        assert Y[k] is not b and np.array_equal(Y[k], P @ b, equal_nan=True), (tag, k, "apply")
        assert np.array_equal(YT[k], P.T @ b, equal_nan=True), (tag, k, "apply_trans")
    return Y, YT


# ---- 1. the golden arrays ----
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("kind", KINDS)
def test_batched_apply_gives_the_golden_arrays(kind, fmt):
    """the five matrices of the golden file (n = 150 - 400) + random members of n = 1, 2, 65 (one past a wave) and 257 (one past the
    workgroup) in ONE batch, every parameter set of CASES: apply_batch equals the reference's apply / apply_trans arrays and P @ b /
    P.T @ b of every member, and every member takes the launch (both factors of these classes store their unit or pivot entry in every
    row: none is degenerate)"""
    cls = _cls(kind)
    gold = np.load(os.path.join(HERE, "golden", "%s.npz" % kind))
    kindm = sp.csr_matrix if fmt == "csr" else sp.csc_matrix
    mats = []
    for name in NAMES:
        key = "%s_%s" % (name, fmt)
        n = gold[key + "/indptr"].shape[0] - 1
        mats.append(kindm((gold[key + "/data"].copy(), gold[key + "/indices"].copy(), gold[key + "/indptr"].copy()), shape=(n, n)))
    mats += [_random(1, 70, fmt), _random(2, 71, fmt), _random(65, 72, fmt), _random(257, 73, fmt)]
    rhs = [C.rhs(A.shape[0]) for A in mats]
    for fill, thr, tol in CASES:
        tag = (kind, fmt, fill, thr, tol)
        B = cls.batch(mats, fill_in=fill, threshold=thr, piv_tol=tol)
        Y, YT = _check_against_the_loop(B, rhs, tag)
        for k, name in enumerate(NAMES):
            g = "%s_%s/f%d_t%g_p%g" % (name, fmt, fill, thr, tol)
            assert np.array_equal(Y[k], gold[g + "/apply"], equal_nan=True), (tag, name)
            assert np.array_equal(YT[k], gold[g + "/apply_trans"], equal_nan=True), (tag, name)
        assert _routes(B, rhs, False) == [0] * len(B), tag
        assert _routes(B, rhs, True) == [0] * len(B), tag


# ---- 2. the cap and the fallback ----
def test_members_past_the_cap_take_the_single_apply(monkeypatch):
    """ILUPP_BATCH_APPLY_MAX_N = 128: members of n = 64 and 128 take the launch (the first with both arrays in LDS, the second with one
    and the hand-over through memory: 16 n against the 1 024 bytes of the lowered cap), n = 129 and 300 the single apply inside the
    same call; all four results are the single applies'.  Both classes in one call.  And the library refuses a wrong length."""
    import ilupp_amd as ilupp
    from ilupp_amd import _native
    monkeypatch.setenv("ILUPP_BATCH_APPLY_MAX_N", "128")
    assert _native.pivot_apply_batch_max_n() == 128
    mats = [_random(n, 400 + k, "csr") for k, n in enumerate([64, 128, 129, 300])]
    B = [ilupp.ILUCPPreconditioner(mats[0]), ilupp.ILUTPPreconditioner(mats[1]), ilupp.ILUCPPreconditioner(mats[2]), ilupp.ILUTPPreconditioner(mats[3])]
    rhs = [C.rhs(A.shape[0]) for A in mats]
    assert _routes(B, rhs, False) == [0, 0, 1, 1]
    assert _routes(B, rhs, True) == [0, 0, 1, 1]
    _check_against_the_loop(B, rhs, "cap")
    # a wrong length: refused with the reference's text, nothing touched
    lib = _native.lib()
    x = [b.copy() for b in rhs]
    H = (ctypes.c_void_p * 4)(*[P.pr._h.value for P in B])
    X = (ctypes.c_void_p * 4)(*[a.ctypes.data for a in x])
    N = (ctypes.c_int64 * 4)(64, 128, 128, 300)
    assert lib.ilupp_hip_pivot_apply_batch(4, H, X, N, 0, None) == -2                          # ILUPP_ERR_WRONG_SIZE
    assert lib.ilupp_hip_last_error().decode() == "vector has wrong size for preconditioner!"
    assert all(np.array_equal(a, b) for a, b in zip(x, rhs))
    with pytest.raises(ValueError, match="vector of 63 elements for a preconditioner of dimension 64"):
        ilupp.apply_batch(B[:1], [np.ones(63)])
    # a member named twice: its scratch vector serves one apply at a time
    H2 = (ctypes.c_void_p * 2)(B[0].pr._h.value, B[0].pr._h.value)
    assert lib.ilupp_hip_pivot_apply_batch(2, H2, X, N, 0, None) == -1


# ---- 3. more members than CUs ----
def test_more_members_than_compute_units():
    """300 ILUTP members of n = 40 with distinct seeds: one launch of 300 workgroups on 256 CUs"""
    cls = _cls("ilutp")
    mats = [_random(40, 1000 + k, "csr") for k in range(300)]
    B = cls.batch(mats)
    rhs = [C.rhs(40) * (1.0 + k / 64.0) for k in range(300)]
    _check_against_the_loop(B, rhs, "300")
    assert _routes(B, rhs, False) == [0] * 300
    assert _routes(B, rhs, True) == [0] * 300


# ---- 4. both hand-overs between the sweeps ----
@pytest.mark.parametrize("kind", KINDS)
def test_both_hand_overs_between_the_sweeps(kind, monkeypatch):
    """the kernel keeps the first sweep's result in a second LDS array when 16 n bytes fit and passes it through memory otherwise: with
    the device's cap N (8 N bytes of LDS), n = N // 2 is the largest member of the first kind and n = N // 2 + 1 the smallest of the
    second; both in one call, rows of 2 - 3 entries"""
    from ilupp_amd import _native
    monkeypatch.delenv("ILUPP_BATCH_APPLY_MAX_N", raising=False)
    cap = _native.pivot_apply_batch_max_n()
    assert cap >= 1024, cap
    mats = [_band(cap // 2, 11), _band(cap // 2 + 1, 12)]
    B = _cls(kind).batch(mats)
    rhs = [C.rhs(A.shape[0]) for A in mats]
    print("%s: cap %d, members of n = %d (two LDS arrays) and %d (one, through memory)" % (kind, cap, cap // 2, cap // 2 + 1))
    _check_against_the_loop(B, rhs, (kind, cap))
    assert _routes(B, rhs, False) == [0, 0] and _routes(B, rhs, True) == [0, 0]


# ---- 5. the device entries ----
@pytest.mark.parametrize("transpose", [False, True])
def test_device_entry_between_a_producer_and_a_consumer(transpose):
    """one packed tensor with gaps between the vectors, filled on a side stream without a sync; pivot_apply_batch_ on that stream; a
    consumer kernel behind it: the results equal the host path, the gaps keep their bits"""
    import torch
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    ns = [150, 65, 257, 40]
    mats = [_random(n, 500 + k, "csr") for k, n in enumerate(ns)]
    B = [(ilupp.ILUCPPreconditioner if k % 2 == 0 else ilupp.ILUTPPreconditioner)(A) for k, A in enumerate(mats)]
    rhs = [C.rhs(n) for n in ns]
    want = ilupp.apply_batch(B, rhs, transpose=transpose)
    gap = 7
    offsets, total = [], gap
    for n in ns:
        offsets.append(total)
        total += n + gap
    pattern = np.int64(0x7FF4DEADBEEF0123)                   # (a signalling NaN's bits: arithmetic on it would not give it back)
    host = np.full(total, pattern, dtype=np.int64)
    for o, b in zip(offsets, rhs):
        host[o:o + b.shape[0]] = b.view(np.int64)
    src = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = torch.empty(total, dtype=torch.int64, device="cuda")
        x.copy_(src, non_blocking=True)                      # the producer: no sync behind it
        routes = ild.pivot_apply_batch_(B, x.view(torch.float64), offsets, transpose=transpose)
        out = x.clone()                                      # the consumer
    side.synchronize()
    got = out.cpu().numpy()
    assert routes == [0, 0, 0, 0]
    mask = np.ones(total, dtype=bool)
    for o, n, w in zip(offsets, ns, want):
        assert np.array_equal(got[o:o + n].view(np.float64), w, equal_nan=True), (o, n)
        mask[o:o + n] = False
    assert np.all(got[mask] == pattern)
    with pytest.raises(ValueError):
        ild.pivot_apply_batch_(B, x.view(torch.float64), [0, 0, 0, total], transpose=transpose)
    with pytest.raises(TypeError):
        ild.pivot_apply_batch_([object()], x.view(torch.float64), [0])


@pytest.mark.parametrize("kind", KINDS)
def test_single_device_apply_equals_apply(kind):
    """PivotedPreconditioner.apply_device on a device vector, both directions, on torch's current stream"""
    import torch
    from ilupp_amd import _native
    A = _random(300, 600, "csc")
    P = _cls(kind)(A)
    b = C.rhs(300)
    for transpose in (False, True):
        want = b.copy()
        (P.apply_trans if transpose else P.apply)(want)
        t = torch.from_numpy(b.copy()).cuda()
        _native.set_caller_stream(torch.cuda.current_stream().cuda_stream, True)
        P.pr.apply_device(t.data_ptr(), 300, transpose=transpose, sync=False)
        assert np.array_equal(t.cpu().numpy(), want, equal_nan=True), (kind, transpose, "sync=False")
        t = torch.from_numpy(b.copy()).cuda()
        P.pr.apply_device(t.data_ptr(), 300, transpose=transpose, sync=True)
        assert np.array_equal(t.cpu().numpy(), want, equal_nan=True), (kind, transpose, "sync=True")
    with pytest.raises(RuntimeError, match="vector has wrong size for preconditioner!"):
        P.pr.apply_device(t.data_ptr(), 299)


# ---- 6. isolation ----
def test_a_member_full_of_nan_leaves_the_others_alone():
    """one member's right-hand side holds NaN and Inf: the other members' results keep their bits, and the member itself gets what its
    single apply gives"""
    import ilupp_amd as ilupp
    mats = [_random(n, 700 + k, "csr") for k, n in enumerate([200, 200, 129, 64])]
    B = [ilupp.ILUCPPreconditioner(mats[0]), ilupp.ILUTPPreconditioner(mats[1]), ilupp.ILUCPPreconditioner(mats[2]), ilupp.ILUTPPreconditioner(mats[3])]
    clean = [C.rhs(A.shape[0]) for A in mats]
    for bad in (0, 1):
        dirty = [b.copy() for b in clean]
        dirty[bad][3] = np.nan
        dirty[bad][77] = np.inf
        dirty[bad][150] = -np.inf
        for transpose in (False, True):
            Yc = ilupp.apply_batch(B, clean, transpose=transpose)
            Yd = ilupp.apply_batch(B, dirty, transpose=transpose)
            for k in range(4):
                if k != bad:
                    assert np.array_equal(Yd[k].view(np.int64), Yc[k].view(np.int64)), (bad, transpose, k)
            alone = (B[bad].T if transpose else B[bad]) @ dirty[bad]
            assert np.array_equal(Yd[bad], alone, equal_nan=True), (bad, transpose)
            assert not np.all(np.isfinite(Yd[bad]))


# ---- 7. side by side, in wall time ----
def test_sixteen_applies_side_by_side_beat_the_loop():
    """16 ILUCP members of n = N_SIDE: one batched call against the same 16 vectors applied one by one with `apply` on the same objects;
    medians of five repetitions after a warm-up call of each"""
    import ilupp_amd as ilupp
    from ilupp_amd import _native
    n = min(N_SIDE, _native.pivot_apply_batch_max_n())      # (lowered only where the device's LDS cap is smaller)
    big = [_dd(n, 500 + k) for k in range(16)]
    B = ilupp.ILUCPPreconditioner.batch(big)
    rhs = [C.rhs(n) * (1.0 + k / 16.0) for k in range(16)]

    def batched():
        t0 = time.perf_counter()
        Y = ilupp.apply_batch(B, rhs)
        return time.perf_counter() - t0, Y

    def looped():
        t0 = time.perf_counter()
        Y = []
        for P, b in zip(B, rhs):
            x = b.copy()
            P.apply(x)
            Y.append(x)
        return time.perf_counter() - t0, Y

    _, Yb = batched()
    _, Yl = looped()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(Yb, Yl))
    assert _routes(B, rhs, False) == [0] * 16
    if n > 4096:
        # (a member of this size that would have the launch to itself takes the single apply: one workgroup needs 0.24 ms where the single
        # apply's sweeps need 0.12 -- profiles/r10_pivot_apply_batch.txt; two members break even, from four on the launch wins)
        assert _routes(B[:1], rhs[:1], False) == [1] and _routes(B[:2], rhs[:2], False) == [0, 0]
        assert np.array_equal(ilupp.apply_batch(B[:1], rhs[:1])[0], Yl[0], equal_nan=True)
    t_batch = float(np.median([batched()[0] for _ in range(5)]))
    t_loop = float(np.median([looped()[0] for _ in range(5)]))
    print("ilucp n %d x 16: t_batch %.5f s, t_loop %.5f s" % (n, t_batch, t_loop))
    assert t_batch < t_loop, (t_batch, t_loop)
