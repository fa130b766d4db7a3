"""GPU tests of the batched apply of the multilevel ILU++ class (ilupp_amd.ml_apply_batch / ilupp_amd.device.ml_apply_batch_ over
ilupp_hip_ml_apply_batch / ilupp_hip_ml_apply_batch_device: one launch of k_ml_apply_batch, one workgroup per member walking its levels
up and down) and of multilevel members in the batched BiCGstab solve (ilupp_amd.device.bicgstab_batch with MultilevelOperator members
over ilupp_hip_bicgstab_batch_ml_device: k_bicgstab_batch<true>).  Every comparison is on the bits, against the single apply (P @ b,
P.T @ b, apply_device) -- which tests/test_gpu_ml.py and tests/test_gpu_mlp.py pin to the reference -- and against the single solve
device.bicgstab(A_k, b_k[:, None], MultilevelOperator(P_k)).

The matrices are those of tests/ml_cases.py as tests/golden/ml10.npz stores them.  Which parameter set gives how many levels was looked
up with the CPU oracle; the tests do not rely on it: they read P.pr.levels() and assert that the batch holds each kind.  Of the sets the
non-pivoting family was first tried with (t0.05_maxlev3, t0.1, t0.05_noterm on weak_120 / weak_200 / weak_300, t0 on laplace2d_400) the
members come out with one level or with three and more; the member with exactly TWO levels is weak_300 under t0.05_mwm_spq, and the
default-constructed parameters (the pivoting chain) give two levels on every weak_* matrix as well."""
import ctypes
import gc
import os

import numpy as np
import pytest
import scipy.sparse as sp

import ml_cases as C

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PATTERN = np.int64(0x7FF4DEADBEEF0123)          # (a signalling NaN's bits: arithmetic on it would not give it back)
PARAMS = {p[0]: p for p in C.PARAMS}

# (matrix, parameter set of ml_cases.PARAMS) of the members built one by one, family without pivoting
SINGLE = [("laplace2d_400", "t0"), ("weak_120", "t0.05_maxlev3"), ("weak_200", "t0.05_noterm"), ("weak_300", "t0.05_mwm_spq"),
          ("weak_120", "t0.1"), ("weak_300", "t0.1"), ("weak_120", "t1"), ("weak_200", "t0"),
          ("offdiag_150", "t0.05_mwm"), ("offdiag_150", "t0.05_mwm_spq"), ("weak_200", "t0.05_mwm")]
BATCHED = ["weak_120", "weak_300", "weak_200", "rdd_300"]          # ILUppPreconditioner.batch, one parameter set for all


def _gold_matrix(name, fmt="csr"):
    z = np.load(os.path.join(HERE, "golden", "ml10.npz"))
    key = "%s_%s" % (name, fmt)
    n = z[key + "/indptr"].shape[0] - 1
    kind = sp.csr_matrix if fmt == "csr" else sp.csc_matrix
    return kind((z[key + "/data"].copy(), z[key + "/indices"].copy(), z[key + "/indptr"].copy()), shape=(n, n))


def _np_params(tag):
    """a parameter set of the family without pivoting (default_configuration(1)-based, ml_cases.PARAMS)"""
    import ilupp_amd as ilupp
    _, thr, pre, knobs = PARAMS[tag]
    return C.engine_params(ilupp, thr, pre, knobs)


def _default_params(thr, config=None):
    """default-constructed parameters (PQ ordering + the factorisation with pivoting); config 10: maximum weighted matching in front"""
    import ilupp_amd as ilupp
    p = ilupp.iluplusplus_precond_parameter()
    if config is not None:
        p.default_configuration(config)
    p.threshold = thr
    return p


def _edge(n, seed):
    """a tridiagonal matrix with a weak diagonal plus ml_cases.weak_random: small pivots end levels, so that levels exist"""
    T = sp.diags([np.full(n - 1, -1.0), np.full(n, 0.5), np.full(n - 1, -1.0)], [-1, 0, 1], format="csr")
    A = (T + C.weak_random(n, 0.03, 0.0, seed)).tocsr()
    A.sort_indices()
    return A


def _tridiag(n):
    """diagonally dominant, rows of 2 - 3 entries: its multilevel object builds in milliseconds whatever n is"""
    A = sp.diags([np.full(n - 1, -1.0), np.full(n, 4.0), np.full(n - 1, -1.5)], [-1, 0, 1], format="csr")
    A.sort_indices()
    return A


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want):
    """bit for bit; a NaN equals a NaN whatever its payload"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(_bits(got)[ok], _bits(want)[ok])


def _rhs(n, k=0):
    return C.rhs(n) * (1.0 + k / 16.0)


@pytest.fixture(scope="module")
def members():
    """[(tag, P, levels)]: members of both families, built one by one and by ILUppPreconditioner.batch; with the single applies P @ b and
    P.T @ b of every member computed once: [(b, P @ b, P.T @ b)]"""
    import ilupp_amd as ilupp
    out = []
    for name, tag in SINGLE:
        out.append(("%s/%s" % (name, tag), ilupp.ILUppPreconditioner(_gold_matrix(name), params=_np_params(tag))))
    mats = [_gold_matrix(name) for name in BATCHED]
    for name, P in zip(BATCHED, ilupp.ILUppPreconditioner.batch(mats, params=_np_params("t0.1"))):
        out.append(("batch:%s/t0.1" % name, P))
    for name, P in zip(BATCHED, ilupp.ILUppPreconditioner.batch(mats, params=_default_params(0.01))):
        out.append(("batch:%s/default 0.01" % name, P))
    out.append(("offdiag_150/default 0.01", ilupp.ILUppPreconditioner(_gold_matrix("offdiag_150"), threshold=0.01)))
    out.append(("offdiag_150/config 10", ilupp.ILUppPreconditioner(_gold_matrix("offdiag_150"), params=_default_params(0.01, 10))))
    out.append(("weak_200/smallpiv", ilupp.ILUppPreconditioner(_gold_matrix("weak_200"), params=_pivot_params("p_t0.05_smallpiv"))))
    out.append(("laplace2d_400 csc/default 1", ilupp.ILUppPreconditioner(_gold_matrix("laplace2d_400", "csc"))))
    ms = [(tag, P, P.pr.levels()) for tag, P in out]
    singles = []
    for k, (tag, P, _) in enumerate(ms):
        b = _rhs(P.shape[0], k)
        singles.append((b, P @ b, P.T @ b))
    return ms, singles


def _pivot_params(tag):
    """a parameter set of ml_cases.PIVOT_PARAMS (the factorisation with pivoting), as tests/test_gpu_mlp.py builds it"""
    import ilupp_amd as ilupp
    _, thr, pre, knobs = {p[0]: p for p in C.PIVOT_PARAMS}[tag]
    return C.engine_params(ilupp, thr, pre, knobs)


# ---- 1. level counts, both families, real permutations and scalings ----
@pytest.mark.parametrize("transpose", [False, True])
def test_members_of_every_level_count_in_one_batch(members, transpose):
    """members with exactly one level, with two, with three and more (and one whose last level is a single row) in ONE batch, of both
    families, singly built and batch-built, CSR- and CSC-built, with matchings and scalings that are not the identity: ml_apply_batch
    equals P @ b / P.T @ b of every member bit for bit, the inputs are not modified, and every member takes the launch"""
    import ilupp_amd as ilupp
    from ilupp_amd import _native
    ms, singles = members
    levels = [lv for _, _, lv in ms]
    print("levels:", {tag: lv for tag, _, lv in ms})
    assert 1 in levels and 2 in levels and max(levels) >= 3, levels
    assert any(P.pr.level_sizes(lv - 1)[0] == 1 and lv > 1 for _, P, lv in ms), "a member whose last level has a single row"
    B, rhs = [P for _, P, _ in ms], [b for b, _, _ in singles]
    keep = [b.copy() for b in rhs]
    Y = ilupp.ml_apply_batch(B, rhs, transpose=transpose)
    assert len(Y) == len(B)
    for k, ((tag, P, lv), (b, y, yt)) in enumerate(zip(ms, singles)):
        assert np.array_equal(_bits(b), _bits(keep[k])) and Y[k] is not b, tag
        assert _same(Y[k], yt if transpose else y), (tag, lv, transpose, float(np.nanmax(np.abs(Y[k] - (yt if transpose else y)))))
    assert _native.ml_apply_batch([P.pr for P in B], [b.copy() for b in rhs], transpose) == [0] * len(B)


# ---- 2. edges ----
def test_edge_sizes_and_tiny_batches(members):
    """n = 1 and n = 2; n = 255, 256 and 257 (the workgroup's row stride) with several levels, in both families; an empty batch; a batch
    of one; a wrong length refused by the library with nothing touched; a member named twice refused"""
    import ilupp_amd as ilupp
    from ilupp_amd import _native
    one, two = sp.csr_matrix(np.array([[2.0]])), sp.csr_matrix(np.array([[2.0, 1.0], [0.5, 3.0]]))
    B = [ilupp.ILUppPreconditioner(one, params=_np_params("t0.1")), ilupp.ILUppPreconditioner(two, params=_np_params("t0.1")),
         ilupp.ILUppPreconditioner(one.copy()), ilupp.ILUppPreconditioner(two.tocsc())]
    edges = [_edge(n, 40 + n) for n in (255, 256, 257)]
    B += [ilupp.ILUppPreconditioner(A, params=_np_params("t0.1")) for A in edges]
    B += ilupp.ILUppPreconditioner.batch(edges, params=_default_params(1.0))
    lv = [P.pr.levels() for P in B]
    print("levels of the edge members:", lv)
    assert all(v >= 2 for v in lv[4:]), lv
    rhs = [_rhs(P.shape[0], k) for k, P in enumerate(B)]
    for transpose in (False, True):
        Y = ilupp.ml_apply_batch(B, rhs, transpose=transpose)
        for k, (P, b) in enumerate(zip(B, rhs)):
            assert _same(Y[k], (P.T if transpose else P) @ b), (k, P.shape, transpose)
        # a batch of one
        for k in (0, 1, 5):
            assert _same(ilupp.ml_apply_batch([B[k]], [rhs[k]], transpose=transpose)[0], Y[k]), (k, transpose)
        assert _native.ml_apply_batch([B[5].pr], [rhs[5].copy()], transpose) == [0]
    assert ilupp.ml_apply_batch([], []) == [] and _native.ml_apply_batch([], [], True) == []
    assert _native.ml_apply_batch_max_n() >= 4097
    # a wrong length: refused with the reference's text, nothing touched; a member named twice
    lib = _native.lib()
    x = [rhs[4].copy(), rhs[5].copy()]
    H = (ctypes.c_void_p * 2)(B[4].pr._h.value, B[5].pr._h.value)
    X = (ctypes.c_void_p * 2)(*[a.ctypes.data for a in x])
    N = (ctypes.c_int64 * 2)(255, 255)
    assert lib.ilupp_hip_ml_apply_batch(2, H, X, N, 0, None) == -2                            # ILUPP_ERR_WRONG_SIZE
    assert lib.ilupp_hip_last_error().decode() == "vector has wrong size for preconditioner!"
    assert np.array_equal(x[0], rhs[4]) and np.array_equal(x[1], rhs[5])
    H2 = (ctypes.c_void_p * 2)(B[4].pr._h.value, B[4].pr._h.value)
    assert lib.ilupp_hip_ml_apply_batch(2, H2, X, (ctypes.c_int64 * 2)(255, 255), 0, None) == -1
    assert lib.ilupp_hip_last_error().decode() == "a preconditioner appears twice in the batch"
    with pytest.raises(ValueError, match="vector of 254 elements for a preconditioner of dimension 255"):
        ilupp.ml_apply_batch(B[4:5], [np.ones(254)])


# ---- 3. the device entry ----
@pytest.mark.parametrize("transpose", [False, True])
def test_device_entry_with_gaps_between_the_slices(members, transpose):
    """one packed tensor, the same vector values at different offsets (members of one dimension get one right-hand side), gaps between
    the slices, filled on a side stream without a sync; ml_apply_batch_ on that stream with ILUppPreconditioners, a
    DevicePreconditioner("ILUpp") and MultilevelOperators as members; a consumer behind it: the results equal the single applies, the gaps
    keep their bits"""
    import torch
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    ms, _ = members
    pick = [k for k, (tag, _, _) in enumerate(ms) if "weak_300" in tag or "weak_120" in tag]
    assert len(pick) >= 5
    A = _gold_matrix("weak_300")
    dA = ild.DeviceCSR.from_scipy(A)
    D = ild.DevicePreconditioner("ILUpp", dA, params=_np_params("t0.1"))
    B = [ms[k][1] for k in pick]
    B = [ild.MultilevelOperator(P) if j % 2 else P for j, P in enumerate(B)] + [D, ild.MultilevelOperator(ild.DevicePreconditioner("ILUpp", dA, params=_default_params(0.01)))]
    ns = [ms[k][1].shape[0] for k in pick] + [300, 300]
    rhs = [C.rhs(n) for n in ns]                                             # (the same values for every member of a dimension)
    want = []
    for P, b in zip(B, rhs):
        t = torch.from_numpy(b.copy()).cuda()
        (P if hasattr(P, "apply_") else ild.MultilevelOperator(P)).apply_(t, transpose=transpose)
        want.append(t.cpu().numpy())
    host_P = [ms[k][1] for k in pick]
    for P, b, w in zip(host_P, rhs, want):
        assert _same(w, (P.T if transpose else P) @ b)                       # (apply_device is the host apply)
    gap, offsets, total = 5, [], 5
    for n in ns:
        offsets.append(total)
        total += n + gap
    host = np.full(total, PATTERN, dtype=np.int64)
    for o, b in zip(offsets, rhs):
        host[o:o + b.shape[0]] = b.view(np.int64)
    src = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = torch.empty(total, dtype=torch.int64, device="cuda")
        x.copy_(src, non_blocking=True)                                      # the producer: no sync behind it
        routes = ild.ml_apply_batch_(B, x.view(torch.float64), offsets, transpose=transpose)
        out = x.clone()                                                      # the consumer
    side.synchronize()
    got = out.cpu().numpy()
    assert routes == [0] * len(B)
    mask = np.ones(total, dtype=bool)
    for k, (o, n, w) in enumerate(zip(offsets, ns, want)):
        assert _same(got[o:o + n].view(np.float64), w), (k, o, n, transpose)
        mask[o:o + n] = False
    assert np.all(got[mask] == PATTERN)
    with pytest.raises(ValueError, match="does not lie inside x"):
        ild.ml_apply_batch_(B[:1], x.view(torch.float64), [total])
    with pytest.raises(TypeError):
        ild.ml_apply_batch_([object()], x.view(torch.float64), [0])
    # the entries that refuse the class still do
    with pytest.raises(TypeError):
        ild.apply_batch_([D], x.view(torch.float64), [offsets[-2]])
    with pytest.raises(TypeError):
        ilupp.apply_batch([host_P[0]], [rhs[0]])


# ---- 4. routes ----
def test_members_past_the_cap_and_a_lone_large_member(members, monkeypatch):
    """one member of n = ml_apply_batch_max_n() + 1 in a batch with small ones: route 1 for it, 0 for the rest, all with the single
    applies' bits; a lone member of n = 4 097: route 1; two of them: the launch.  And ILUPP_BATCH_APPLY_MAX_N lowers the cap."""
    import ilupp_amd as ilupp
    from ilupp_amd import _native
    monkeypatch.delenv("ILUPP_BATCH_APPLY_MAX_N", raising=False)
    cap = _native.ml_apply_batch_max_n()
    print("ml_apply_batch_max_n:", cap)
    assert 4097 <= cap <= 1 << 16, cap
    ms, singles = members
    p = _np_params("t0.1")
    big = ilupp.ILUppPreconditioner(_tridiag(cap + 1), params=p)
    at_cap = ilupp.ILUppPreconditioner(_tridiag(cap), params=p)
    B = [ms[4][1], big, ms[5][1], at_cap]
    rhs = [singles[4][0], _rhs(cap + 1, 3), singles[5][0], _rhs(cap, 5)]
    for transpose in (False, True):
        assert _native.ml_apply_batch([P.pr for P in B], [b.copy() for b in rhs], transpose) == [0, 1, 0, 0]
        Y = ilupp.ml_apply_batch(B, rhs, transpose=transpose)
        for k, (P, b) in enumerate(zip(B, rhs)):
            assert _same(Y[k], (P.T if transpose else P) @ b), (k, transpose)
    lone = [ilupp.ILUppPreconditioner(_tridiag(4097), params=p), ilupp.ILUppPreconditioner(_tridiag(4096), params=p),
            ilupp.ILUppPreconditioner(_tridiag(4097), params=_np_params("t0.05_mwm"))]
    lr = [_rhs(P.shape[0], k) for k, P in enumerate(lone)]
    assert _native.ml_apply_batch([lone[0].pr], [lr[0].copy()], False) == [1]
    assert _native.ml_apply_batch([lone[1].pr], [lr[1].copy()], False) == [0]
    assert _native.ml_apply_batch([P.pr for P in lone], [b.copy() for b in lr], True) == [0, 0, 0]
    for transpose in (False, True):
        for sub in ([0], [1], [0, 1, 2]):
            Y = ilupp.ml_apply_batch([lone[k] for k in sub], [lr[k] for k in sub], transpose=transpose)
            for y, k in zip(Y, sub):
                assert _same(y, (lone[k].T if transpose else lone[k]) @ lr[k]), (sub, k, transpose)
    monkeypatch.setenv("ILUPP_BATCH_APPLY_MAX_N", "128")
    assert _native.ml_apply_batch_max_n() == 128
    small = [ms[1][1], ms[4][1], ms[3][1]]                                     # n = 120, 120, 300
    sr = [singles[1][0], singles[4][0], singles[3][0]]
    assert _native.ml_apply_batch([P.pr for P in small], [b.copy() for b in sr], False) == [0, 0, 1]
    for y, k in zip(ilupp.ml_apply_batch(small, sr), (1, 4, 3)):
        assert _same(y, singles[k][1]), k


# ---- 5. call sequences ----
def test_call_sequences(members):
    """the single apply, then the batch, then the single apply on the same objects; the batch twice (the second call finds its tables on
    the device); a member destroyed right behind a launch that was not waited for, the other members' results still correct"""
    import torch
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    ms, singles = members
    idx = [4, 5, 3, 12, 13]
    B, rhs = [ms[k][1] for k in idx], [singles[k][0] for k in idx]
    for transpose in (False, True):
        want = [singles[k][2 if transpose else 1] for k in idx]
        for P, b, w in zip(B, rhs, want):
            assert _same((P.T if transpose else P) @ b, w)
        for rep in range(2):
            for y, w in zip(ilupp.ml_apply_batch(B, rhs, transpose=transpose), want):
                assert _same(y, w), (transpose, rep)
        for P, b, w in zip(B, rhs, want):
            assert _same((P.T if transpose else P) @ b, w)
    # device entry, not waited for: a single apply of a member right behind it, then the batch again
    ns = [P.shape[0] for P in B]
    offsets = list(np.cumsum([0] + ns[:-1]))
    packed = np.concatenate(rhs)
    x = torch.from_numpy(packed.copy()).cuda()
    ild.ml_apply_batch_(B, x, offsets)
    t = torch.from_numpy(rhs[1].copy()).cuda()
    ild.MultilevelOperator(B[1]).apply_(t)
    x2 = torch.from_numpy(packed.copy()).cuda()
    ild.ml_apply_batch_(B, x2, offsets)
    torch.cuda.synchronize()
    assert _same(t.cpu().numpy(), singles[idx[1]][1])
    for got in (x.cpu().numpy(), x2.cpu().numpy()):
        for k, (o, n) in enumerate(zip(offsets, ns)):
            assert _same(got[o:o + n], singles[idx[k]][1]), k
    # a member of its own, destroyed right behind the launch
    A = _gold_matrix("weak_120")
    doomed = ilupp.ILUppPreconditioner(A, params=_np_params("t0.1"))
    b0 = _rhs(120, 9)
    w0 = doomed @ b0
    x3 = torch.from_numpy(np.concatenate([b0, packed])).cuda()
    ild.ml_apply_batch_([doomed] + B, x3, [0] + [120 + o for o in offsets])
    del doomed
    gc.collect()
    fresh = ilupp.ILUppPreconditioner(A, params=_np_params("t0.1"))          # (takes the pooled blocks the destruction gave back)
    assert _same(fresh @ b0, w0)
    got = x3.cpu().numpy()
    assert _same(got[:120], w0)
    for k, (o, n) in enumerate(zip(offsets, ns)):
        assert _same(got[120 + o:120 + o + n], singles[idx[k]][1]), k


# ---- 6. the solve ----
def _solve_case(ms, picks, extra):
    """(As, Ms, b, offsets): multilevel members ms[k] for k in picks, each on its own matrix, then the members of `extra`"""
    import torch
    import ilupp_amd.device as ild
    As, Ms, rhs = [], [], []
    for k in picks:
        tag, P, _ = ms[k]
        name = tag.split("/")[0].replace("batch:", "").replace(" csc", "")
        As.append(ild.DeviceCSR.from_scipy(_gold_matrix(name)))
        Ms.append(ild.MultilevelOperator(P))
    for A, M in extra:
        As.append(A)
        Ms.append(M)
    rhs = [np.random.default_rng(500 + k).standard_normal(A.n) + 2.0 for k, A in enumerate(As)]
    gap, offsets, total = 3, [], 3
    for v in rhs:
        offsets.append(total)
        total += v.shape[0] + gap
    host = np.zeros(total)
    for o, v in zip(offsets, rhs):
        host[o:o + v.shape[0]] = v
    return As, Ms, torch.from_numpy(host).cuda(), offsets


def _solves_equal_the_loop(As, Ms, b, offsets, **kw):
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    st = {}
    x = ild.bicgstab_batch(As, b, offsets, Ms, stats=st, **kw)
    xh = x.cpu().numpy()
    for k, (A, M, o) in enumerate(zip(As, Ms, offsets)):
        single = M if M is None or hasattr(M, "apply_") else (
            ild.PivotedOperator(M) if isinstance(getattr(M, "pr", M), _native.PivotedPreconditioner) else ild.FactorOperator(M))
        s1 = {}
        xr = ild.bicgstab(A, b[o:o + A.n][:, None], single, stats=s1, **kw)[:, 0].cpu().numpy()
        print("member %d (n %d): iterations %d, converged %s, relres %.3e, max |x| %.3e" % (
            k, A.n, int(s1["iterations"][0]), bool(s1["converged"][0]), float(s1["relres"][0]), float(np.nanmax(np.abs(xr)))))
        assert _same(xh[o:o + A.n], xr), (k, "x", kw)
        assert int(st["iterations"][k]) == int(s1["iterations"][0]), (k, "iterations", kw)
        assert bool(st["converged"][k]) == bool(s1["converged"][0]), (k, "converged", kw)
        assert _same(st["relres"][k:k + 1].numpy(), s1["relres"].numpy()), (k, "relres", kw)
    mask = np.ones(xh.shape[0], dtype=bool)
    for A, o in zip(As, offsets):
        mask[o:o + A.n] = False
    assert np.all(xh[mask] == 0.0)
    return st


@pytest.mark.parametrize("check_every", [1, 0])
def test_solve_with_multilevel_members_alone(members, check_every):
    """five systems of n <= 400 whose members are MultilevelOperators (one to six levels, both families): every member's solution and
    stats equal device.bicgstab(A_k, b_k[:, None], MultilevelOperator(P_k)) bit for bit, and every member takes the launch"""
    ms, _ = members
    picks = [0, 3, 4, 5, 12]
    assert sorted(set(ms[k][2] for k in picks))[:2] == [1, 2] and max(ms[k][2] for k in picks) >= 3
    As, Ms, b, offsets = _solve_case(ms, picks, [])
    st = _solves_equal_the_loop(As, Ms, b, offsets, maxiter=8, rtol=1e-10 if check_every else 0.0, check_every=check_every)
    assert st["route"] == [0] * len(As)


@pytest.mark.parametrize("check_every", [1, 0])
def test_solve_with_a_mixed_batch(members, check_every):
    """three multilevel members mixed with one ILU0, one ILUCP and one member without a preconditioner, in one launch of the second
    instantiation: every member equals its single solve bit for bit"""
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    ms, _ = members
    A1, A2, A3 = _gold_matrix("rdd_300"), _gold_matrix("p3d_6_7_5"), _gold_matrix("laplace2d_400")
    d1, d2, d3 = [ild.DeviceCSR.from_scipy(A) for A in (A1, A2, A3)]
    extra = [(d1, ild.DevicePreconditioner("ILU0", d1)), (d2, ilupp.ILUCPPreconditioner(A2)), (d3, None)]
    As, Ms, b, offsets = _solve_case(ms, [4, 13, 3], extra)
    order = [3, 0, 4, 1, 5, 2]                                                # (the kinds interleaved)
    As, Ms, offsets = [As[k] for k in order], [Ms[k] for k in order], [offsets[k] for k in order]
    st = _solves_equal_the_loop(As, Ms, b, offsets, maxiter=8, rtol=1e-10 if check_every else 0.0, check_every=check_every)
    assert st["route"] == [0] * len(As)


def test_solve_without_a_multilevel_member_and_past_the_cap(members, monkeypatch):
    """a batch with no multilevel member (ILU0, ILUCP, none) equals the loop of single solves as it always did; with the cap lowered to
    128 a multilevel member of n = 300 takes route 1 and is solved by the single solve inside the call, the one of n = 120 stays in the
    launch; the bare multilevel objects keep their TypeError; the library's entry refuses a handle that is no multilevel object"""
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    ms, _ = members
    A1, A2, A3 = _gold_matrix("rdd_300"), _gold_matrix("p3d_6_7_5"), _gold_matrix("weak_120")
    d1, d2, d3 = [ild.DeviceCSR.from_scipy(A) for A in (A1, A2, A3)]
    extra = [(d1, ild.DevicePreconditioner("ILU0", d1)), (d2, ilupp.ILUCPPreconditioner(A2)), (d3, None)]
    As, Ms, b, offsets = _solve_case(ms, [], extra)
    for ce in (1, 0):
        st = _solves_equal_the_loop(As, Ms, b, offsets, maxiter=8, rtol=1e-10 if ce else 0.0, check_every=ce)
        assert st["route"] == [0, 0, 0]
    assert _native.bicgstab_batch_ml_max_n() >= 4096 and _native.bicgstab_batch_max_n() >= 4096
    for bad in (ms[4][1], ild.DevicePreconditioner("ILUpp", d3, params=_np_params("t0.1"))):
        with pytest.raises(TypeError):
            ild.bicgstab_batch([d3], b, [offsets[2]], [bad])
    monkeypatch.setenv("ILUPP_BATCH_APPLY_MAX_N", "128")
    assert _native.bicgstab_batch_ml_max_n() == 128
    As, Ms, b, offsets = _solve_case(ms, [4, 5], extra[2:])                   # n = 120 (launch), 300 (route 1), 120 without a preconditioner
    st = _solves_equal_the_loop(As, Ms, b, offsets, maxiter=8, rtol=1e-10, check_every=1)
    assert st["route"] == [0, 1, 0]
    # no multilevel member is left for the launch: the other member gets the launch it always had
    As, Ms, b, offsets = _solve_case(ms, [5], extra[2:])
    st = _solves_equal_the_loop(As, Ms, b, offsets, maxiter=8, rtol=1e-10, check_every=1)
    assert st["route"] == [1, 0]
