"""GPU tests of the batched BiCGstab solve with members of every class in one launch (ilupp_amd.device.bicgstab_batch over
ilupp_hip_bicgstab_batch_device: k_bicgstab_batch, one workgroup per system with the whole left-preconditioned loop inside it, the
member an ILUCP / ILUTP object, an ILU0 / ILUT / ILUC / IChol0 / ICholT object or none).  Parity is bitwise throughout, against what
exists without the batch, one member at a time: ilupp_amd.device.bicgstab(A_k, b_k[:, None], M_k, ...) -- the solution on its int64
view, the iteration count, the converged flag and the bits of the relative residual."""
import ctypes
import time

import numpy as np
import pytest
import scipy.sparse as sp

import matgen

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 65, 256, 257, 300, 512, 513]     # one row; a wave and one; one chunk of the dot, 2 chunks of 129, of 150, of 256, 3 chunks of 171
PATTERN = np.int64(0x7FF4DEADBEEF0123)          # (a signalling NaN's bits: arithmetic on it would not give it back)


def _csr(t):
    d, i, p = t
    n = p.shape[0] - 1
    A = sp.csr_matrix((np.asarray(d, dtype=np.float64), i, p), shape=(n, n))
    A.sort_indices()
    return A


def _dd(n, seed):
    """matgen.random_dd as it comes: nonsymmetric, diagonally dominant"""
    return _csr(matgen.random_dd(n, 8, 25.0, seed))


def _sym(n, seed):
    A = sp.csr_matrix(matgen.symmetrize(*matgen.random_dd(n, 8, 25.0, seed)), shape=(n, n))
    A.sort_indices()
    return A


def _band(n, seed):
    """rows of 2 - 3 entries: a random tridiagonal matrix with a heavy diagonal"""
    rng = np.random.default_rng(seed)
    A = sp.diags([rng.standard_normal(n - 1), 4.0 + rng.random(n), rng.standard_normal(n - 1)], [-1, 0, 1], format="csr")
    A.sort_indices()
    return A


def _scaled(A, seed):
    """the same pattern, every value scaled by 1 + 0.1 u"""
    B = A.copy()
    B.data = A.data * (1.0 + 0.1 * np.random.default_rng(seed).random(A.data.shape[0]))
    return B


def _rhs(n, seed=0):
    return np.random.default_rng(1000 + seed).standard_normal(n) + 2.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _pack(vectors, gap=3, fill=0.0):
    """the vectors in one array with `gap` elements in front of, between and behind them: (array, offsets)"""
    offsets, total = [], gap
    for v in vectors:
        offsets.append(total)
        total += v.shape[0] + gap
    host = np.full(total, fill, dtype=np.float64)
    for o, v in zip(offsets, vectors):
        host[o:o + v.shape[0]] = v
    return host, offsets


def _gaps(host_len, offsets, ns):
    mask = np.ones(host_len, dtype=bool)
    for o, n in zip(offsets, ns):
        mask[o:o + n] = False
    return mask


def _member(kind, A, dA, how, **params):
    """one member three ways: 0 = a DevicePreconditioner, 1 = the host class of the ctypes binding itself, 2 = a FactorOperator of it"""
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    if how == 0:
        return ild.DevicePreconditioner(kind, dA, **params)
    defaults = {"ILUT": dict(fill_in=100, threshold=0.1), "ILUC": dict(fill_in=100, threshold=0.1), "ICholT": dict(add_fill_in=0, threshold=0.0)}
    kw = dict(defaults.get(kind, {}))
    kw.update(params)
    P = getattr(ilupp, kind + "Preconditioner")(A, **kw)
    return P if how == 1 else ild.FactorOperator(P)


def _single(M):
    """what solves with a member alone"""
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    if M is None or hasattr(M, "apply_"):
        return M
    return ild.PivotedOperator(M) if isinstance(getattr(M, "pr", M), _native.PivotedPreconditioner) else ild.FactorOperator(M)


def _device(mats):
    import ilupp_amd.device as ild
    return [ild.DeviceCSR.from_scipy(A) for A in mats]


def _loop(As, Ms, b, offsets, x0=None, **kw):
    """the reference: one member at a time through device.bicgstab; per member (x, iterations, converged, relres)"""
    import ilupp_amd.device as ild
    out = []
    for A, M, o in zip(As, Ms, offsets):
        st = {}
        x = ild.bicgstab(A, b[o:o + A.n][:, None], _single(M), x0=None if x0 is None else x0[o:o + A.n][:, None], stats=st, **kw)
        out.append((x[:, 0].cpu().numpy(), int(st["iterations"][0]), bool(st["converged"][0]), st["relres"].numpy().copy()))
    return out


def _batch_equals(As, Ms, b, offsets, ref, x0=None, nan_members=(), tag="", **kw):
    """bicgstab_batch against `ref` (what _loop gave): the solutions on their int64 views (equal_nan for the members of nan_members, whose
    NaNs need not share a payload), iterations, converged and the bits of relres.  Returns (x on the host, stats)."""
    import ilupp_amd.device as ild
    st = {}
    x = ild.bicgstab_batch(As, b, offsets, Ms, x0=x0, stats=st, **kw)
    assert x.shape == b.shape and x.data_ptr() != b.data_ptr()
    xh = x.cpu().numpy()
    assert len(st["route"]) == len(As) and st["iterations"].dtype.is_floating_point is False and st["iterations"].shape == (len(As),)
    for k, (A, o, (xr, it, conv, rel)) in enumerate(zip(As, offsets, ref)):
        got = xh[o:o + A.n]
        if k in nan_members:
            assert np.array_equal(got, xr, equal_nan=True), (tag, k, "x")
            assert np.array_equal(st["relres"][k:k + 1].numpy(), rel, equal_nan=True), (tag, k, "relres")
        else:
            assert np.array_equal(_bits(got), _bits(xr)), (tag, k, "x", float(np.max(np.abs(got - xr))))
            assert np.array_equal(_bits(st["relres"][k:k + 1].numpy()), _bits(rel)), (tag, k, "relres", float(st["relres"][k]), rel)
        assert int(st["iterations"][k]) == it, (tag, k, "iterations", int(st["iterations"][k]), it)
        assert bool(st["converged"][k]) == conv, (tag, k, "converged")
    return xh, st


# ---- 1. every shape, every non-pivoting kind and none, in one batch ----
SOLVE_KINDS = ["ILU0", "ILUT", "ILUC", None, "IChol0"]          # (IChol0 on the symmetrised matrix)
TRIES = 64


def _tiny_rhs(dA, M, base, **kw):
    """The right-hand side of a member of n <= 2 for a run with checks on.  BiCGstab solves such a system in the first half step, and
    where that leaves s (or, an iteration on, r) exactly zero the loop divides 0 by 0 and stops as broken down instead of converged:
    which of the two happens is a matter of the last bit of b.  So: the first of a seeded sequence of 64 candidates for which the
    single solve -- the reference alone, all candidates as the columns of one block, each column having the bits of its solve alone
    -- converges; where none does (a preconditioner that is exact for such a matrix leaves s = r - 1 * r = 0 almost always) the first
    candidate, and the member's breakdown is what the batch is compared with.  Returns (the vector, whether it converges)."""
    import torch
    import ilupp_amd.device as ild
    V = np.stack([_rhs(dA.n, base + 1000 * seed) for seed in range(TRIES)], axis=1)
    st = {}
    ild.bicgstab(dA, torch.from_numpy(np.ascontiguousarray(V)).cuda(), _single(M), stats=st, **kw)
    good = np.flatnonzero(st["converged"].numpy())
    pick = int(good[0]) if good.size else 0
    return V[:, pick].copy(), bool(good.size)


@pytest.fixture(scope="module")
def solve_members():
    """(As, Ms, right-hand sides on the host, b on the device, offsets): the members of n <= 2 with a plain seeded one, which the runs with checks on replace"""
    import torch
    d, i, p = matgen.poisson3d(8)
    mats = [(_dd(n, 60 + k), _sym(n, 60 + k)) for k, n in enumerate(SIZES)] + [(_csr((d, i, p)), _csr((d, i, p)))]
    As, Ms, rhs = [], [], []
    for k, (A, S) in enumerate(mats):
        dA, dS = _device([A, S])
        for j, kind in enumerate(SOLVE_KINDS):
            mat, dmat = (S, dS) if kind == "IChol0" else (A, dA)
            As.append(dmat)
            Ms.append(None if kind is None else _member(kind, mat, dmat, (k + j) % 3))
            n = A.shape[0]
            rhs.append(_rhs(n, 7 * k + j) if n <= 2 else _rhs(n, 7 * k + j) * (1.0 + j / 4.0))
    host, offsets = _pack(rhs)
    return As, Ms, rhs, torch.from_numpy(host).cuda(), offsets


@pytest.mark.parametrize("check_every", [0, 1, 3])
def test_solves_equal_the_loop(solve_members, check_every):
    """ILU0, ILUT, ILUC, no preconditioner and IChol0 (on the symmetrised matrix) on every matrix (random_dd of n = 1, 2, 65, 256, 257,
    300, 512, 513 as it comes, nonsymmetric, and poisson3d(8)), DevicePreconditioners, host classes and FactorOperators in turn, in ONE
    batch.  check_every = 0: at most 6 iterations each, nobody converges (the members of n <= 2 are exact after one step and break down
    or run on, as the last bit has it).  check_every = 1 and 3 with rtol = 1e-10, at most 40 iterations: asserted on the LOOP's stats
    before the comparison -- every member of n > 2 converges, and not all at the same iteration -- so the comparison is of members
    that stop alone.  The members of n <= 2 get their right-hand sides from _tiny_rhs for these runs: those for which a candidate
    converges are compared as converged members, the others (printed) as members that break down."""
    import torch
    As, Ms, rhs, b, offsets = solve_members
    kw = dict(maxiter=6, check_every=0) if check_every == 0 else dict(maxiter=40, rtol=1e-10, check_every=check_every)
    big = [k for k, A in enumerate(As) if A.n > 2]
    tiny = [k for k, A in enumerate(As) if A.n <= 2]
    assert len(tiny) == 10
    if check_every:
        rhs, found = list(rhs), []
        for k in tiny:
            rhs[k], ok = _tiny_rhs(As[k], Ms[k], k, **kw)
            found.append(ok)
        print("check_every %d: members of n <= 2 with a right-hand side that converges: %s" % (check_every, found))
        b = torch.from_numpy(_pack(rhs)[0]).cuda()
    ref = _loop(As, Ms, b, offsets, **kw)
    its = [it for _, it, _, _ in ref]
    print("check_every %d: iterations of the reference loop %s" % (check_every, its))
    if check_every:
        assert all(ref[k][2] for k in big), [k for k in big if not ref[k][2]]
        assert len(set(its[k] for k in big)) >= 2 and all(0 < its[k] < 40 for k in big), its
        assert all(float(ref[k][3][0]) <= 1e-10 for k in big)
        assert [ref[k][2] for k in tiny] == found                      # (a column of the block has the bits of its solve alone)
    else:
        assert max(its) == 6 and not any(conv for _, _, conv, _ in ref)
    xh, st = _batch_equals(As, Ms, b, offsets, ref, tag=("solve", check_every), **kw)
    assert st["route"] == [0] * len(As)
    assert np.all(_bits(xh[_gaps(xh.shape[0], offsets, [A.n for A in As])]) == 0)          # (the gaps: zeros, untouched)


# ---- 2. pivoting and non-pivoting members in one launch ----
def test_mixed_families_in_one_launch():
    """ILUCP and ILUTP members (n = 65, 300, 513; random_dd and tridiagonal matrices) interleaved with ILU0 members and members without a
    preconditioner: every member equals its single solve, and the pivoting members have, bit for bit, what a batch of them alone gives"""
    import torch
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    pmats = [_dd(65, 21), _band(300, 22), _dd(513, 23), _band(65, 24), _dd(300, 25), _band(513, 26)]
    Ps = [(ilupp.ILUCPPreconditioner if k % 2 == 0 else ilupp.ILUTPPreconditioner)(A) for k, A in enumerate(pmats)]
    Ps[1], Ps[4] = ild.PivotedOperator(Ps[1]), ild.PivotedOperator(Ps[4])
    omats = [_dd(129, 31), _dd(257, 32), _dd(64, 33), _dd(300, 34), _dd(513, 35), _dd(40, 36)]
    dP, dO = _device(pmats), _device(omats)
    Os = [ild.DevicePreconditioner("ILU0", dO[0]), None, _member("ILU0", omats[2], dO[2], 1), None, _member("ILU0", omats[4], dO[4], 2), None]
    As, Ms = [], []
    for k in range(6):
        As += [dP[k], dO[k]]
        Ms += [Ps[k], Os[k]]
    host, offsets = _pack([_rhs(A.n, k) for k, A in enumerate(As)])
    b = torch.from_numpy(host).cuda()
    for kw in (dict(maxiter=7, check_every=0), dict(maxiter=40, rtol=1e-10, check_every=2)):
        ref = _loop(As, Ms, b, offsets, **kw)
        xh, st = _batch_equals(As, Ms, b, offsets, ref, tag=("mixed", kw["maxiter"]), **kw)
        assert st["route"] == [0] * 12
        assert all(it > 0 for _, it, _, _ in ref)
        sto = {}
        old = ild.bicgstab_batch(As[0::2], b, offsets[0::2], Ms[0::2], stats=sto, **kw).cpu().numpy()      # the pivoting members in a batch of their own
        assert sto["route"] == [0] * 6
        for j, (A, o) in enumerate(zip(As[0::2], offsets[0::2])):
            assert np.array_equal(_bits(old[o:o + A.n]), _bits(xh[o:o + A.n])), j
            for key in ("iterations", "converged"):
                assert sto[key][j] == st[key][2 * j], (j, key)
            assert np.array_equal(_bits(sto["relres"][j:j + 1].numpy()), _bits(st["relres"][2 * j:2 * j + 1].numpy())), j


# ---- 3. x0 ----
def test_a_start_vector_and_an_exact_one(solve_members):
    """x0 given: used as the loop uses it, the gaps keep x0's bits (a signalling-NaN pattern); two members whose x0 is exact (b = A x0 by
    the library's own SpMV, so r is zero to the bit) leave at once: converged, 0 iterations, x = x0"""
    import torch
    As, Ms, _, b, offsets = solve_members
    As, Ms, offsets = As[10:25], Ms[10:25], offsets[10:25]
    ns = [A.n for A in As]
    x0i = np.full(b.numel(), PATTERN, dtype=np.int64)
    rng = np.random.default_rng(5)
    for o, n in zip(offsets, ns):
        x0i[o:o + n] = rng.standard_normal(n).view(np.int64)
    x0 = torch.from_numpy(x0i).cuda().view(torch.float64)
    b = b.clone()
    exact = (3, 5)                                                       # (one without a preconditioner, one with ILU0)
    assert Ms[3] is None and Ms[5] is not None
    for k in exact:
        o, n = offsets[k], ns[k]
        b[o:o + n] = As[k].matmat(x0[o:o + n].clone()[:, None])[:, 0]
    for kw in (dict(maxiter=4, check_every=0), dict(maxiter=40, rtol=1e-10, check_every=2)):
        ref = _loop(As, Ms, b, offsets, x0=x0, **kw)
        xh, st = _batch_equals(As, Ms, b, offsets, ref, x0=x0, tag=("x0", kw["maxiter"]), **kw)
        assert np.all(_bits(xh)[_gaps(xh.shape[0], offsets, ns)] == PATTERN)                  # (the gaps keep x0's bits)
        for k in exact:
            o, n = offsets[k], ns[k]
            assert bool(st["converged"][k]) and int(st["iterations"][k]) == 0 and float(st["relres"][k]) == 0.0
            assert np.array_equal(_bits(xh[o:o + n]), x0i[o:o + n])
        assert any(int(st["iterations"][k]) > 0 for k in range(len(As)) if k not in exact)


# ---- 4. isolation and breakdown ----
def test_zero_nan_and_breakdown_members_leave_the_others_alone():
    """member 0: an all-zero right-hand side -- converged at once, 0 iterations, x = x0's slice; member 1: NaN and +-Inf in the right-hand
    side -- not converged, what the loop gives; member 2: A = 2 I without a preconditioner and b = ones, the first half step is exact
    (alpha = 1/2, s = 0 to the bit), so omega = 0 / 0 -- and member 3: blocks [[0, 1], [1, 0]], A p = p for p = ones, the same; member
    4: diag(+1, -1, ...) of even size, (Ap, r0*) = 0 -- all three stop in the first iteration as not converged with x = x0 = 0, which is
    asserted on the single solves first; members 5 - 7 keep the bits they have in a batch without the others"""
    import torch
    import ilupp_amd.device as ild
    n_b = 66
    two_i = sp.identity(n_b, format="csr") * 2.0
    swap = sp.kron(sp.identity(n_b // 2), sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])), format="csr")
    swap.sort_indices()
    ind = sp.diags(np.where(np.arange(n_b) % 2 == 0, 1.0, -1.0), format="csr")
    mats = [_dd(200, 700), _dd(200, 701), sp.csr_matrix(two_i), swap, ind, _dd(129, 702), _dd(300, 703), _dd(257, 704)]
    As = _device(mats)
    Ms = [ild.DevicePreconditioner("ILU0", As[0]), ild.DevicePreconditioner("ILU0", As[1]), None, None, None,
          ild.DevicePreconditioner("ILUT", As[5]), None, ild.DevicePreconditioner("ILU0", As[7])]
    rhs = [_rhs(A.shape[0], k) for k, A in enumerate(mats)]
    rhs[0] = np.zeros(200)
    rhs[1][3], rhs[1][77], rhs[1][150] = np.nan, np.inf, -np.inf
    for k in (2, 3, 4):
        rhs[k] = np.ones(n_b)
    host, offsets = _pack(rhs)
    b = torch.from_numpy(host).cuda()
    x0h = np.random.default_rng(6).standard_normal(b.numel())
    for k in (2, 3, 4):
        x0h[offsets[k]:offsets[k] + n_b] = 0.0
    x0 = torch.from_numpy(x0h).cuda()
    kw = dict(maxiter=6, rtol=1e-12, check_every=2)
    ref = _loop(As, Ms, b, offsets, x0=x0, **kw)
    for k in (2, 3, 4):                                                  # the single solves break down: no iteration counted, r as at the start
        assert ref[k][1] == 0 and not ref[k][2] and float(ref[k][3][0]) == 1.0 and np.all(ref[k][0] == 0.0), (k, ref[k][1:])
    xh, st = _batch_equals(As, Ms, b, offsets, ref, x0=x0, nan_members=(1,), tag="isolation", **kw)
    assert st["route"] == [0] * 8
    assert bool(st["converged"][0]) and int(st["iterations"][0]) == 0 and float(st["relres"][0]) == 0.0
    assert np.array_equal(_bits(xh[offsets[0]:offsets[0] + 200]), _bits(x0h[offsets[0]:offsets[0] + 200]))
    assert not bool(st["converged"][1]) and np.isnan(float(st["relres"][1]))
    assert all(int(st["iterations"][k]) > 0 for k in (5, 6, 7))
    # the clean members in a batch of their own
    _batch_equals(As[5:], Ms[5:], b, offsets[5:], ref[5:], x0=x0, tag="clean alone", **kw)


# ---- 5. more members than CUs ----
def test_more_members_than_compute_units():
    """300 members of n = 40 with distinct seeds, ILU0, none and ILUT in turn: one launch of 300 workgroups on 256 CUs"""
    import torch
    import ilupp_amd.device as ild
    mats = [_dd(40, 1000 + k) for k in range(300)]
    As = _device(mats)
    Ms = [None if k % 3 == 1 else ild.DevicePreconditioner("ILU0" if k % 3 == 0 else "ILUT", A) for k, A in enumerate(As)]
    host, offsets = _pack([_rhs(40, k) * (1.0 + k / 64.0) for k in range(300)], gap=1)
    b = torch.from_numpy(host).cuda()
    ref = _loop(As, Ms, b, offsets, maxiter=4)
    _, st = _batch_equals(As, Ms, b, offsets, ref, maxiter=4, tag="300")
    assert st["route"] == [0] * 300


# ---- 6. the cap and the routes ----
def test_both_lds_paths_and_a_member_past_the_cap(monkeypatch):
    """ILUPP_BATCH_APPLY_MAX_N = 600 (4 800 bytes for the sweeps): n = 300 keeps both arrays in LDS (16 n = 4 800), n = 513 takes the
    one-array path through tmp (16 n > 4 800 >= 8 n), n = 700 exceeds the cap and goes through the single solve inside the same call;
    and an ILU0 member of poisson3d(8), whose single apply runs static sweeps, is solved in the launch from its CSR triangles; every
    member equals its single solve"""
    import torch
    import ilupp_amd.device as ild
    monkeypatch.setenv("ILUPP_BATCH_APPLY_MAX_N", "600")
    assert ild._native.bicgstab_batch_max_n() == 600
    mats = [_dd(n, 400 + k) for k, n in enumerate([300, 513, 700, 513, 300])] + [_csr(matgen.poisson3d(8))]
    ns = [A.shape[0] for A in mats]
    As = _device(mats)
    Ms = [ild.DevicePreconditioner("ILU0", As[0]), ild.DevicePreconditioner("ILUT", As[1]), ild.DevicePreconditioner("ILU0", As[2]),
          ild.DevicePreconditioner("ILUC", As[3]), None, ild.DevicePreconditioner("ILU0", As[5])]
    path = Ms[5].pr.path()
    print("path of ILU0 on poisson3d(8): %s" % path)
    assert "static" in path, path
    host, offsets = _pack([_rhs(n, k) for k, n in enumerate(ns)])
    b = torch.from_numpy(host).cuda()
    for kw in (dict(maxiter=5), dict(maxiter=40, rtol=1e-10, check_every=1)):
        ref = _loop(As, Ms, b, offsets, **kw)
        _, st = _batch_equals(As, Ms, b, offsets, ref, tag=("cap", kw["maxiter"]), **kw)
        assert st["route"] == [0, 0, 1, 0, 0, 0]
    assert Ms[5].pr.path() == path


# ---- 7. the pipeline: re-factorise, solve, re-factorise, with no host wait between ----
def test_refactor_then_solve_without_a_host_wait():
    """8 ILU0 members (n = 65 ... 513; DevicePreconditioners, host objects and FactorOperators in turn) and two sets of new values on the
    same patterns: refactor_batch_(check=False) directly followed by bicgstab_batch (no stats: no host wait), twice over, each result
    equal to the single solve with a freshly constructed DevicePreconditioner("ILU0") of those values; then a refactor_batch_ straight
    after a bicgstab_batch -- it must see that launch finished before it rewrites the factors, and leaves those of a fresh construction"""
    import torch
    import ilupp_amd.device as ild
    ns = [65, 129, 200, 256, 257, 300, 400, 513]
    mats = [_dd(n, 540 + k) for k, n in enumerate(ns)]
    A1 = [_scaled(A, 70 + k) for k, A in enumerate(mats)]
    A2 = [_scaled(A, 80 + k) for k, A in enumerate(mats)]
    d0, d1, d2 = _device(mats), _device(A1), _device(A2)
    members = [_member("ILU0", A, dA, k % 3) for k, (A, dA) in enumerate(zip(mats, d0))]
    host, offsets = _pack([_rhs(n, 50 + k) for k, n in enumerate(ns)])
    b = torch.from_numpy(host).cuda()
    kw = dict(maxiter=6, rtol=0.0, check_every=0)
    fresh1, fresh2 = [ild.DevicePreconditioner("ILU0", dA) for dA in d1], [ild.DevicePreconditioner("ILU0", dA) for dA in d2]
    want1 = [r[0] for r in _loop(d1, fresh1, b, offsets, **kw)]
    want2 = [r[0] for r in _loop(d2, fresh2, b, offsets, **kw)]
    assert not any(np.array_equal(a, c) for a, c in zip(want1, want2))
    factors = lambda M: [(f[0], f[1], f[2]) for f in M.pr.factors_info()]
    f1 = [factors(M) for M in fresh1]
    torch.cuda.synchronize()
    r1, s1 = ild.refactor_batch_(members, d1, check=False)
    x1 = ild.bicgstab_batch(d1, b, offsets, members, **kw)
    r2, s2 = ild.refactor_batch_(members, d2, check=False)              # (behind the launch that reads the first set's factors)
    x2 = ild.bicgstab_batch(d2, b, offsets, members, **kw)
    r3, s3 = ild.refactor_batch_(members, d1, check=False)              # straight after a solve nobody waited for
    torch.cuda.synchronize()
    assert r1 == r2 == r3 == [0] * 8
    assert s1.cpu().tolist() == s2.cpu().tolist() == s3.cpu().tolist() == [0] * 8
    x1h, x2h = x1.cpu().numpy(), x2.cpu().numpy()
    for k, (o, n) in enumerate(zip(offsets, ns)):
        assert np.array_equal(_bits(x1h[o:o + n]), _bits(want1[k])), (k, "first values")
        assert np.array_equal(_bits(x2h[o:o + n]), _bits(want2[k])), (k, "second values")
        F = factors(members[k])
        assert len(F) == len(f1[k]) == 2, k
        for a, c in zip(F, f1[k]):
            assert np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2]) and np.array_equal(_bits(a[0]), _bits(c[0])), k


# ---- 8. stream ordering ----
def test_between_a_producer_and_a_consumer_on_a_side_stream():
    """b is filled on a side stream without a sync, bicgstab_batch runs on that stream, a consumer clone behind it: the results equal the
    default-stream call and the gaps keep x0's bits; a single apply_ of a member right behind the batched call gives what it gives
    alone; and an ILU(0) member re-factorised right behind the call, for other values, is not seen by the launch -- while the next
    single apply sees the new factor"""
    import torch
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    ns = [150, 65, 257, 40, 129]
    mats = [_dd(n, 500 + k) for k, n in enumerate(ns)]
    As = _device(mats)
    Ms = [ild.DevicePreconditioner("ILUT", As[0]), ild.DevicePreconditioner("ILU0", As[1]), ild.DevicePreconditioner("ILUC", As[2]), None,
          ilupp.ILUCPPreconditioner(mats[4])]
    A1b = _scaled(mats[1], 2)
    dA1b = ild.DeviceCSR.from_scipy(A1b)
    fresh = ild.DevicePreconditioner("ILU0", dA1b)
    v1 = torch.from_numpy(_rhs(ns[1], 11)).cuda()
    new_alone = fresh.apply_(v1.clone()).cpu().numpy()
    old_alone = Ms[1].apply_(v1.clone()).cpu().numpy()
    assert not np.array_equal(new_alone, old_alone)
    host, offsets = _pack([_rhs(n, k) for k, n in enumerate(ns)], gap=7)
    x0i = np.full(host.shape[0], PATTERN, dtype=np.int64)
    rng = np.random.default_rng(8)
    for o, n in zip(offsets, ns):
        x0i[o:o + n] = rng.standard_normal(n).view(np.int64)
    x0 = torch.from_numpy(x0i).cuda().view(torch.float64)
    kw = dict(maxiter=7, rtol=1e-13, check_every=3)
    st0 = {}
    want = ild.bicgstab_batch(As, torch.from_numpy(host).cuda(), offsets, Ms, x0=x0, stats=st0, **kw).cpu().numpy()
    assert st0["route"] == [0] * 5
    ref = _loop(As, Ms, torch.from_numpy(host).cuda(), offsets, x0=x0, **kw)
    for (xr, _, _, _), o, n in zip(ref, offsets, ns):
        assert np.array_equal(_bits(want[o:o + n]), _bits(xr))
    v = torch.from_numpy(_rhs(ns[2], 12)).cuda()
    alone = Ms[2].apply_(v.clone()).cpu().numpy()
    src = torch.from_numpy(host).pin_memory()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = torch.empty(host.shape[0], dtype=torch.float64, device="cuda")
        b.copy_(src, non_blocking=True)                      # the producer: no sync behind it
        x = ild.bicgstab_batch(As, b, offsets, Ms, x0=x0, **kw)
        out = x.clone()                                      # the consumer
        behind = Ms[2].apply_(v.clone())                     # a single apply of a member right behind the launch
        ild._on_current_stream()
        Ms[1].pr.refactor_device(dA1b.data.data_ptr(), dA1b.indices.data_ptr(), dA1b.indptr.data_ptr())      # (waits for the launch that reads the old factor)
        single = Ms[1].apply_(v1.clone())
    side.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.all(_bits(got)[_gaps(host.shape[0], offsets, ns)] == PATTERN)
    assert np.array_equal(_bits(behind.cpu().numpy()), _bits(alone))
    assert np.array_equal(_bits(single.cpu().numpy()), _bits(new_alone))
    ild._on_current_stream()


# ---- 9. the refusals that need built objects ----
def test_refusals_that_need_built_objects():
    import torch
    import ilupp_amd as ilupp
    import ilupp_amd.device as ild
    from ilupp_amd import _native
    mats = [_dd(64, 900), _dd(65, 901)]
    As = _device(mats)
    Ms = [ild.DevicePreconditioner("ILU0", A) for A in As]
    b = torch.ones(140, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="appears twice"):
        ild.bicgstab_batch([As[0], As[0]], b, [0, 70], [Ms[0], Ms[0]])
    P = ilupp.ILUCPPreconditioner(mats[0])
    with pytest.raises(RuntimeError, match="appears twice"):
        ild.bicgstab_batch([As[0], As[1], As[0]], b, [0, 70, 0], [P, None, ild.PivotedOperator(P)])
    st = {}
    x = ild.bicgstab_batch([], b, [], [], stats=st)
    assert x.shape == b.shape and x.data_ptr() != b.data_ptr() and float(x.abs().sum()) == 0.0 and st["route"] == []
    assert all(st[k].numel() == 0 for k in ("iterations", "converged", "relres"))
    # a slice outside b and a dimension that is not the member's, on device tensors
    with pytest.raises(ValueError, match="does not lie inside b"):
        ild.bicgstab_batch(As, b, [0, 76], [Ms[0], None])
    with pytest.raises(ValueError, match="member 1: the matrix has dimension 64, the preconditioner 65"):
        ild.bicgstab_batch([As[0], As[0]], b, [0, 70], [None, Ms[1]])
    # the C entry names a multilevel handle instead of reading it as a factor pair, and a dimension that is not the member's
    params = ilupp.iluplusplus_precond_parameter()
    params.default_configuration(1)
    ml = ild.DevicePreconditioner("ILUpp", As[0], params=params)
    with pytest.raises(TypeError, match="ILUCPPreconditioner / ILUTPPreconditioner"):
        ild.bicgstab_batch([As[0]], b, [0], [ml])
    lib, VP = _native.lib(), ctypes.c_void_p
    keep = b.clone()
    A = As[0]
    one = lambda v: (VP * 1)(v)
    rc = lib.ilupp_hip_bicgstab_batch_device(1, one(ml.pr._h), None, (ctypes.c_int64 * 1)(64), one(A.data.data_ptr()), one(A.indices.data_ptr()),
                                             one(A.indptr.data_ptr()), (ctypes.c_int64 * 1)(A.nnz), b.data_ptr(), None, b.data_ptr(),
                                             (ctypes.c_int64 * 1)(0), b.data_ptr(), 7 * 64, 3, 0.0, 0, b.data_ptr(), b.data_ptr(), b.data_ptr(),
                                             b.data_ptr(), 1, (ctypes.c_int32 * 1)())
    assert rc == -1 and lib.ilupp_hip_last_error().decode() == "a multilevel preconditioner cannot be a member of a batch"
    mat1 = [(As[1].data.data_ptr(), As[1].indices.data_ptr(), As[1].indptr.data_ptr(), As[1].nnz)]
    tail = (b.data_ptr(), 0, b.data_ptr(), [0], b.data_ptr(), 7 * 65, 3, 0.0, 0, b.data_ptr(), b.data_ptr(), b.data_ptr(), b.data_ptr())
    with pytest.raises(RuntimeError, match="wrong size"):
        _native.bicgstab_batch_device([Ms[0].pr], [65], mat1, *tail)
    with pytest.raises(RuntimeError, match="wrong size"):
        _native.bicgstab_batch_device([P.pr if hasattr(P, "pr") else P], [65], mat1, *tail)
    torch.cuda.synchronize()
    assert torch.equal(b, keep)


# ---- 10. side by side, in wall time ----
def test_sixteen_solves_side_by_side_beat_the_loop():
    """16 ILU0 members on nonsymmetric matrices, n = 4 000, 20 iterations each (rtol = 0: the work is fixed): one bicgstab_batch call
    against the loop of the 16 single device.bicgstab solves on the same objects, measured in this test; medians of five after a
    warm-up of each"""
    import torch
    import ilupp_amd.device as ild
    n = 4000
    mats = [_dd(n, 500 + k) for k in range(16)]
    As = _device(mats)
    Ms = [ild.DevicePreconditioner("ILU0", A) for A in As]
    host, offsets = _pack([_rhs(n, k) * (1.0 + k / 16.0) for k in range(16)], gap=0)
    b = torch.from_numpy(host).cuda()
    kw = dict(maxiter=20, rtol=0.0, check_every=0)

    def batched():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = ild.bicgstab_batch(As, b, offsets, Ms, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, x

    def looped():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X = [ild.bicgstab(A, b[o:o + n][:, None], M, **kw) for A, M, o in zip(As, Ms, offsets)]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, X

    ref = _loop(As, Ms, b, offsets, **kw)
    _, st = _batch_equals(As, Ms, b, offsets, ref, tag="side by side", **kw)
    assert st["route"] == [0] * 16 and all(it == 20 for _, it, _, _ in ref)
    batched(), looped()
    t_batch = float(np.median([batched()[0] for _ in range(5)]))
    t_loop = float(np.median([looped()[0] for _ in range(5)]))
    print("ilu0 n %d x 16, 20 iterations: t_batch %.5f s, t_loop %.5f s" % (n, t_batch, t_loop))
    assert t_batch < t_loop, (t_batch, t_loop)
