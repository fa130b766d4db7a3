"""The two one-wave chain kernels with pivoting (ilucp.hip: k_ilucp / k_ilucp_batch, ilutp.hip: k_ilutp / k_ilutp_batch, with the helpers of
dp_dev.h and select_largest / wave_sort_u64 of piluc_dev.h) on the cases of tests/pivot_cases.py: every case sits on one pass edge, tie
rule, selection branch or store limit of a chain, which tests/test_pivot_ref.py proves on the CPU from the model's records.  Here every
case, as CSR and as the CSC arrays of the transpose (the same arrays under the other label), is built alone and as a member of one batch
per parameter set, and compared bit for bit with the oracle: index and pointer arrays, values as uint64 (a NaN where the oracle has
one), the permutation, apply and apply_trans, total_nnz, zero_pivots.  The cases the reference refuses must raise its message, and the
ILUPP_DEBUG line must name the status and the row or step the model predicts."""
import functools
import re
import time

import numpy as np
import pytest

import ml_cases
from capture_util import Env as _Env, Stderr as _Stderr
import pivot_cases as C
import pivot_ref as R

pytestmark = pytest.mark.gpu

_RE = {"tp": re.compile(r"\[ilupp\] ilutp: n (\d+), stores of (\d+): status (-?\d+) at row (\d+)"),
       "cp": re.compile(r"\[ilupp\] ilucp: n (\d+), stores of (\d+): status (-?\d+) at step (\d+)")}
MESSAGES = {("tp", R.ERR_MEMORY): "ILUTP2: memory reserved was insufficient.",
            ("tp", R.ERR_ZERO_PIVOT): "matrix_sparse::ILUTP2: encountered zero pivot in row %d",
            ("cp", R.ERR_MEMORY): "ILUCP4: Insufficient memory reserved. Increase mem_factor"}
STATUS = {R.OK: 0, R.ERR_MEMORY: 3, R.ERR_ZERO_PIVOT: 1}
FORMATS = ("csr", "csc")


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_values(got, want, tag):
    """bit for bit; where the oracle has a NaN, a NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, tag
    nan = np.isnan(want)
    assert np.all(np.isnan(got[nan])) and np.array_equal(_u64(got[~nan]), _u64(want[~nan])), tag


def _create(kind, batch=False):
    from ilupp_amd import _native
    if batch:
        return _native.ILUTPPreconditioner_batch if kind == "tp" else _native.ILUCPPreconditioner_batch
    return _native.ILUTPPreconditioner if kind == "tp" else _native.ILUCPPreconditioner


def _args(p):
    return (p["fill_in"], p["threshold"], p["piv_tol"], p["rp"], p["mem_factor"])


def _measure(P, n):
    L, U, perm = P.raw()
    b = ml_cases.rhs(n)
    x = b.copy(); P.apply(x)
    xt = b.copy(); P.apply_trans(xt)
    return dict(L=L, U=U, perm=perm, x=x, xt=xt, total_nnz=P.total_nnz, zero_pivots=P.zero_pivots)


@functools.lru_cache(maxsize=None)
def _expected(name, fmt):
    """the oracle's object of one orientation with both applies, or its error code (computed once, left unchanged)"""
    from oracle import oracle as O
    c = C.CASES[name]
    ptr, idx, val = C.arrays(name)
    try:
        Q = (O.ILUTP if c.kind == "tp" else O.ILUCP)(O.orc(), (val, idx, ptr, fmt == "csr"), **c.params)
    except O.OracleError as e:
        return e.code
    b = ml_cases.rhs(ptr.shape[0] - 1)
    return dict(L=Q.L, U=Q.U, perm=Q.perm, x=Q.apply(b), xt=Q.apply(b, O.TRANSPOSE), total_nnz=len(Q.L[0]) + len(Q.U[0]), zero_pivots=Q.zero_pivots)


@functools.lru_cache(maxsize=None)
def _alone(name, fmt):
    """what the device does with one orientation of a case built alone: its arrays and solves, or (the message raised,); and the debug line"""
    c = C.CASES[name]
    ptr, idx, val = C.arrays(name)
    n = ptr.shape[0] - 1
    t0 = time.perf_counter()
    with _Env(ILUPP_DEBUG="1"), _Stderr() as cap:
        try:
            out = _measure(_create(c.kind)(val, idx, ptr, fmt == "csr", *_args(c.params)), n)
        except RuntimeError as e:
            out = (str(e),)
    lines = _RE[c.kind].findall(cap.err)
    assert len(lines) == 1, (name, fmt, cap.err[-2000:])
    return out, tuple(int(v) for v in lines[0]), time.perf_counter() - t0


def _judge(name, fmt, got, what):
    want = _expected(name, fmt)
    tag = (name, fmt, what)
    assert isinstance(got, dict) and isinstance(want, dict), tag + (got if not isinstance(got, dict) else "built", want if not isinstance(want, dict) else "built")
    for t in "LU":
        assert np.array_equal(got[t][2], want[t][2]) and np.array_equal(got[t][1], want[t][1]), tag + (t, "pattern")
        _same_values(got[t][0], want[t][0], tag + (t, "values"))
    assert np.array_equal(got["perm"], want["perm"]), tag + ("perm",)
    _same_values(got["x"], want["x"], tag + ("apply",))
    _same_values(got["xt"], want["xt"], tag + ("apply_trans",))
    assert got["total_nnz"] == want["total_nnz"] and got["zero_pivots"] == want["zero_pivots"], tag


@pytest.mark.parametrize("name", C.NAMES)
def test_case(name):
    c = C.CASES[name]
    m = C.model(name)
    ptr = C.arrays(name)[0]
    n = ptr.shape[0] - 1
    for fmt in FORMATS:
        got, (dn, dres, dstatus, dat), dt = _alone(name, fmt)
        print("%s %s: %.4f s, status %d at %d" % (name, fmt, dt, dstatus, dat))
        assert (dn, dres) == (n, m.records[0]["reserved"]), (name, fmt, dn, dres)
        assert (dstatus, dat) == (STATUS[m.err], m.err_at), (name, fmt, "status and row seen", (dstatus, dat), "predicted", (STATUS[m.err], m.err_at), m.err_store)
        if m.err != R.OK:
            assert _expected(name, fmt) == m.err, (name, fmt)
            msg = MESSAGES[(c.kind, m.err)]
            assert got == ((msg % m.err_at) if "%d" in msg else msg,), (name, fmt, got)
        else:
            _judge(name, fmt, got, "alone")


def _groups(kind):
    """the cases both libraries build, by parameter set: one batch each"""
    groups = {}
    for name in C.NAMES:
        c = C.CASES[name]
        if c.kind == kind and C.model(name).err == R.OK:
            groups.setdefault(_args(c.params), []).append(name)
    return groups


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kind", ["tp", "cp"])
def test_members_of_a_batch(kind, fmt):
    """one .batch() call per parameter set, every member the oracle's object and the object built alone"""
    groups = _groups(kind)
    assert sum(len(g) for g in groups.values()) == sum(1 for nm in C.NAMES if C.CASES[nm].kind == kind and C.model(nm).err == R.OK)
    assert max(len(g) for g in groups.values()) >= 10
    for args, names in groups.items():
        B = _create(kind, batch=True)([tuple(C.arrays(nm)[q] for q in (2, 1, 0)) for nm in names], fmt == "csr", *args)
        assert len(B) == len(names)
        for nm, P in zip(names, B):
            got = _measure(P, C.arrays(nm)[0].shape[0] - 1)
            _judge(nm, fmt, got, "member of a batch of %d" % len(names))
            one = _alone(nm, fmt)[0]
            for t in "LU":
                for x, y in zip(got[t], one[t]):
                    assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), (nm, fmt, t)
            assert np.array_equal(got["perm"], one["perm"]) and np.array_equal(got["x"], one["x"], equal_nan=True) and np.array_equal(got["xt"], one["xt"], equal_nan=True)


@pytest.mark.parametrize("kind", ["tp", "cp"])
def test_a_refused_member_is_named(kind):
    """a batch with one of the refused cases in the middle: the reference's message with the member's number"""
    bad = "tp/overU" if kind == "tp" else "cp/overL"
    good = ["%s/n2" % kind, "%s/fitL" % kind]
    c = C.CASES[bad]
    mats = [tuple(C.arrays(nm)[q] for q in (2, 1, 0)) for nm in (good[0], bad, good[1])]
    with pytest.raises(RuntimeError, match=r"matrix 1 of the batch: .*%s.*\(matrix 1 of the batch" % re.escape(MESSAGES[(kind, R.ERR_MEMORY)])):
        _create(kind, batch=True)(mats, True, *_args(c.params))
