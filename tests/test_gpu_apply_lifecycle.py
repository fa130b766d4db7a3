"""Apply-state lifecycle: ONE object through a sequence of applies, block applies, batched applies, re-factorisations and factor
read-backs, every result compared bit for bit (uint64 views, no tolerance) with the oracle's for the value set the object holds AT THAT
MOMENT.  The host layer (ilupp_amd/csrc/api.hip) builds many forms lazily and keeps them per object; the rest of the suite runs
construct -> apply -> apply_trans on fresh objects, so nothing there varies the ORDER of calls.  Here the transposed static records, the
transposed storages, all four level-ordered copies, the block buffers and the CSR value copy exist when the values change, a transposed
apply is the first call of an object, applies and batched launches are in flight when the next call comes.

A stale copy gives a plausible vector, so a mismatch is looked up among the results under the OTHER value sets: the message names the
case, the sequence so far, the operation, and which value set the result belongs to.  Cases, op model and sequences:
lifecycle_cases.py; that the value sets can be told apart at all: test_lifecycle_cases.py.

    a, t      host apply / apply_trans                    A, T     apply_ on a device vector, not waited for; read back at the next sync
    AA, TA    two of them in flight, then sync            B*, Bt*  host block apply, k = 3 and 9, one column with a NaN
    C, Ct     apply_batch_ with a small twin, sync off    R        re-factorisation with the next value set (ILU(0))
    F         factors_info() against the oracle's factors"""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
import lifecycle_cases as LC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _caller_stream():
    """the device wrappers order the library on torch's current stream; the modules after this one start as they would without it"""
    yield
    from ilupp_amd import _native
    _native.set_caller_stream(0, False)


_DEVICE = {}


def _device_matrix(key, d, i, p):
    """DeviceCSR per (case, value set), uploaded once"""
    import torch
    import ilupp_amd.device as ild
    if key not in _DEVICE:
        dev = torch.device("cuda", 0)
        _DEVICE[key] = ild.DeviceCSR(torch.from_numpy(np.array(d)).to(dev), torch.from_numpy(np.array(i)).to(dev), torch.from_numpy(np.array(p)).to(dev))
    return _DEVICE[key]


def _device_pool(case):
    import torch
    key = ("pool", case.name)
    if key not in _DEVICE:
        _DEVICE[key] = torch.from_numpy(np.array(LC.rhs_pool(case.n))).to(torch.device("cuda", 0))
    return _DEVICE[key]


class Runner:
    """one object of `case` and the operations on it; `run` checks every result against LC.expected for the current value set"""

    def __init__(self, case, vecwave=True):
        import ilupp_amd.device as ild
        self.case, self.model, self.vecwave = case, LC.Model(case), vecwave
        self.done, self.pending, self.applied = [], [], False
        self.twin = None
        A0 = self._matrix(0)
        if case.batch:
            self.M, self.twin = ild.DevicePreconditioner.batch("ILU0", [A0, self._twin_matrix()])
        else:
            self.M = ild.DevicePreconditioner(case.kind, A0, **case.params)
        self.pr = self.M.pr
        # the object is on the path the case is about, before anything is concluded from it
        path = self.pr.path()
        assert path == case.path, (case.name, path)
        if case.refactor:
            assert case.kernels(self.pr.kernel_names(), vecwave), (case.name, self.pr.kernel_names())

    def _matrix(self, k):
        _, i, p = self.case.matrix
        return _device_matrix((self.case.name, k), LC.values(self.case, k), i, p)

    @staticmethod
    def _twin_matrix():
        return _device_matrix(("twin", 0), *LC.twin_matrix())

    def _twin(self):
        import ilupp_amd.device as ild
        if self.twin is None:
            self.twin = ild.DevicePreconditioner("ILU0", self._twin_matrix())
        return self.twin

    # ---- checking -----------------------------------------------------------------------------------------------------------------------
    def _check(self, op, k, idx, got, at):
        want = LC.expected(self.case, k, op)[idx]
        got = np.asarray(got)
        if LC.same_bits(got, want):
            return
        bad = np.flatnonzero((LC.bits(got) != LC.bits(want)).reshape(want.shape[0], -1).any(axis=1)) if got.shape == want.shape else []
        raise AssertionError("%s: after [%s], operation %s (result %d, value set %d): %d of %d rows differ (first %s); the result %s"
                             % (self.case.name, " ".join(self.done[:at + 1]), op, idx, k, len(bad), want.shape[0],
                                bad[:1].tolist() if len(bad) else "-", LC.diagnose(self.case, k, op, idx, got)))

    def _drain(self):
        """wait for everything in flight and compare what it wrote, each with the value set of ITS moment"""
        import torch
        if not self.pending:
            return
        self.M.sync()
        torch.cuda.synchronize()
        pending, self.pending = self.pending, []
        for (op, k, idx, x, at) in pending:
            self._check(op, k, idx, x.cpu().numpy(), at)

    # ---- operations ---------------------------------------------------------------------------------------------------------------------
    def _host(self, op):
        x = np.array(LC.rhs_pool(self.case.n)[:, 0])
        (self.pr.apply if op == "a" else self.pr.apply_trans)(x)
        self._check(op, self.model.cur, 0, x, len(self.done) - 1)
        self.applied = True

    def _device(self, op, idx, col, transpose):
        x = _device_pool(self.case)[:, col].contiguous()
        self.M.apply_(x, transpose=transpose)
        self.pending.append((op, self.model.cur, idx, x, len(self.done) - 1))
        self.applied = True

    def _block(self, op):
        k, transpose = int(op[-1]), op.startswith("Bt")
        pool = LC.rhs_pool(self.case.n)
        X = np.ascontiguousarray(pool if k == LC.POOL else pool[:, LC.B3_COLS]).copy()
        self.pr.apply_block(X, transpose=transpose)
        self._check(op, self.model.cur, 0, X, len(self.done) - 1)
        assert self.pr.block_path() == self.case.block, (self.case.name, op, self.pr.block_path())

    def _batched(self, op):
        import torch
        import ilupp_amd.device as ild
        from ilupp_amd import _native
        n, twin = self.case.n, self._twin()
        assert n <= _native.pivot_apply_batch_max_n(), (self.case.name, n)
        x = torch.cat([_device_pool(self.case)[:, 2].contiguous(), torch.from_numpy(G.rhs(twin.n)).to(torch.device("cuda", 0))])
        routes = ild.apply_batch_([self.M, twin], x, [0, n], transpose=(op == "Ct"))
        assert list(routes) == [0, 0], (self.case.name, op, routes)        # both members in the launch
        at = len(self.done) - 1
        self.pending.append((op, self.model.cur, 0, x[:n], at))
        self.pending.append((op, self.model.cur, 1, x[n:], at))

    def _factors(self, op):
        info = self.pr.factors_info()
        want = LC.oracle_factors(self.case, self.model.cur)
        assert len(info) == len(want), (self.case.name, len(info))
        for idx, (f, w) in enumerate(zip(info, want)):
            assert bool(f[3]) == bool(w[3]) and np.array_equal(f[2], w[2]) and np.array_equal(f[1], w[1]), (self.case.name, "pattern of factor", idx)
            self._check(op, self.model.cur, idx, f[0], len(self.done) - 1)

    def step(self, op):
        self.done.append(op)
        self.model.step(op)
        if op in ("a", "t"):
            self._host(op)
        elif op in ("A", "T"):
            self._device(op, 0, 1, op == "T")
            return                                         # stays in flight
        elif op in ("AA", "TA"):
            self._device(op, 0, 1, op == "TA")
            self._device(op, 1, 2, False)
        elif op[0] == "B":
            self._block(op)
        elif op in ("C", "Ct"):
            self._batched(op)
            return                                         # stays in flight
        elif op == "R":
            self.M.refactor_(self._matrix(self.model.cur))
        else:
            self._factors(op)
        self._drain()

    def run(self, seq):
        for op in LC.parse(seq):
            self.step(op)
        self._drain()
        if self.applied and not self.case.refactor:
            # (an LL^T object names the sweeps of its pair once an apply has analysed it)
            assert self.case.kernels(self.pr.kernel_names(), self.vecwave), (self.case.name, self.pr.kernel_names())
        return self


def _fixed():
    return [pytest.param(c, num, toks, id="%s-seq%d" % (c.name, num)) for c in LC.CASES for num, toks in LC.fixed_sequences(c).items()]


@pytest.mark.parametrize("case,num,toks", _fixed())
def test_fixed_sequence(case, num, toks):
    Runner(case).run(toks)


@pytest.mark.parametrize("j", [0, 1])
@pytest.mark.parametrize("case", LC.CASES, ids=[c.name for c in LC.CASES])
def test_random_sequence(case, j):
    """12 operations from the case's alphabet, at most 3 re-factorisations; ILUPP_FUZZ_OFFSET shifts the seeds"""
    Runner(case).run(LC.random_sequences(case)[j])


_NO_VECWAVE_SCRIPT = r'''
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import lifecycle_cases as LC
import test_gpu_apply_lifecycle as T
case = LC.BY_NAME["box24x30x20"]
for num in (2, 4, 5):
    r = T.Runner(case, vecwave=False).run(LC.FIXED[num])
    print("SEQ %%d kernels=%%s" %% (num, ";".join(r.pr.kernel_names())), flush=True)
print("lifecycle ok")
'''


def test_box_grid_without_vector_wave_sweeps():
    """ILUPP_NO_VECWAVE=1 (read once per process): the sweeps are k_sptrsv_wx on the level-major copies, the path of a schedule with
    vec_ok false.  Sequences 2, 4 and 5 on the box grid."""
    code = _NO_VECWAVE_SCRIPT % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ILUPP_NO_VECWAVE="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lifecycle ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SEQ ")]
    assert len(lines) == 3, lines
    for ln in lines:
        assert "kernels=k_ilu0_wa<" in ln and ";k_sptrsv_wx<1, false>;k_sptrsv_wx<-1, true>" in ln, ln


_DECLINED_SCRIPT = r'''
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import lifecycle_cases as LC
import test_gpu_apply_lifecycle as T
for name in ("upwind_z_slab32", "upwind_y32"):
    for num in (7, 2):
        T.Runner(LC.BY_NAME[name]).run(LC.FIXED[num])
        print("RAN %%s %%d" %% (name, num), flush=True)
print("lifecycle ok")
'''


def test_upwind_objects_decline_their_transposed_records_once():
    """The two upwind cases are where static sweeps (apply) and generic ones (apply_trans) alternate on one object.  That their transposed
    static records ARE declined shows only in the library's debug line (ILUPP_DEBUG=1: "static transposed records: a of b entries of U,
    c of d of L", c < d), hence a child; and it is tried once per object, however many transposed applies and re-factorisations follow."""
    code = _DECLINED_SCRIPT % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ILUPP_DEBUG="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lifecycle ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stderr.splitlines() if "static transposed records:" in ln]
    assert len(lines) == 4, lines                                       # four objects, one attempt each
    for ln in lines:
        f = ln.split("static transposed records:")[1].replace(",", " ").split()
        u_got, u_all, l_got, l_all = int(f[0]), int(f[2]), int(f[6]), int(f[8])
        assert u_got == u_all and l_got < l_all, ln
