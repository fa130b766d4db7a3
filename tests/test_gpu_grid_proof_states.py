"""GPU tests of the four states of the box-grid proof protocol (api.hip: ilu0_factor; st_wave.hip: ilu0_numeric_wx): who proves the
guessed pattern -- the factor launch itself behind its tiles, or k_grid_check on the side stream -- and which factor kernel runs, the
wave-exchange kernel (which takes the verdict along with its own read-back) or another one (ILUPP_NO_WXF=1: the proof is then queued in
front of the verdict's read-back by the host).  The switches are read once per process, so every state runs in a child process.

One box grid, 33 x 50 x 40 -- the smallest 3-D shape of test_gpu_grid.py with ny, nz >= 16; 4 x 3 patches, fewer than any chip has CUs,
so the tail proof is wanted --, and its twin with one column index moved in a middle row.  Per state: the true grid takes the grid
analysis and the twin the general one, each with the bits of a process under ILUPP_NO_GRID=1 (factors, total_nnz, one apply, one
apply_trans); the true grid is taken for a grid again after the failed proof.  In the default state, a re-factorisation of the
grid-built object with scaled values equals a fresh construction from those values, factors and a following apply."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import hashlib, sys
sys.path[:0] = [%(root)r, %(tests)r]
refactor = len(sys.argv) > 1 and sys.argv[1] == "refactor"
if refactor:
    import torch                 # (before the library opens the device, as in the test processes: tests/conftest.py)
    torch.cuda.init()
import numpy as np, matgen
from ilupp_amd import _native

def digest(P, n):
    h = hashlib.sha256()
    for f in P.factors_info():
        for a in f[:3]:
            h.update(np.ascontiguousarray(a).tobytes())
    h.update(str(P.total_nnz).encode())
    b = np.random.default_rng(11).random(n)
    x = b.copy(); P.apply(x); h.update(x.tobytes())
    x = b.copy(); P.apply_trans(x); h.update(x.tobytes())
    return h.hexdigest()

nx, ny, nz = 33, 50, 40
d, i, p = matgen.poisson3d(nx, ny, nz)
d = d * (1.0 + 0.25 * np.random.default_rng(7).random(d.shape[0]))
n = p.shape[0] - 1
# the twin: row r in the middle of the grid, one off-diagonal column moved to the free place next to it (sorted, same count)
r = (nz // 2) * nx * ny + (ny // 2) * nx + nx // 2
i2 = i.copy()
row = i2[p[r]:p[r + 1]]
for j in range(row.shape[0]):
    nxt = row[j + 1] if j + 1 < row.shape[0] else n
    if row[j] != r and row[j] + 1 < nxt:
        row[j] += 1
        break
assert not np.array_equal(i, i2)

P = _native.ILU0Preconditioner(d, i, p, True)
print("TRUE", P.analysis_path(), P.kernel_names()[0].replace(" ", ""), digest(P, n), flush=True)
P = _native.ILU0Preconditioner(d, i2, p, True)
print("MOVED", P.analysis_path(), digest(P, n), flush=True)
P = _native.ILU0Preconditioner(d, i, p, True)
print("AGAIN", P.analysis_path(), flush=True)

if refactor:
    dev = torch.device("cuda", 0)
    td, ti, tp = (torch.from_numpy(a).to(dev) for a in (d, i, p))
    torch.cuda.synchronize()
    Pd = _native.ILU0Preconditioner_device(td.data_ptr(), ti.data_ptr(), tp.data_ptr(), n, True)
    built = Pd.analysis_path()
    td2 = torch.from_numpy(d * 1.5).to(dev)
    torch.cuda.synchronize()
    Pd.refactor_device(td2.data_ptr(), ti.data_ptr(), tp.data_ptr())
    Pf = _native.ILU0Preconditioner(d * 1.5, i, p, True)
    b = np.random.default_rng(6).random(n)
    x = torch.from_numpy(b).to(dev)
    Pd.apply_device(x.data_ptr(), n, transpose=False, sync=True)
    y = b.copy(); Pf.apply(y)
    same_apply = bool(np.array_equal(x.cpu().numpy(), y))
    same_factors = all(np.array_equal(a, c) for f, g in zip(Pd.factors_info(), Pf.factors_info()) for a, c in zip(f[:3], g[:3]))
    print("REFACTOR", built, Pf.analysis_path(), same_factors, same_apply, flush=True)
"""

WX, SD = "k_ilu0_wa<0,4,4>", "k_ilu0_sd"
_STATES = {
    "tail-proof-wx": ({}, WX),
    "side-proof-wx": ({"ILUPP_GRID_TAIL_PROOF": "0"}, WX),
    "tail-proof-other-kernel": ({"ILUPP_NO_WXF": "1"}, SD),
    "side-proof-other-kernel": ({"ILUPP_NO_WXF": "1", "ILUPP_GRID_TAIL_PROOF": "0"}, SD),
}
_dead = []          # the first child that faulted, aborted or ran into its time limit: nothing is started after it
_ref = {}


def _child(env, *args):
    if _dead:
        pytest.fail("not started: an earlier child process ended badly (%s)" % _dead[0])
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    e = {k: v for k, v in os.environ.items() if k not in ("ILUPP_NO_GRID", "ILUPP_NO_WXF", "ILUPP_GRID_TAIL_PROOF", "ILUPP_NO_WR")}
    e.update(env)
    try:
        r = subprocess.run([sys.executable, "-c", code] + list(args), capture_output=True, text=True, timeout=120, env=e, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _dead.append("%r: time limit" % (env,))
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
        _dead.append("%r: exit status %d" % (env, r.returncode))
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    return {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l.strip()}


def _reference():
    """the digests of the general pass (ILUPP_NO_GRID=1), computed once"""
    if not _ref:
        got = _child({"ILUPP_NO_GRID": "1"})
        assert got["TRUE"][0] == got["MOVED"][0] == got["AGAIN"][0] == "general", got
        _ref.update(got)
    return _ref


@pytest.mark.parametrize("state", list(_STATES))
def test_each_proof_state_gives_the_general_pass_bits(state):
    env, kernel = _STATES[state]
    ref = _reference()
    got = _child(env, *(["refactor"] if not env else []))
    # the true grid: grid analysis, this state's factor kernel, the general pass' bits
    assert got["TRUE"][:2] == ["grid", kernel], got
    assert got["TRUE"][2] == ref["TRUE"][2], got
    # one moved column: never the grid; the bits of the general pass for THIS matrix
    assert got["MOVED"][0] == "general", got
    assert got["MOVED"][1] == ref["MOVED"][1], got
    # ... and the true grid is a grid again afterwards
    assert got["AGAIN"] == ["grid"], got
    if not env:
        # re-factorisation of the grid-built object = a fresh construction from the scaled values, factors and a following apply
        assert got["REFACTOR"] == ["grid", "grid", "True", "True"], got
