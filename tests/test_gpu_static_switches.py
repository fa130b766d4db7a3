"""The static level-major form (ilupp_amd/csrc/st.hip) under the switches that choose between its kernel generations.  st.hip reads each
switch once into a static, so every setting runs in a fresh interpreter:

* {}                  the wave-exchange schedules and kernels wherever the lanes fit their classes;
* ILUPP_NO_WR=1       round 3's skews and round 2's sweeps for every object (the link kernel then skips the lane classification);
* ILUPP_PACK_FMT0=1   a factor pair's records by template position first, converted to the class-aligned format by a second pass.

Each child builds IChol0 on a 17 x 33 x 65 grid (symmetrically scaled; its analysis runs one schedule, the sweeps of its stored pair two),
ILU(0) on a 64 x 48 x 40 grid and ILU(0) on test_gpu_paths.py's mesh with missing transposed entries (k_ilu0_st and the sweeps of round
2): the smallest shapes that still reach 16 x 16 patches, more than one workgroup and an export across a tile border.  Factors, apply and
apply_trans must be array-equal to the oracle under every setting.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r'''
import sys, numpy as np, scipy.sparse as sp
sys.path[:0] = [%(root)r, %(tests)r]
import matgen, golden_util as G, ilupp_amd as ilupp
import test_gpu_paths as TP
from ilupp_amd import _native
from oracle import oracle as O

def ichol0():
    d, i, p = matgen.poisson3d(17, 33, 65)
    n = p.shape[0] - 1
    A = sp.csr_matrix((d, i, p), shape=(n, n))
    D = sp.diags(1.0 + 0.5 * np.random.default_rng(7).random(n))          # symmetric scaling: stays positive definite
    A = (D @ A @ D).tocsr(); A.sort_indices()
    P = ilupp.IChol0Preconditioner(A)
    Lo = O.orc().ichol0((A.data, A.indices, A.indptr, True))
    (L,) = P.factors()
    assert G.mat_equal((L.data, L.indices, L.indptr, isinstance(L, sp.csr_matrix)), Lo)
    b = G.rhs(n)
    want = O.orc().apply_llt(Lo, b, O.ID)
    for rep in range(2):
        x = b.copy(); P.apply(x)
        assert np.array_equal(x, want)
        xt = b.copy(); P.apply_trans(xt)
        assert np.array_equal(xt, want)
    return P.pr.path(), P.pr.kernel_names()

def ilu0(d, i, p):
    d = d * (1.0 + 0.25 * np.random.default_rng(3).random(d.shape[0]))
    n = p.shape[0] - 1
    P = _native.ILU0Preconditioner(d, i, p, True)
    L, U = O.orc().ilu0((d, i, p, True))
    (ld, li, lp, _, _, _), (ud, ui, up, _, _, _) = P.factors_info()
    assert np.array_equal(lp, L[2]) and np.array_equal(li, L[1]) and np.array_equal(up, U[2]) and np.array_equal(ui, U[1])
    assert np.array_equal(ld, L[0]) and np.array_equal(ud, U[0])
    b = np.random.default_rng(1).random(n)
    for rep in range(2):
        x = b.copy(); P.apply(x)
        assert np.array_equal(x, O.orc().apply_lu(L, U, b, O.ID))
        xt = b.copy(); P.apply_trans(xt)
        assert np.array_equal(xt, O.orc().apply_lu(L, U, b, O.TRANSPOSE))
    return P.path(), P.kernel_names()

for name, run in (("ichol0", ichol0), ("ilu0-grid", lambda: ilu0(*matgen.poisson3d(64, 48, 40))), ("ilu0-mesh", lambda: ilu0(*TP._mesh_missing_upper()))):
    path, kernels = run()
    print("CASE %%s path=%%s kernels=%%s oracle=True" %% (name, path, ";".join(kernels)), flush=True)
'''

_SETTINGS = {
    "default": {},
    "no_wr": {"ILUPP_NO_WR": "1"},
    "pack_fmt0": {"ILUPP_PACK_FMT0": "1"},
}


def _run(setting):
    code = _SCRIPT % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    e = dict(os.environ)
    e.update(_SETTINGS[setting])
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    return {ln.split()[1]: ln for ln in r.stdout.splitlines() if ln.startswith("CASE ")}


@pytest.mark.parametrize("setting", list(_SETTINGS))
def test_static_form_gives_the_oracles_bits_under_every_switch(setting):
    got = _run(setting)
    assert sorted(got) == ["ichol0", "ilu0-grid", "ilu0-mesh"], got
    assert "path=ichol0:static-level-major " in got["ichol0"] and "kernels=k_ichol0_st;" in got["ichol0"], got["ichol0"]
    assert "path=ilu0:static-level-major " in got["ilu0-mesh"] and "kernels=k_ilu0_st;" in got["ilu0-mesh"], got["ilu0-mesh"]
    assert "path=ilu0:static-" in got["ilu0-grid"], got["ilu0-grid"]
    if setting == "no_wr":
        # round 2's sweeps for every object
        for ln in got.values():
            assert "k_sptrsv_st<" in ln and "k_sptrsv_w" not in ln, ln
