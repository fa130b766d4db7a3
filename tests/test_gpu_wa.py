"""GPU parity tests of the ILU(0) factor kernel of box grids (ilupp_amd/csrc/st_wave.hip: k_ilu0_wa; reference ILU0.hpp:26-106): the
wave-exchange factor kernel fed by LDS-DMA, without a barrier in its loop, with prefetcher waves reading ahead for the tiles at work.

* every case gives the oracle's factors (values, indices and row pointers of L and U) and the oracle's apply, bit for bit, in both
  record layouts the kernel writes: the default (L's records compact, format 2) and ILUPP_NO_COMPACT_L=1 (format 1, the layout
  whenever the vector-wave sweeps do not run); the two layouts give the same digest;
* on box grids whose patches are cut by the domain, with more tiles than the chip holds workgroups (the prefetchers must not stay
  behind their tile's end then), 2-D and 3-D, CSR and CSC, nonsymmetric values, a value array that is only 8-byte aligned;
* the kernel the object reports (ilupp_hip_kernel_names) is k_ilu0_wa<0, 4, 4>, and k_ilu0_sd below 16 lines in y.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r'''
import sys, hashlib, numpy as np, scipy.sparse as sp
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import matgen, golden_util as G, ilupp_amd as ilupp
from ilupp_amd import _native
from oracle import oracle as O
rng = np.random.default_rng(17)
big = sys.argv[1] == "big"
def check(name, data, indices, indptr, is_csr, factors, apply):
    """factors and one apply against the oracle; a digest over both"""
    Lo, Uo = O.orc().ilu0((data, indices, indptr, is_csr))
    (L, U) = factors
    assert G.mat_equal(L, Lo) and G.mat_equal(U, Uo), name
    x = np.linspace(-1.0, 2.0, indptr.shape[0] - 1)
    y = x.copy(); apply(y)
    assert np.array_equal(y, O.orc().apply_lu(Lo, Uo, x, O.ID)), name
    h = hashlib.sha256()
    for M in (L, U):
        for a in M[:3]:
            h.update(np.ascontiguousarray(a).tobytes())
    h.update(y.tobytes())
    return h.hexdigest()[:24]
cases = []
shapes = ((24, 24, 24), (70, 45, 37), (100, 60, 40), (17, 33, 65), (40, 272, 272)) if not big else ((96, 160, 144),)
for shape in shapes:
    d, i, p = matgen.poisson3d(*shape)
    cases.append(("7pt%%dx%%dx%%d" %% shape, sp.csr_matrix((d * (1.0 + 0.3 * rng.random(d.shape[0])), i, p))))
if not big:
    d, i, p = matgen.poisson2d(300, 300)
    cases.append(("5pt", sp.csr_matrix((d * (1.0 + 0.3 * rng.random(d.shape[0])), i, p))))
    d, i, p = matgen.poisson3d(33, 20, 50)
    cases.append(("csc", sp.csr_matrix((d * (1.0 + 0.3 * rng.random(d.shape[0])), i, p)).tocsc()))
for name, A in cases:
    A.indices = A.indices.astype(np.int32); A.indptr = A.indptr.astype(np.int32)
    csr = sp.isspmatrix_csr(A)
    P = ilupp.ILU0Preconditioner(A)
    L, U = P.factors()
    dig = check(name, A.data, A.indices, A.indptr, csr, [(M.data, M.indices, M.indptr, csr) for M in (L, U)], P.apply)
    print("CASE %%s %%s path=%%s kernels=%%s oracle=True" %% (name, dig, P.pr.path(), ";".join(P.pr.kernel_names())), flush=True)
if not big:
    # a value array that is only 8-byte aligned (the DMA windows are 16-byte pieces)
    d, i, p = matgen.poisson3d(40, 40, 40)
    d = d * (1.0 + 0.3 * rng.random(d.shape[0]))
    n = p.shape[0] - 1
    dev = torch.device("cuda", 0)
    buf = torch.zeros(d.shape[0] + 1, dtype=torch.float64, device=dev)
    buf[1:] = torch.from_numpy(d).to(dev)
    ti, tp = torch.from_numpy(i).to(dev), torch.from_numpy(p).to(dev)
    P = _native.ILU0Preconditioner_device(buf[1:].data_ptr(), ti.data_ptr(), tp.data_ptr(), n, True)
    fi = P.factors_info()
    dig = check("misaligned", d, i, p, True, [(f[0], f[1], f[2], True) for f in fi[:2]], P.apply)
    print("CASE misaligned %%s path=%%s kernels=%%s oracle=True" %% (dig, P.path(), ";".join(P.kernel_names())), flush=True)
'''

_VARIANTS = {
    "default": {},
    "format1": {"ILUPP_NO_COMPACT_L": "1"},      # L's records as {lA, 1} pairs (the default leaves the constant out: format 2)
}


def _run(variant, size="small"):
    code = _SCRIPT % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    e = dict(os.environ)
    e.update(_VARIANTS[variant])
    r = subprocess.run([sys.executable, "-c", code, size], env=e, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("CASE "):
            f = ln.split()
            out[f[1]] = (f[2], ln)
    return out


@pytest.fixture(scope="module")
def runs():
    return {}


def _cached(runs, variant):
    if variant not in runs:
        runs[variant] = _run(variant)
    return runs[variant]


@pytest.mark.parametrize("variant", ["default", "format1"])
def test_every_variant_gives_the_oracles_bits(variant, runs):
    got = _cached(runs, variant)
    assert len(got) == 8, got
    for name, (digest, line) in got.items():
        assert "oracle=True" in line, line
        if name.startswith("7pt"):
            assert "kernels=k_ilu0_wa<0, 4, 4>;" in line, line


def test_both_record_layouts_give_the_same_bits(runs):
    a, b = _cached(runs, "default"), _cached(runs, "format1")
    assert {k: v[0] for k, v in a.items()} == {k: v[0] for k, v in b.items()}


def test_medium_grid_against_oracle():
    got = _run("default", "big")
    assert len(got) == 1 and all("oracle=True" in v[1] for v in got.values()), got


def test_random_box_shapes_predicted_sizes_and_edge_tiles():
    """Box grids of random dimensions (patches cut by the domain in y and z, lines of 16 .. 90 rows, more or fewer tiles than the chip
    has workgroups): the closed-form analysis' predicted sizes must be what the device finds (a mismatch redoes the construction the
    general way and shows as another path), and factors + apply are the oracle's bits.  ILUPP_FUZZ_OFFSET shifts the seed."""
    import numpy as np
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import matgen
    import scipy.sparse as sp
    import ilupp_amd as ilupp
    from oracle import oracle as O
    rng = np.random.default_rng(4242 + int(os.environ.get("ILUPP_FUZZ_OFFSET", "0")))
    done = 0
    while done < 10:
        nx, ny, nz = int(rng.integers(16, 91)), int(rng.integers(8, 71)), int(rng.integers(8, 71))
        if nx * ny * nz < (1 << 16) or ny * nz < 512:
            continue
        done += 1
        d, i, p = matgen.poisson3d(nx, ny, nz)
        d = d * (1.0 + 0.3 * rng.random(d.shape[0]))
        n = p.shape[0] - 1
        A = sp.csr_matrix((d, i, p), shape=(n, n))
        P = ilupp.ILU0Preconditioner(A)
        assert P.pr.path() == "ilu0:static-direct", ((nx, ny, nz), P.pr.path())
        assert P.pr.analysis_path() == "grid", ((nx, ny, nz), P.pr.analysis_path())
        # (fewer than 16 lines in y: the z-neighbour is not lane - 16, the wave-exchange kernels decline and k_ilu0_sd runs)
        assert P.pr.kernel_names()[0] == ("k_ilu0_wa<0, 4, 4>" if ny >= 16 else "k_ilu0_sd"), ((nx, ny, nz), P.pr.kernel_names())
        Lo, Uo = O.orc().ilu0((d, i, p, True))
        L, U = P.factors()
        assert np.array_equal(L.indptr, Lo[2]) and np.array_equal(L.indices, Lo[1]) and np.array_equal(U.indptr, Uo[2]) and np.array_equal(U.indices, Uo[1]), (nx, ny, nz)
        assert np.array_equal(L.data, Lo[0]) and np.array_equal(U.data, Uo[0]), (nx, ny, nz)
        b = rng.random(n)
        x = b.copy(); P.apply(x)
        assert np.array_equal(x, O.orc().apply_lu(Lo, Uo, b, O.ID)), (nx, ny, nz)
