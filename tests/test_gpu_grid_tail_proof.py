"""GPU tests of the tail proof (st_wave.hip: wa_tail_proof): on a box grid whose factor launch holds one workgroup per CU, no k_grid_check
runs in front of k_ilu0_wa -- the workgroups whose tile has ended check every row's pointer and columns against the closed form, late in
the launch, and the verdict comes home with the kernel's read-back.  What is tested: true grids give the reference's bits with the tail
proof and without it (ILUPP_GRID_TAIL_PROOF=0); a pattern that differs from the grid in ONE row -- wherever that row lies in the proof's
slices -- or in the last row pointer is never taken for the grid; verdict word, claim counter and the remembered shape survive a failed
proof; a launch of more tiles than CUs keeps the separate proof.  Everything is compared, as arrays, with the oracle's restatement of
the reference (ILU0.hpp:26-106, sparse_implementation.h:4040-4087)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import matgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE = 4096                      # rows of one claim (st_wave.hip: kTailSlice)
DIMS = (64, 48, 40)               # n = 122880 = 30 slices; 3 x 3 tiles


def _unsym(d, seed):
    return d * (1.0 + 0.25 * np.random.default_rng(seed).random(d.shape[0]))


_grids = {}


def _grid(dims, seed=7):
    if dims not in _grids:
        d, i, p = matgen.poisson3d(*dims)
        _grids[dims] = (_unsym(d, seed), i, p)
    return _grids[dims]


def _digest(P, n):
    h = hashlib.sha256()
    for f in P.factors_info():
        for a in f[:3]:
            h.update(np.ascontiguousarray(a).tobytes())
    x = np.ones(n); P.apply(x); h.update(x.tobytes())
    return h.hexdigest()


def _equals_oracle(P, a):
    """factors (values and index arrays) and apply(ones), array-equal"""
    from oracle import oracle as O
    d, i, p = a
    n = p.shape[0] - 1
    L, U = O.orc().ilu0((d, i, p, True))
    (ld, li, lp, _, _, _), (ud, ui, up, _, _, _) = P.factors_info()
    for got, want in ((lp, L[2]), (li, L[1]), (up, U[2]), (ui, U[1]), (ld, L[0]), (ud, U[0])):
        assert np.array_equal(got, want)
    x = np.ones(n); P.apply(x)
    assert np.array_equal(x, O.orc().trisolve(U, O.UPPER, O.ID, O.orc().trisolve(L, O.LOWER, O.ID, np.ones(n))))


def _move_a_column(i, p, r):
    """row r with one off-diagonal column moved to the free place next to it (sorted, same count, diagonal kept)"""
    n = p.shape[0] - 1
    i = i.copy()
    row = i[p[r]:p[r + 1]]
    for j in range(row.shape[0]):
        nxt = row[j + 1] if j + 1 < row.shape[0] else n
        if row[j] != r and row[j] + 1 < nxt:
            row[j] += 1
            return i
    raise AssertionError("row %d has no column to move" % r)


_CHILD = r"""
import hashlib, sys
sys.path[:0] = [%r, %r]
import numpy as np, matgen
from ilupp_amd import _native
for dims in ((64, 48, 40), (40, 33, 50)):
    d, i, p = matgen.poisson3d(*dims)
    d = d * (1.0 + 0.25 * np.random.default_rng(7).random(d.shape[0]))
    P = _native.ILU0Preconditioner(d, i, p, True)
    h = hashlib.sha256()
    for f in P.factors_info():
        for a in f[:3]:
            h.update(np.ascontiguousarray(a).tobytes())
    x = np.ones(p.shape[0] - 1); P.apply(x); h.update(x.tobytes())
    print(P.path(), P.analysis_path(), ";".join(P.kernel_names()), h.hexdigest())
"""


def test_true_grids_with_and_without_the_tail_proof():
    """(a) 64 x 48 x 40, and 40 x 33 x 50 (n = 66000: no multiple of the slice or of 256, a partial last slice): grid analysis, the
    static direct path, the reference's bits -- and the same path, kernels and bits from a process with ILUPP_GRID_TAIL_PROOF=0"""
    from ilupp_amd import _native
    mine = []
    for dims in (DIMS, (40, 33, 50)):
        a = _grid(dims)
        n = a[2].shape[0] - 1
        assert n % SLICE != 0 or dims == DIMS
        P = _native.ILU0Preconditioner(a[0], a[1], a[2], True)
        assert P.analysis_path() == "grid" and P.path() == "ilu0:static-direct"
        assert P.kernel_names()[0] == "k_ilu0_wa<0, 4, 4>"
        _equals_oracle(P, a)
        mine.append("%s %s %s %s" % (P.path(), P.analysis_path(), ";".join(P.kernel_names()), _digest(P, n)))
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ILUPP_GRID_TAIL_PROOF="0"), cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [l for l in r.stdout.splitlines() if l.strip()] == mine


N = DIMS[0] * DIMS[1] * DIMS[2]


@pytest.mark.parametrize("r", [1, 100, SLICE - 1, SLICE, N - 2000, N - 1],
                         ids=["next-to-row-0", "first-slice", "slice-end", "slice-start", "last-slice", "last-row"])
def test_one_moved_column_is_caught_wherever_its_row_lies(r):
    """(b) the general path with the reference's bits for THIS matrix, never the grid's"""
    from ilupp_amd import _native
    d, i, p = _grid(DIMS)
    i2 = _move_a_column(i, p, r)
    P = _native.ILU0Preconditioner(d, i2, p, True)
    assert P.analysis_path() == "general"
    _equals_oracle(P, (d, i2, p))


def test_a_last_row_pointer_that_is_not_the_count_handed_in():
    """(b) ptr[n] = nnz - 1 on the device, nnz handed in (a shape remembered from the true grid is guessed without reading anything):
    only the proof's look at ptr[n] can tell.  No object comes back as a grid -- the reading way finds the last row without its diagonal"""
    import torch
    from ilupp_amd import _native
    d, i, p = _grid(DIMS)
    n, nnz = p.shape[0] - 1, int(p[-1])
    dev = torch.device("cuda", 0)
    td, ti, tp = (torch.from_numpy(a).to(dev) for a in (d, i, p))
    torch.cuda.synchronize()
    P = _native.ILU0Preconditioner_device(td.data_ptr(), ti.data_ptr(), tp.data_ptr(), n, True, nnz=nnz)      # (learns the shape)
    assert P.analysis_path() == "grid"
    tp[n] = nnz - 1
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        _native.ILU0Preconditioner_device(td.data_ptr(), ti.data_ptr(), tp.data_ptr(), n, True, nnz=nnz)
    tp[n] = nnz
    torch.cuda.synchronize()
    P = _native.ILU0Preconditioner_device(td.data_ptr(), ti.data_ptr(), tp.data_ptr(), n, True, nnz=nnz)
    assert P.analysis_path() == "grid"
    _equals_oracle(P, (d, i, p))


def test_good_bad_good_on_one_index_array():
    """(c) the same device arrays, changed in place: a stale claim counter would let the bad matrix through unchecked, a stale verdict
    would refuse the good one; the failed proof forgets the remembered shape and the next good construction learns it again"""
    import torch
    from ilupp_amd import _native
    d, i, p = _grid(DIMS)
    n, nnz = p.shape[0] - 1, int(p[-1])
    r = 17 * SLICE + 77
    i2 = _move_a_column(i, p, r)
    q = int(np.nonzero(i2 != i)[0][0])
    dev = torch.device("cuda", 0)
    td, ti, tp = (torch.from_numpy(a).to(dev) for a in (d, i, p))
    torch.cuda.synchronize()

    def make():
        return _native.ILU0Preconditioner_device(td.data_ptr(), ti.data_ptr(), tp.data_ptr(), n, True, nnz=nnz)

    for rep in range(2):
        P = make()
        assert P.analysis_path() == "grid" and P.path() == "ilu0:static-direct"
        _equals_oracle(P, (d, i, p))
        ti[q] = int(i2[q]); torch.cuda.synchronize()
        P = make()
        assert P.analysis_path() == "general"
        _equals_oracle(P, (d, i2, p))
        ti[q] = int(i[q]); torch.cuda.synchronize()
    P = make()                                     # (the reading way: learns the shape again)
    assert P.analysis_path() == "grid"
    P = make()                                     # (... and this one recalls it)
    assert P.analysis_path() == "grid" and P.kernel_names()[0] == "k_ilu0_wa<0, 4, 4>"
    _equals_oracle(P, (d, i, p))


def test_more_tiles_than_cus_keeps_the_separate_proof():
    """(d) 16 x 272 x 272: 289 tiles, more than the chip has CUs -- the workgroups of such a launch hand their CU on, k_grid_check runs"""
    from ilupp_amd import _native
    dims = (16, 272, 272)
    d, i, p = _grid(dims, seed=3)
    P = _native.ILU0Preconditioner(d, i, p, True)
    assert P.analysis_path() == "grid" and P.path() == "ilu0:static-direct"
    _equals_oracle(P, (d, i, p))
    i2 = _move_a_column(i, p, 700001)
    P = _native.ILU0Preconditioner(d, i2, p, True)
    assert P.analysis_path() == "general"
    _equals_oracle(P, (d, i2, p))


def test_sixteen_random_rows():
    """(e) every row is covered: 16 seeded single-row perturbations, all caught"""
    from ilupp_amd import _native
    d, i, p = _grid(DIMS)
    rng = np.random.default_rng(20240)
    for r in rng.integers(1, N, size=16):
        i2 = _move_a_column(i, p, int(r))
        assert not np.array_equal(i2, i)
        P = _native.ILU0Preconditioner(d, i2, p, True)
        assert P.analysis_path() == "general", int(r)
        _equals_oracle(P, (d, i2, p))
