"""The capacity cases (tests/capacity_cases.py) against the demand model, on the CPU: the modelled maxima of every case, that the
on-capacity cases fill a capacity exactly and their twins exceed it by one, and that every step that can stop an attempt of a
route-asserted case stops it for the same cause -- the first capacity code written wins a race in the kernel, so only then is the route
the GPU tests assert deterministic."""
import numpy as np
import pytest
import scipy.sparse as sp

import capacity_cases as K


def _oracle():
    from oracle import oracle as O
    return O.orc()


def _index(dem, q):
    return max(h[q] for d in dem for h in d)


@pytest.mark.parametrize("name", sorted(K.ILUC_TABLE))
def test_table_maxima_and_routes(name):
    A, fill, forced, classes = K.iluc_case(name)
    dem, deps, start, route = K.iluc_model(name, _oracle())
    assert K.maxima(dem) == K.ILUC_TABLE[name][4], name
    assert start == classes[0], (name, start)
    assert route is not None and K.classes_of(route) == classes, (name, route)
    assert route[-1][1] is None


@pytest.mark.parametrize("name", sorted(K.ILUC_TWINS))
def test_twin_routes(name):
    A, fill, forced, classes = K.iluc_case(name)
    dem, deps, start, route = K.iluc_model(name, _oracle())
    assert route is not None and K.classes_of(route) == classes, (name, route)
    if forced is None:
        assert start == classes[0]


@pytest.mark.parametrize("name", sorted(K.ON_CAPACITY))
def test_on_capacity_and_one_over(name):
    q, cap, twin = K.ON_CAPACITY[name]
    dem = K.iluc_model(name, _oracle())[0]
    over = K.iluc_model(twin, _oracle())[0]
    assert _index(dem, q) == cap, (name, _index(dem, q))
    assert _index(over, q) == cap + 1, (twin, _index(over, q))
    # the capacity is one of the class the case completes in
    cls = K.iluc_case(name)[3][-1]
    assert cap == K.ILUC_CLASSES[cls][(1, 2, 0, 1)[q]]


@pytest.mark.parametrize("name", sorted(K.ILUC_TABLE) + sorted(K.ILUC_TWINS))
@pytest.mark.parametrize("transposed", [False, True])
def test_one_cause_per_failing_class(name, transposed):
    """in every class a case leaves, all steps that can fail first agree on records or entries (both input orientations: column input
    hands the kernel the transposed view)"""
    A, fill, forced, classes = K.iluc_case(name)
    dem, deps, start, route = K.iluc_model(name, _oracle(), transposed)
    n = A.shape[0]
    for cls in range(5):
        causes = set(K.failing_causes(dem, deps, K.iluc_class(cls, n)).values())
        assert len(causes) <= 1, (name, cls, causes)
    assert route is not None
    if not transposed:
        assert K.classes_of(route) == classes


def test_forced_classes_hold_what_the_model_says():
    """a class "can hold" a case when no step exceeds it: every case fits class 4, and the class it completes in"""
    for name in sorted(K.ILUC_TABLE):
        A, fill, forced, classes = K.iluc_case(name)
        dem, deps, start, route = K.iluc_model(name, _oracle())
        holds = [c for c in range(5) if not K.failing_causes(dem, deps, K.iluc_class(c, A.shape[0]))]
        assert 4 in holds and classes[-1] in holds, (name, holds)
        assert all(c not in holds for c in classes[:-1]), (name, holds)


def test_ladders():
    assert [K.iluc_next(c, K.RECORDS) for c in range(4)] == [3, 3, 3, 4]
    assert [K.iluc_next(c, K.ENTRIES) for c in range(4)] == [1, 2, 4, 4]
    assert [K.piluc_next(c, K.RECORDS) for c in range(4)] == [2, 2, 3, 4]
    assert [K.piluc_next(c, K.ENTRIES) for c in range(4)] == [1, 2, 4, 4]
    assert K.iluc_class(4, 16384) == (1 << 19, 16384, 4096) and K.iluc_class(4, 16385)[1] == 16384
    assert K.iluc_class(4, 600) == (1 << 19, 1024, 1024)


def test_generators_are_diagonally_dominant():
    for A in (K.arrow_last(34), K.arrow_first(60), K.row_first(129), K.row_first(129, True), K.comb(31, 8, 7), K.comb(119, 8, 8),
              K.spd_arrow_last(18), K.spd_arrow_first(40)):
        A = sp.csr_matrix(A)
        d = np.abs(A.diagonal())
        off = np.asarray(abs(A).sum(axis=1)).ravel() - d
        assert np.all(d > off)
    for A in (K.spd_arrow_last(18), K.spd_arrow_first(40)):
        assert abs(A - A.T).nnz == 0
    t = sp.csr_matrix(K.row_first(40, True))
    assert np.unique(np.abs(t[0, 1:].toarray())).shape[0] == 1


def test_error_cases_on_the_cpu():
    """the oracle's errors that the GPU tests expect from upper classes"""
    from oracle import oracle as O
    B = K.without_diagonal(K.arrow_last(140), (5, 20))
    with pytest.raises(O.OracleError) as ei:
        _oracle().iluc(K.as_input(B), 5, 0.0)
    assert ei.value.code == O.ERR_ZERO_PIVOT and ei.value.row == 5
    F = K.arrow_first(60)
    assert K.iluc_start(F.nnz, 60, 60) == 2
    with pytest.raises(O.OracleError) as ei:
        _oracle().iluc(K.as_input(F), 60, 0.0)
    assert ei.value.code == O.ERR_MEMORY


def test_icholt_arrow_boundary():
    """spd_arrow_last(N): row N-1 is reached by N-1 columns, T is 16 in classes 0..2 (it depends on the average row only): N = 17 fits,
    N = 18 fails three classes on records and completes in the largest, whose T grows with n"""
    for N, fits in ((17, True), (18, False)):
        nnz_tri = 2 * N - 1
        assert [K.icholt_T(nnz_tri, N, 0, c) for c in range(3)] == [16, 16, 16]
        assert (N - 1 <= 16) == fits
        assert K.icholt_T(nnz_tri, N, 0, 3) >= N - 1
    # spd_arrow_first: column 0 of the triangle has N rows: 2048 is the slot capacity of the largest class
    assert K.ICHOLT_LARGEST[1] == 2048 and all(c[1] < 2048 for c in K.ICHOLT_CLASSES)
