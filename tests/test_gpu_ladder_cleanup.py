"""A factorisation that walks its capacity ladder gives back every pool block of every attempt: ilupp_hip_live_blocks() reads the same
before and after a second run of a case that hops between classes, is refused, doubles its stores or ends with an error in a forced
class.  The cases and their routes are pinned (bit for bit against the oracle) by tests/test_gpu_capacity_ladders.py; here the route is
asserted only to show that the ladder was walked.  The scheme of tests/test_gpu_construct_cleanup.py: a first run absorbs what the
process sets up once, and the objects of the second run are dropped and collected before the second reading."""
import gc

import pytest
import scipy.sparse as sp

import capacity_cases as K
import matgen
import ml_cases as C
from test_gpu_capacity_ladders import NOPRE, _Env, _piluc_attempts, _route, _without_store_growth

pytestmark = pytest.mark.gpu


def _iluc(A, fill):
    def run():
        import ilupp_amd as ilupp
        return ilupp.ILUCPreconditioner(A, fill_in=fill, threshold=0.0)
    return run


def _icholt(A):
    def run():
        import ilupp_amd as ilupp
        return ilupp.ICholTPreconditioner(A, add_fill_in=0, threshold=0.0)
    return run


def _ml(A):
    def run():
        import ilupp_amd as ilupp
        from test_gpu_ml import _native_ml
        return _native_ml(A, C.engine_params(ilupp, *NOPRE))
    return run


def _random_dd_300():
    d, i, p = matgen.random_dd(300, k=9)
    return sp.csr_matrix((d, i, p), shape=(300, 300))


def _not_spd_17():
    """the 17 x 17 SPD arrow (16 reaches of the last row: T = 16 holds them in every class) with one negative diagonal entry"""
    A = K.spd_arrow_last(17).tolil()
    A[5, 5] = -1.0
    A = A.tocsr(); A.sort_indices()
    return A


def _classes(family):
    return lambda err: [c for c, _ in _route(err, family)]


def _icholt_attempts(err):
    return _route(err, "icholt")


def _piluc_classes(err):
    return [a[0] for a in _without_store_growth(_piluc_attempts(err)[0])]


def _piluc_store_growth(err):
    """the statuses of the attempts: "stores too small" (16) at least once, then 0"""
    return [a[3] for a in _piluc_attempts(err)[0]]


# id -> (constructor, environment, the exception it ends with or None, what the ILUPP_DEBUG lines must show)
CASES = {
    "iluc-0-1-2-4": (lambda: _iluc(K.row_first(600, True), 5), {}, None, (_classes("iluc"), [0, 1, 2, 4])),
    "iluc-0-3": (lambda: _iluc(K.arrow_last(34), 5), {}, None, (_classes("iluc"), [0, 3])),
    "iluc-refused-16385": (lambda: _iluc(K.row_first(16385), 5), {}, (NotImplementedError, K.ILUC_REFUSAL), (_classes("iluc"), [0, 1, 2, 4])),
    "piluc-0-1-2-4": (lambda: _ml(_random_dd_300()), {"ILUPP_NO_PILUC_CHAIN": 1}, None, (_piluc_classes, [0, 1, 2, 4])),
    "piluc-store-doubling": (lambda: _ml(_random_dd_300()), {"ILUPP_NO_PILUC_CHAIN": 1, "ILUPP_PILUC_CLASS": 4}, None, (_piluc_store_growth, None)),
    "icholt-0-1-2-3": (lambda: _icholt(K.spd_arrow_last(18)), {}, None, (_classes("icholt"), [0, 1, 2, 3])),
    "icholt-refused-2049": (lambda: _icholt(K.spd_arrow_first(2049)), {}, (RuntimeError, "largest capacity class"), (_classes("icholt"), [0, 1, 2, 3])),
    "icholt-not-spd-class-2": (lambda: _icholt(_not_spd_17()), {"ILUPP_ICHOLT_CLASS": 2}, (RuntimeError, "not positive definite"),
                               (_icholt_attempts, [(2, 3)])),
}


def _once(run, raises):
    if raises is None:
        P = run()
        del P
    else:
        with pytest.raises(raises[0], match=raises[1]):
            run()
    gc.collect()


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_walked_ladder_leaves_no_block(capfd, name):
    from ilupp_amd import _native
    make, env, raises, (seen_of, expected) = CASES[name]
    run = make()
    with _Env(ILUPP_DEBUG=1, **env):
        _once(run, raises)                      # (a first run: what the process sets up once, on first use, is no leak)
        before = _native.live_blocks()
        capfd.readouterr()
        _once(run, raises)
        err = capfd.readouterr().err
        after = _native.live_blocks()
    seen = seen_of(err)
    if expected is None:
        assert len(seen) >= 2 and set(seen[:-1]) == {16} and seen[-1] == 0, (name, seen)
    else:
        assert seen == expected, (name, seen)
    assert after == before, (name, before, after)
