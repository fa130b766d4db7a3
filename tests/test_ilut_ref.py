"""The CPU model of the wave-parallel ILUT kernel (tests/ilut_ref.py) against the oracle, and the cases of tests/ilut_cases.py against the
figures that put them on their boundaries: for every case and both orientations the model's L and U have the oracle's bits (and the
reference's own where oracle/_ref was built), the records show what the case's name says (CASES[name].pin), and route() gives the route
written in the table -- so a case that drifts off its boundary fails here, without a GPU."""
import numpy as np
import pytest

import ilut_cases as C
import ilut_ref as R


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


model = C.model


def inputs(name):
    """(format, oracle input) of both orientations: the CSC arrays of the transpose are the CSR arrays of the matrix"""
    A = C.matrix(name)
    d, i, p = A.data.astype(np.float64), A.indices.astype(np.int32), A.indptr.astype(np.int32)
    return (("csr", (d, i, p, True)), ("csc", (d, i, p, False)))


def _same(got, want, what):
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]), what
    assert np.array_equal(_u64(got[0]), _u64(want[0])), what


@pytest.mark.parametrize("name", C.NAMES)
def test_model_has_the_oracles_bits(name):
    from oracle import oracle as O
    L, U, _ = model(name)
    c = C.CASES[name]
    libs = [("oracle", O.orc())] + ([("reference", O.ref())] if O.ref_available() else [])
    for who, lib in libs:
        for fmt, M in inputs(name):
            Lo, Uo = lib.ilut(M, c.p, c.tau)
            assert bool(Lo[3]) == (fmt == "csr") and bool(Uo[3]) == (fmt == "csr")
            if fmt == "csc":                   # (binding.cpp:440-444: the factors of column input come back swapped)
                Lo, Uo = Uo, Lo
            _same(L, Lo, (name, who, fmt, "L")); _same(U, Uo, (name, who, fmt, "U"))


@pytest.mark.parametrize("name", C.NAMES)
def test_case_is_on_its_boundary(name):
    _, _, rows = model(name)
    c = C.CASES[name]
    n = len(rows)
    route, events = R.route(rows, n, c.p)
    assert route == c.route, (name, route, c.route)
    if route[0] is not None:
        assert route[0] == route[1] + route[2] + route[3] == len(events)
    c.pin(rows, events, c.p)


def test_the_list_covers_every_route_event():
    """a tier-1 overflow by each of the three causes, a mid-row move after at least one elimination, an end move, a restart in tier 3,
    the natural fall-back to the largest class by each of its three causes, the largest class at once"""
    seen = set()
    for name in C.NAMES:
        _, _, rows = model(name)
        route, events = R.route(rows, len(rows), C.CASES[name].p)
        for e in events.values():
            seen.update(("t1:" + e[0], "t2:%s" % e[1], "t3:%s" % e[2]))
        if route[0] is None:
            seen.add("big at once")
    for want in ("t1:pool", "t1:uslots", "t1:kept", "t2:ok", "t2:move", "t2:endmove", "t2:restart:pool", "t2:restart:uslots", "t2:restart:kept",
                 "t3:ok", "t3:pool", "t3:uslots", "t3:kept", "big at once"):
        assert want in seen, (want, sorted(seen))


def test_switches_change_the_route():
    """ILUPP_ILUT_NO_TIER2=1: nothing leaves tier 2 because nothing enters it; ILUPP_ILUT_CAP=256: the p <= 32 cases take the routes of
    the larger class"""
    for name in C.TIER_CASES:
        _, _, rows = model(name)
        r, ev = R.route(rows, len(rows), C.CASES[name].p, tier2=False)
        assert r[:4] == C.CASES[name].route[:4] and r[4] == 0 and r[5] == 0 and all(e[1] is None and e[2] == "ok" for e in ev.values()), name
    want = {"pool128": C.OK, "pool129": C.OK, "uslots128": C.OK, "uslots129": C.OK, "chain128": C.OK, "chain129": C.OK, "left502": (1, 1, 0, 0, 0, 0, False),
            "left513": (1, 1, 0, 0, 0, 0, False)}
    assert sorted(want) == sorted(C.CAP256_CASES)
    for name in C.CAP256_CASES:
        _, _, rows = model(name)
        assert R.route(rows, len(rows), C.CASES[name].p, cap256=True)[0] == want[name], name


def test_select_orders_and_ties():
    """the dropping step alone: strict >, (magnitude desc, position asc), the sort only for a tie at the cut among more than 16"""
    from oracle import oracle as O
    sort = O.orc().sort_slots_by_abs_desc
    cols = np.arange(40, 0, -1)
    vals = np.array([(-1.0) ** q * (1.0 + (q % 5)) for q in range(40)])
    sel, rec = R.select(cols, vals, 3, 0.0, sort)
    assert rec["ncand"] == 40 and rec["tie"] and rec["sorted"] and rec["nsel"] == 3 and np.all(np.abs(vals[sel]) == 5.0)
    assert list(cols[sel]) == sorted(cols[sel])
    sel, rec = R.select(cols[:10], vals[:10], 3, 0.0, sort)
    assert rec["tie"] and not rec["sorted"] and sorted(sel) == [3, 4, 9]                 # 5.0 at 4 and 9, then the FIRST 4.0 (3, not 8)
    sel, rec = R.select(cols[:10], vals[:10], 2, 0.0, sort)
    assert not rec["tie"] and sorted(sel) == [4, 9]
    sel, rec = R.select(cols[:10], vals[:10], 9, 0.45, sort)                             # norm = sqrt(110): the threshold is 4.72
    assert rec["ncand"] == 2 and sorted(sel) == [4, 9]
    assert R.select(cols, vals, 0, 0.0, sort)[1]["nsel"] == 0
    assert R.clip_p(0, 7) == 1 and R.clip_p(9, 7) == 7
