"""The capacity ladders as ilupp_amd/csrc/df_ladder.h states them (class tables, status words, start classes, next classes, ICholT's record
counts, the ILUPP_*_CLASS switches) against the independent statement of tests/capacity_cases.py.  The header is plain C++:
tests/df_ladder_harness.cpp is built with g++ under AddressSanitizer and UBSan and prints one line per fact.  No GPU."""
import os
import subprocess

import pytest

import capacity_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# resident waves per CU of the classes (DESIGN_OTHER_PATHS.md: the ICholT table, sections 4c and 4e)
WAVES = {"iluc": (16, 8, 2, 2, 4), "piluc": (16, 8, 2, 2, 4), "icholt": (24, 12, 3, 1)}
# the status words as the ILUPP_DEBUG lines print them (tests/test_gpu_capacity_ladders.py parses them; capacity_cases.py's docstring)
STATUS = {"ok": 0, "capacity": 1, "timeout": 2, "pivot_nan": 3, "pivot_dropped": 4, "own_part": 11, "records_read": 12, "entries": 13, "slots": 14,
          "records_written": 15, "stores": 16}


@pytest.fixture(scope="module")
def facts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("df_ladder") / "df_ladder_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "ilupp_amd", "csrc"), os.path.join(ROOT, "tests", "df_ladder_harness.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    e = {k: v for k, v in os.environ.items() if not k.startswith("ILUPP_")}
    r = subprocess.run([out], capture_output=True, text=True, env=e, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("df_ladder_harness: ok\n"), r.stdout[-2000:] + r.stderr
    by_kind = {}
    for line in r.stdout.splitlines()[:-1]:
        w = line.split()
        by_kind.setdefault(w[0], []).append(w[1:])
    return by_kind


def _cause(status):
    return K.RECORDS if status in (12, 15) else K.ENTRIES


def test_status_words_and_attempt_codes(facts):
    (w,) = facts["status"]
    assert dict(zip(w[0::2], (int(x) for x in w[1::2]))) == STATUS
    assert facts["attempt"] == [["outside", "1", "stores", "2"]]


def test_class_tables(facts):
    rows = {(w[0], int(w[1])): tuple(int(x) for x in w[2:]) for w in facts["class"]}
    expected = {}
    for c in range(4):
        expected[("iluc", c)] = K.ILUC_CLASSES[c]
        expected[("piluc", c)] = K.PILUC_CLASSES[c]
    # the largest classes: the limits their run-time sizes grow to (partial ILUC: 2^26 entries, its slots grow with the matrix)
    expected[("iluc", 4)] = K.iluc_class(4, 10 ** 6)
    expected[("piluc", 4)] = (1 << 26, 0, K.iluc_class(4, 10 ** 6)[2])
    for c in range(3):
        expected[("icholt", c)] = K.ICHOLT_CLASSES[c]
    expected[("icholt", 3)] = K.ICHOLT_LARGEST
    assert {k: v[:3] for k, v in rows.items()} == expected
    assert {k: v[3] for k, v in rows.items()} == {(f, c): WAVES[f][c] for f in WAVES for c in range(len(WAVES[f]))}


def test_crout_record_counts(facts):
    assert len(facts["records"]) > 100
    for w in facts["records"]:
        if w[0] == "icholt":
            nnz, n, fill, cls, T = (int(x) for x in w[1:])
            want = K.icholt_T(nnz, n, fill, cls)
            assert T == (-1 if want is None else want), w
        else:
            n, cls, T = (int(x) for x in w[1:])
            table = K.ILUC_CLASSES if w[0] == "iluc" else K.PILUC_CLASSES
            assert T == (table[cls][2] if cls < 4 else K.iluc_class(4, n)[2]), w


def test_icholt_refuses_in_classes_0_and_1_only(facts):
    refused = {int(w[4]) for w in facts["records"] if w[0] == "icholt" and int(w[5]) == -1}
    assert refused == {0, 1}


def test_start_classes(facts):
    seen = set()
    for w in facts["start"]:
        v = [int(x) for x in w[1:]]
        if w[0] == "iluc":
            assert v[3] == K.iluc_start(v[0], v[1], v[2]), w
        else:
            assert v[2] == K.piluc_start(v[0], v[1]), w
        seen.add((w[0], v[-1]))
    assert seen == {(f, c) for f in ("iluc", "piluc") for c in (0, 1, 2)}           # (the grid reaches every start class of both)


def test_next_classes(facts):
    got = {(w[0], int(w[1]), int(w[2])): int(w[3]) for w in facts["next"]}
    want = {}
    for s in (0, 11, 12, 13, 14, 15):
        for c in range(5):
            # (status 0: an attempt that refused before its launch -- ILUC goes to the next class, partial ILUC treats it like entries)
            want[("iluc", c, s)] = c + 1 if s == 0 else K.iluc_next(c, _cause(s))
            if c < 4:
                want[("piluc", c, s)] = K.piluc_next(c, _cause(s))
    # ICholT (status 1, or 0 for a refusal before the launch): always the next class, 4 = refused (capacity_cases.py has no rule to restate:
    # test_gpu_capacity_ladders.py pins 0 -> 1 -> 2 -> 3 and the refusal)
    want.update({("icholt", c, s): c + 1 for c in range(4) for s in (0, 1)})
    assert got == want
    assert got[("iluc", 4, 13)] == 5 and got[("iluc", 4, 12)] == 5                 # past the largest class: refused


def test_start_class_switches(facts):
    got = {(w[0], w[1]): int(w[2]) for w in facts["env"]}
    # negative: 0; ILUC and partial ILUC clamp to their largest class; ICholT above 3: class 4, where its ladder makes no attempt
    assert got == {("iluc", "-1"): 0, ("iluc", "0"): 0, ("iluc", "3"): 3, ("iluc", "4"): 4, ("iluc", "5"): 4, ("iluc", "unset"): 1,
                   ("piluc", "-1"): 0, ("piluc", "0"): 0, ("piluc", "3"): 3, ("piluc", "4"): 4, ("piluc", "5"): 4, ("piluc", "unset"): 2,
                   ("icholt", "-1"): 0, ("icholt", "0"): 0, ("icholt", "3"): 3, ("icholt", "4"): 4, ("icholt", "5"): 4, ("icholt", "unset"): 0}
