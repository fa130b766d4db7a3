"""Recorded answers of the REAL reference for the live comparisons of tests/test_oracle_*.py and tests/test_pivot_ref.py (tests/ref_replay.py): runs those tests
against oracle/_ref and keeps, for every call they make of it, a digest of the call and a digest of the reference's answer.

Run where the reference's sources are present:   make -C oracle ref && python tests/golden/make_golden_live.py    -> tests/golden/ref_live.npz"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pytest  # noqa: E402

import ref_replay  # noqa: E402
from oracle import oracle as O  # noqa: E402

TESTS = ["test_oracle_golden.py::test_oracle_vs_reference_live", "test_oracle_golden.py::test_restatement_vs_reference_on_fuzz_matrices",
         "test_oracle_iluc.py::test_restatement_vs_reference_live", "test_oracle_ilucp.py::test_oracle_against_reference_live",
         "test_oracle_ilucp.py::test_mem_factor_is_truncated_before_the_product", "test_oracle_ilutp.py::test_oracle_against_reference_live",
         "test_oracle_ml.py::test_oracle_against_reference_live", "test_oracle_ml.py::test_oracle_against_reference_fuzz",
         "test_oracle_mlp.py::test_oracle_against_reference_live", "test_pivot_ref.py::test_oracle_agrees_with_the_reference"]


def main():
    if not O.ref_available():
        raise SystemExit("oracle/_ref not built: make -C oracle ref")
    if os.environ.get("ILUPP_FUZZ_OFFSET", "0") != "0":
        raise SystemExit("record with the default seeds (ILUPP_FUZZ_OFFSET unset)")
    ref_replay.start_recording()
    rc = pytest.main(["-q", "-p", "no:cacheprovider"] + [os.path.join(ROOT, "tests", t) for t in TESTS])
    if rc != 0:
        raise SystemExit("the live tests failed: nothing recorded")
    print("%d calls -> %s" % (ref_replay.save_recording(), ref_replay.GOLDEN))


if __name__ == "__main__":
    main()
