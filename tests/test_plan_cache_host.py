"""The container of parked analysis plans (ilupp_amd/csrc/plan_cache.h) on the CPU: a stand-alone program over the header alone, built
under AddressSanitizer and UBSan, drives it through its rules -- key equality, a take removes, the least recently parked plan of a device
leaves first and every block of a plan that leaves is released exactly once, drop-all, the byte limit, two threads that park and take."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan_cache") / "plan_cache_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "ilupp_amd", "csrc"), os.path.join(ROOT, "tests", "plan_cache_harness.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_plan_cache_rules_under_sanitizers(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "plan_cache_harness: ok" in r.stdout, r.stdout + r.stderr
