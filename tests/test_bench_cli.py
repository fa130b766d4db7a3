"""bench.py without a GPU: the fixed sample --dump-outputs keeps of a long array, and the options that only a --full run takes."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_fixed_and_bounded():
    a = np.arange(3 * bench.DUMP_SAMPLE, dtype=np.int32)
    s = bench._dump_sample(a)
    assert s.dtype == np.float64 and s.shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(s, bench._dump_sample(a.copy()))
    assert np.all(np.diff(s) > 0)               # (the array holds its own positions: sorted, none twice)
    small = np.linspace(0.0, 1.0, 1000)
    assert np.array_equal(bench._dump_sample(small), small)
    assert 7 * bench.DUMP_SAMPLE * 8 <= 64 * 10 ** 6      # seven arrays at most


def test_config_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--config needs --full" in r.stderr, r.stderr
