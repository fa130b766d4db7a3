#!/usr/bin/env python3
"""Construction wall times of the benchmark's ILUC, C4 and C5 rows (bench.py: extra_config), every repetition printed: the rows whose
host code is the capacity ladders of iluc_df.hip, icholt_df.hip and piluc_df.hip (C4 takes ICholT's grid path in front of its ladder).
usage: ladder_host_times.py [REPS]   -> one JSON line {row: [ms, ...]}, the first (cold) construction of each row left out"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import ilupp_amd as ilupp  # noqa: E402
import matgen  # noqa: E402
from ilupp_amd import _native  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
dev = torch.device("cuda", 0)
prm = ilupp.iluplusplus_precond_parameter()
prm.default_configuration(1)
prm.threshold = 1e-3
ROWS = (
    ("ILUC", lambda: matgen.poisson3d(128), lambda a: _native.ILUCPreconditioner_device(*a, True, 8, 1e-2)),
    ("C4", lambda: matgen.poisson3d(256), lambda a: _native.ICholTPreconditioner_device(*a, True, 0, 0.0)),
    ("C5", lambda: matgen.random_dd(1000000, 8, 25.0, 12345), lambda a: _native.MultilevelILUCDPPreconditioner_device(*a, True, prm)),
)
out = {}
for name, matrix, make in ROWS:
    d, i, p = matrix()
    n = p.shape[0] - 1
    t = [torch.from_numpy(x).to(dev) for x in (d, i, p)]
    args = (t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n)
    ms = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = make(args)
        ms.append(1e3 * (time.perf_counter() - t0))
        P = None
    out[name] = ms[1:]
    del t
    torch.cuda.empty_cache()
print(json.dumps(out))
