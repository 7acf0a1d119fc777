#!/usr/bin/env python3
"""Host-bound leg of the row-bank search: wall time of 200 back-to-back ``cosine_topk`` calls with one synchronise at the end, after
20 warm-up calls, on the row bank of tests/golden/make_row_trace_golden.py (N = 4608, D = 128) at Q = 40, k = 5 -- once on the fp32
PreparedBank, once on the resident bf16 one.  So small a search is all host time: the request, the driver, the read-back of the redo
flags.  One JSON line {bank: ms per 200 calls}.
usage: python3 tools/bench_row_host.py [--calls 200 --warmup 20]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sky_embeddings_amd.search import cosine_topk  # noqa: E402
from tests.golden.make_row_trace_golden import RowFixture  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
a = ap.parse_args()
fx = RowFixture()
out = {}
for name in ("pb32", "res_bf16"):
    for n in (a.warmup, a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            cosine_topk(fx.q, fx.banks[name], 5)
        torch.cuda.synchronize()
        out[name] = round((time.perf_counter() - t0) * 1e3, 3)
print(json.dumps(out))
