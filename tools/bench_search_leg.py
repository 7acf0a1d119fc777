#!/usr/bin/env python3
"""bench.py's search leg alone (bench.bench_search: the 1M x 768 bank, q1 / q_small / q_large = 10 000 queries, k = 100), without the
training step and the rest of --full: one JSON line {label: {sec, queries_per_sec, path, redone, kernel_ms, checksum}}.
usage: python3 tools/bench_search_leg.py [--bank-rows N --queries Q --topk K]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bank-rows", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=10_000)
ap.add_argument("--topk", type=int, default=100)
res, _ = bench.bench_search(ap.parse_args(), 0, 1, torch.device("cuda", 0))
keep = ("Q", "sec", "queries_per_sec", "path", "redone", "kernel_ms", "checksum")
print(json.dumps({label: {k: r[k] for k in keep} for label, r in res.items()}))
