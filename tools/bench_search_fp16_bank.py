#!/usr/bin/env python3
"""Many-query exact top-k over a resident fp16 bank against the same search over the fp32 bank it widens to, in ONE process:
Q = 10 000 queries, N = 1 M rows, D = 768, k = 100 (the headline search shape).

Memory first, each bank built alone (its PreparedBank + half_image + one search): resident bytes and the peak.  Then both
banks side by side, searches alternating fp32 / fp16 after a warm-up of each; host clock around a search that ends in a device
synchronise.  Prints one JSON line: ms per search of both (median, min, max over the rounds), the queries re-run exactly, the
memory figures, and whether both routes returned the same bits.
usage: python tools/bench_search_fp16_bank.py [--Q 10000] [--N 1000000] [--D 768] [--k 100] [--rounds 10]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sky_embeddings_amd.search import PreparedBank, cosine_topk


def rows_fp16(N, D):
    g = torch.Generator(device="cuda").manual_seed(2024)
    bank = torch.empty(N, D, device="cuda", dtype=torch.float16)
    for s in range(0, N, 50_000):
        bank[s:s + 50_000] = torch.randn(min(50_000, N - s), D, device="cuda", generator=g).to(torch.float16)
    return bank


def built_alone(bank, w, queries, k):
    """Resident and peak bytes of one PreparedBank with its half image and one search, the bank's own bytes included."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    pb = PreparedBank(bank, w)
    pb.half_image()
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()
    cosine_topk(queries, pb, k)
    torch.cuda.synchronize()
    return {"bank_bytes": bank.numel() * bank.element_size(), "resident_bytes": resident, "peak_bytes": torch.cuda.max_memory_allocated()}


def timed(queries, pb, k):
    st = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s, i = cosine_topk(queries, pb, k, stats=st)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, st, s, i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=10_000)
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_search_fp16_bank: no GPU: nothing is measured without one")
    queries = torch.randn(a.Q, a.D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2025))
    w = 1.0 / (torch.rand(a.D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) + 0.5) ** 2
    w = w / w.sum()
    base = torch.cuda.memory_allocated()
    x16 = rows_fp16(a.N, a.D)
    mem16 = built_alone(x16, w, queries, a.k)
    x32 = x16.float()                      # the widened bank: the same rows
    del x16
    mem32 = built_alone(x32, w, queries, a.k)
    for m in (mem16, mem32):
        m["resident_bytes"] -= base
        m["peak_bytes"] -= base
    x16 = x32.to(torch.float16)            # exact: every element is an fp16 value
    pb32, pb16 = PreparedBank(x32, w), PreparedBank(x16, w)
    for pb in (pb32, pb16):                # warm-up: code objects, the half images, the allocator's blocks
        timed(queries, pb, a.k)
        timed(queries, pb, a.k)
    t32, t16 = [], []
    for _ in range(a.rounds):
        ms, st32, s32, i32 = timed(queries, pb32, a.k)
        t32.append(ms)
        ms, st16, s16, i16 = timed(queries, pb16, a.k)
        t16.append(ms)

    def summary(t):
        return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    print(json.dumps({"tool": "bench_search_fp16_bank", "Q": a.Q, "N": a.N, "D": a.D, "k": a.k, "rounds": a.rounds,
                      "fp32_ms": summary(t32), "fp16_ms": summary(t16), "fp32_path": st32["path"], "fp16_path": st16["path"],
                      "fp32_redone": st32["redone"], "fp16_redone": st16["redone"],
                      "same_bits": bool(torch.equal(s32, s16) and torch.equal(i32, i16)),
                      "fp32_alone": mem32, "fp16_alone": mem16}))


if __name__ == "__main__":
    main()
