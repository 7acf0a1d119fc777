#!/usr/bin/env python3
"""Many-query top-k over a SELECTION of a prepared bank (cosine_topk(queries, PreparedBank, k, select=Selection)) against the
unselected search and the two routes there were before, in ONE process per bank dtype: Q = 10 000, N = 1 M, D = 768, k = 100.

Legs, interleaved round by round after a warm-up of each (host clock around a call that ends in a device synchronise):
  unselected            the whole bank
  all / r50 / r10       the feature under an all-True, a 50 % random and a 10 % random selection (every tile stays live)
  runs10                10 % of the rows in contiguous runs of 4096 (about 90 % of the tiles empty)
  tokens_r10            alternative 1: cosine_topk(queries, flat bank, k, select=...), the token search in groups of 16 queries --
                        timed on the first --token-queries queries and scaled by Q / that (recorded as "scaled_from")
  compact_r10           alternative 2: PreparedBank(bank[flags]) built from scratch + one search (gather, norms, half image)
and, once per selection, the preparation the Selection keeps (two short launches + a read-back).
Writes one JSON file.  usage: python tools/bench_search_select.py [--rounds 10] [--out profiles/search_select_1m.json]
(--slow-rounds 0 leaves the two alternatives out, --dtypes fp32 runs one bank: a short run for a kernel trace; --dtypes takes fp32, fp16
and bf16 -- the 16-bit banks are built through PreparedBank.resident)"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sky_embeddings_amd.search import PreparedBank, Selection, cosine_topk


def rows(N, D, dtype):
    g = torch.Generator(device="cuda").manual_seed(2024)
    bank = torch.empty(N, D, device="cuda", dtype=dtype)
    for s in range(0, N, 50_000):
        bank[s:s + 50_000] = torch.randn(min(50_000, N - s), D, device="cuda", generator=g).to(dtype)
    return bank


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3), "n": len(t)}


def one_dtype(a, dtype, queries, w):
    bank = rows(a.N, a.D, dtype)
    pb = PreparedBank(bank, w) if dtype == torch.float32 else PreparedBank.resident(bank, w)   # (a bf16 bank has no other way in)
    g = torch.Generator(device="cuda").manual_seed(11)
    u = torch.rand(a.N, device="cuda", generator=g)
    runs = torch.rand((a.N + 4095) // 4096, device="cuda", generator=g) < 0.1
    flags = {"all": torch.ones(a.N, device="cuda", dtype=torch.bool), "r50": u < 0.5, "r10": u < 0.1,
             "runs10": runs.repeat_interleave(4096)[:a.N].contiguous()}
    sels = {n: Selection(f) for n, f in flags.items()}
    out = {"selected": {n: s.count for n, s in sels.items()}}
    pb.half_image()
    out["prepare_ms"] = {n: round(clock(lambda s=s: s.prefilter(pb))[0], 3) for n, s in sels.items()}
    stats = {n: {} for n in sels}
    legs = {"unselected": lambda: cosine_topk(queries, pb, a.k)}
    for n, s in sels.items():
        legs[n] = lambda s=s, n=n: cosine_topk(queries, pb, a.k, stats=stats[n], select=s)
    qs = queries[:a.token_queries]
    slow = {"tokens_r10": lambda: cosine_topk(qs, bank, a.k, weights=w, select=sels["r10"]),
            "compact_r10": lambda: cosine_topk(queries, (PreparedBank if dtype == torch.float32 else PreparedBank.resident)(
                bank[flags["r10"]], w), a.k)}
    if a.slow_rounds == 0:                                        # (a profiler run of the feature's own legs)
        slow = {}
    for fn in list(legs.values()) * 2 + list(slow.values()):      # warm-up: code objects, images, the allocator's blocks
        fn()
    t = {n: [] for n in list(legs) + list(slow)}
    for r in range(a.rounds):
        for n, fn in legs.items():
            t[n].append(clock(fn)[0])
        if r < a.slow_rounds:
            for n, fn in slow.items():
                t[n].append(clock(fn)[0])
    out["ms"] = {n: summary(v) for n, v in t.items()}
    if slow:
        scale = a.Q / qs.shape[0]
        out["ms"]["tokens_r10"] = {"scaled_from": {"queries": qs.shape[0], **out["ms"]["tokens_r10"]},
                                   "median": round(out["ms"]["tokens_r10"]["median"] * scale, 1)}
    out["stats"] = {n: {"redone": s.get("redone"), "tiles": s.get("tiles"), "path": s.get("path")} for n, s in stats.items()}
    s0, i0 = legs["unselected"]()
    s1, i1 = legs["all"]()
    out["all_equals_unselected"] = bool(torch.equal(s0, s1) and torch.equal(i0, i1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=10_000)
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--slow-rounds", type=int, default=3)
    ap.add_argument("--token-queries", type=int, default=512)
    ap.add_argument("--dtypes", default="fp32,fp16")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "search_select_1m.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_search_select: no GPU: nothing is measured without one")
    queries = torch.randn(a.Q, a.D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2025))
    w = 1.0 / (torch.rand(a.D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) + 0.5) ** 2
    w = w / w.sum()
    res = {"tool": "bench_search_select", "Q": a.Q, "N": a.N, "D": a.D, "k": a.k, "rounds": a.rounds}
    for name in a.dtypes.split(","):
        res[name] = one_dtype(a, {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[name], queries, w)
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
