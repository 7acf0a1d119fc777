#!/usr/bin/env python3
"""Many-query exact top-k over a resident bf16 bank (PreparedBank.resident) against the resident fp16 bank's search, in ONE
process: Q = 10 000 queries, N = 1 M rows, D = 768, k = 100 (the headline search shape), unit-normal rows.

Legs, interleaved round by round after two warm-ups of each (host clock around a search that ends in a device synchronise):
  fp16        PreparedBank(bank_fp16): one fp16 query pass (that route's default)
  bf16_hi     PreparedBank.resident(bank_bf16), SKYEMB_PREFILTER_LO=0: one bf16 query pass
  bf16_hilo   the same bank, SKYEMB_PREFILTER_LO=1: two passes
and, once, the route a bf16 bank had before -- the token search with one token per row on the bare tensor -- timed on the
first --token-queries queries and scaled by Q / that.  The bf16 result is checked against the token route's on those queries.
Writes one JSON file.  usage: python tools/bench_search_bf16_bank.py [--rounds 10] [--out profiles/search_bf16_1m.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sky_embeddings_amd.search import PreparedBank, cosine_topk


def rows(N, D, dtype):
    g = torch.Generator(device="cuda").manual_seed(2024)
    bank = torch.empty(N, D, device="cuda", dtype=dtype)
    for s in range(0, N, 50_000):
        bank[s:s + 50_000] = torch.randn(min(50_000, N - s), D, device="cuda", generator=g).to(dtype)
    return bank


def timed(queries, bank, k, lo=None, **kw):
    if lo is None:
        os.environ.pop("SKYEMB_PREFILTER_LO", None)
    else:
        os.environ["SKYEMB_PREFILTER_LO"] = lo       # (the library reads it per call)
    st = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s, i = cosine_topk(queries, bank, k, stats=st, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    os.environ.pop("SKYEMB_PREFILTER_LO", None)
    return ms, st, s, i


def summary(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3), "n": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=10_000)
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--token-queries", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "search_bf16_1m.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_search_bf16_bank: no GPU: nothing is measured without one")
    queries = torch.randn(a.Q, a.D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2025))
    w = 1.0 / (torch.rand(a.D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) + 0.5) ** 2
    w = w / w.sum()
    res = {"tool": "bench_search_bf16_bank", "Q": a.Q, "N": a.N, "D": a.D, "k": a.k, "rounds": a.rounds}
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    xb = rows(a.N, a.D, torch.bfloat16)
    torch.cuda.reset_peak_memory_stats()
    pbb = PreparedBank.resident(xb, w)
    pbb.half_image()
    torch.cuda.synchronize()
    res["bf16_alone"] = {"bank_bytes": xb.numel() * 2, "resident_bytes": torch.cuda.memory_allocated() - base}
    timed(queries, pbb, a.k, "0")
    res["bf16_alone"]["peak_bytes"] = torch.cuda.max_memory_allocated() - base
    pbh = PreparedBank(rows(a.N, a.D, torch.float16), w)
    legs = {"fp16": (pbh, None), "bf16_hi": (pbb, "0"), "bf16_hilo": (pbb, "1")}
    for pb, lo in list(legs.values()) * 2:            # warm-up: code objects, row constants, the allocator's blocks
        timed(queries, pb, a.k, lo)
    t = {n: [] for n in legs}
    last = {}
    for _ in range(a.rounds):
        for n, (pb, lo) in legs.items():
            ms, st, s, i = timed(queries, pb, a.k, lo)
            t[n].append(ms)
            last[n] = (st, s, i)
    res["ms"] = {n: summary(v) for n, v in t.items()}
    res["stats"] = {n: {"path": v[0].get("path"), "redone": v[0].get("redone")} for n, v in last.items()}
    res["bf16_variants_same_bits"] = bool(torch.equal(last["bf16_hi"][1], last["bf16_hilo"][1]) and torch.equal(last["bf16_hi"][2], last["bf16_hilo"][2]))
    ms, st, s, i = timed(queries, pbb, a.k)           # SKYEMB_PREFILTER_LO unset: the default variant
    res["bf16_default_ms_once"] = round(ms, 3)
    # the route before: the bare bf16 tensor, token search in groups of 16 queries
    qs = queries[:a.token_queries]
    timed(qs[:32], xb, a.k, weights=w)
    tok = [timed(qs, xb, a.k, weights=w) for _ in range(2)]
    res["token_route"] = {"queries": qs.shape[0], "ms": round(min(x[0] for x in tok), 2), "path": tok[-1][1].get("path"),
                          "scaled_to_Q_ms": round(min(x[0] for x in tok) * a.Q / qs.shape[0], 1)}
    res["bf16_equals_token_route"] = bool(torch.equal(tok[-1][2], last["bf16_hi"][1][:qs.shape[0]]) and
                                          torch.equal(tok[-1][3], last["bf16_hi"][2][:qs.shape[0]]))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
