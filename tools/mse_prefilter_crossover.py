#!/usr/bin/env python
"""Where the two-stage weighted-MSE token route starts to pay: ``distance_topk_tokens(.., 'MSE', combine)`` over a resident fp16
bank of N = 15 625 images x P = 64 tokens x D = 768, k = 100, for Q in {32, 64, 128, 256, 512, 1024}, by the grouped route
(SKYEMB_TOPK_PREFILTER=0: one pass over the bank per 16 queries) and by the two-stage route WITH its row-constants launch (the
TokenBank's held constants are dropped before every timed call).  The two routes alternate inside one process, call by call, so
drift of the clocks and of the shared host hits both alike; every call is timed by a host clock around a device synchronise, one
warm-up call per route and shape first; the table holds the median and the spread of the repeats.

``TOKEN_MSE_PREFILTER_MIN_Q`` (sky_embeddings_amd/search.py) is the smallest Q of the grid at which the two-stage route is at least
10 % faster under BOTH combines -- the margin keeps the choice outside the box-to-box spread the README records -- or 1024 when it
wins nowhere.

    python tools/mse_prefilter_crossover.py --out profiles/mse_prefilter_crossover.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sky_embeddings_amd import search  # noqa: E402

GRID = (32, 64, 128, 256, 512, 1024)
MARGIN = 0.10


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=15625)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(0)
    N, P, D, k = a.images, a.tokens, a.dim, a.k
    # embedding-like rows: standardised features, tokens of an image share a direction
    bank = (torch.randn(N, 1, D, device="cuda", generator=g) + 0.7 * torch.randn(N, P, D, device="cuda", generator=g)).to(getattr(torch, a.dtype))
    w = torch.rand(D, device="cuda", generator=g) + 0.1
    tb = search.TokenBank.resident(bank, w)
    search.TOKEN_MSE_PREFILTER_MIN_Q = search.TOKEN_MSE_PREFILTER_MIN_Q_SMALL = 1      # the route under test decides by the switch alone
    rows = []
    for combine in ("min", "max"):
        for Q in GRID:
            idx = torch.randint(0, N, (Q,), device="cuda", generator=g)
            q = (bank[idx, 0].float() + 0.3 * torch.randn(Q, D, device="cuda", generator=g)).contiguous()   # targets near bank tokens

            def grouped():
                os.environ["SKYEMB_TOPK_PREFILTER"] = "0"
                st = {}
                out = search.distance_topk_tokens(q, tb, k, "MSE", combine, stats=st)
                assert st["path"] == "tokens"
                return out

            def two_stage():
                os.environ["SKYEMB_TOPK_PREFILTER"] = "1"
                tb._stage1_mse = None                         # the row-constants launch is part of the call
                st = {}
                out = search.distance_topk_tokens(q, tb, k, "MSE", combine, stats=st)
                assert st["path"] == "prefiltered", st
                return out, st["redone"]

            ref = timed(grouped)[1]
            (got, redone) = timed(two_stage)[1]
            same = bool(torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]))
            tg, tn = [], []
            for _ in range(a.reps):
                tg.append(timed(grouped)[0])
                tn.append(timed(two_stage)[0])
            row = dict(combine=combine, Q=Q, grouped_ms=statistics.median(tg), two_stage_ms=statistics.median(tn),
                       grouped_ms_all=tg, two_stage_ms_all=tn, redone=redone, bit_equal=same)
            row["speedup"] = row["grouped_ms"] / row["two_stage_ms"]
            rows.append(row)
            print(json.dumps({kk: row[kk] for kk in ("combine", "Q", "grouped_ms", "two_stage_ms", "speedup", "redone", "bit_equal")}), flush=True)
    wins = [Q for Q in GRID if all(r["two_stage_ms"] <= (1.0 - MARGIN) * r["grouped_ms"] for r in rows if r["Q"] >= Q)]
    result = dict(shape=dict(N=N, P=P, D=D, k=k, dtype=a.dtype), reps=a.reps, margin=MARGIN, device=torch.cuda.get_device_name(0), rows=rows,
                  min_q=min(wins) if wins else None, note="two_stage_ms includes the row-constants launch (skyemb_token_mse_rowp)")
    print(json.dumps(dict(min_q=result["min_q"])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
