#!/usr/bin/env python
"""Where the two-stage weighted-MSE token route starts to pay with PER-QUERY weights (the opt-in route of ``distance_topk_tokens``:
``TokenBank.prepare_mse_per_query``): the bank of tools/mse_prefilter_crossover.py -- N = 15 625 images x P = 64 tokens x D = 768,
k = 100, fp16 and bf16 -- for Q in {16, 32, 64, 128, 256, 1024}, 'min' and 'max', weights [Q, D] with one row per query.

Every point is timed against the grouped per-query route (SKYEMB_TOPK_PREFILTER=0) on the same bank in the same build; those kernels
are the parent commit's, so that is the parent's time.  The two-stage time INCLUDES the query preparation and the first-threshold
sample; the one-off build of the image [x ; x o x] (``ops.token_mse_pq_image``: it depends on neither the weights nor the queries)
is reported separately, per dtype.  The two routes alternate inside one process, call by call; every call is timed by a host clock
around a device synchronise, one warm-up call per route and shape first; the table holds the median and all repeats.

``TOKEN_MSE_PQ_PREFILTER_MIN_Q`` (sky_embeddings_amd/search.py) is the smallest Q of the grid from which the two-stage route is at
least 10 % faster at every larger point too, both combines, both dtypes -- in BOTH of two runs of this tool -- or 1024 when it wins
nowhere.

    python tools/bench_mse_per_query.py --out profiles/mse_per_query_crossover.json
    python tools/bench_mse_per_query.py --out profiles/mse_per_query_crossover_repeat.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sky_embeddings_amd import ops, search  # noqa: E402

GRID = (16, 32, 64, 128, 256, 1024)
MARGIN = 0.10


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def smallest_q(rows):
    wins = [Q for Q in GRID if all(r["two_stage_ms"] <= (1.0 - MARGIN) * r["grouped_ms"] for r in rows if r["Q"] >= Q)]
    return min(wins) if wins else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=15625)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtypes", default="float16,bfloat16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    N, P, D, k = a.images, a.tokens, a.dim, a.k
    for name in ("TOKEN_MSE_PQ_PREFILTER_MIN_Q", "TOKEN_MSE_PREFILTER_MIN_Q_SMALL"):
        setattr(search, name, 1)                                  # the route under test decides by the switch alone
    rows, image_ms = [], {}
    for dtype in a.dtypes.split(","):
        g = torch.Generator(device="cuda").manual_seed(0)
        # embedding-like rows: standardised features, tokens of an image share a direction
        bank = (torch.randn(N, 1, D, device="cuda", generator=g) + 0.7 * torch.randn(N, P, D, device="cuda", generator=g)).to(getattr(torch, dtype))
        tb = search.TokenBank.resident(bank)
        timed(lambda: ops.token_mse_pq_image(bank))               # warm-up: the first launch of the kernel
        builds = [timed(lambda: ops.token_mse_pq_image(bank))[0] for _ in range(a.reps)]
        image_ms[dtype] = dict(median=statistics.median(builds), all=builds, bytes=4 * N * P * D)
        tb.prepare_mse_per_query()
        for combine in ("min", "max"):
            for Q in GRID:
                idx = torch.randint(0, N, (Q,), device="cuda", generator=g)
                q = (bank[idx, 0].float() + 0.3 * torch.randn(Q, D, device="cuda", generator=g)).contiguous()   # targets near bank tokens
                # one weight row per target, as the inverse variance of a target group would give: positive, a decade of spread
                w = torch.exp(2.3 * torch.rand(Q, D, device="cuda", generator=g)).contiguous()

                def grouped():
                    os.environ["SKYEMB_TOPK_PREFILTER"] = "0"
                    st = {}
                    out = search.distance_topk_tokens(q, tb, k, "MSE", combine, weights=w, stats=st)
                    assert st["path"] == "tokens" and st["per_query_weights"]
                    return out, st

                def two_stage():
                    os.environ["SKYEMB_TOPK_PREFILTER"] = "1"
                    st = {}
                    out = search.distance_topk_tokens(q, tb, k, "MSE", combine, weights=w, stats=st)
                    assert st["path"] == "prefiltered" and st["per_query_weights"], st
                    return out, st

                ref, sg = timed(grouped)[1]
                got, st = timed(two_stage)[1]
                same = bool(torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]))
                tg, tn = [], []
                for _ in range(a.reps):
                    tg.append(timed(grouped)[0])
                    tn.append(timed(two_stage)[0])
                row = dict(dtype=dtype, combine=combine, Q=Q, group=sg["group"], grouped_ms=statistics.median(tg),
                           two_stage_ms=statistics.median(tn), grouped_ms_all=tg, two_stage_ms_all=tn, redone=st["redone"], bit_equal=same)
                row["speedup"] = row["grouped_ms"] / row["two_stage_ms"]
                rows.append(row)
                print(json.dumps({kk: row[kk] for kk in ("dtype", "combine", "Q", "grouped_ms", "two_stage_ms", "speedup", "redone", "bit_equal")}),
                      flush=True)
        del tb, bank
        torch.cuda.empty_cache()
    min_q = smallest_q(rows)
    result = dict(shape=dict(N=N, P=P, D=D, k=k, dtypes=a.dtypes.split(",")), reps=a.reps, margin=MARGIN, device=torch.cuda.get_device_name(0),
                  rows=rows, image_build_ms=image_ms, constants=dict(TOKEN_MSE_PQ_PREFILTER_MIN_Q=min_q),
                  note="two_stage_ms includes prepare_distance_weights, the query images and the first-threshold sample; the image "
                       "[x ; x o x] is built once per bank (image_build_ms) and is not part of it")
    print(json.dumps(dict(image_build_ms={d: v["median"] for d, v in image_ms.items()}, constants=result["constants"])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
