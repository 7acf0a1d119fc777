#!/usr/bin/env python
"""Where the two-stage weighted-MSE token route starts to pay under combine 'mean' (the opt-in route of ``distance_topk_tokens``:
``TokenBank.prepare_mse_mean``): two banks of 0.77e9 elements -- the project's measured one, N = 15 625 images x P = 64 tokens x
D = 768, and N = 250 000 x P = 4 x D = 768 (stage 1 skips only a factor P of the rows, so the advantage shrinks with P) --, k = 100,
fp16 and bf16, for Q in {16, 32, 64, 128, 256, 512, 1024}.

Every point is timed against the grouped route (SKYEMB_TOPK_PREFILTER=0) on the same bank in the same build; those kernels are the
parent commit's, so that is the parent's time.  The two-stage time INCLUDES the query preparation, the first-threshold sample and the
row-constants launch (``ops.token_mse_mean_rowp``: the bank's cached constants are dropped before every call); the one-off pooling
pass (``ops.token_mse_mean_pool``: it depends on neither the weights nor the queries) is reported separately, per bank and dtype.
The two routes alternate inside one process, call by call; every call is timed by a host clock around a device synchronise, one
warm-up call per route and shape first; the table holds the median and all repeats.

``TOKEN_MSE_MEAN_PREFILTER_MIN_Q`` (sky_embeddings_amd/search.py) is the smallest Q of the grid from which the two-stage route is at
least 10 % faster at every larger point too, on every bank and dtype -- in BOTH of two runs of this tool -- or 1024 when it wins
nowhere.

    python tools/bench_mse_mean.py --out profiles/mse_mean_crossover.json
    python tools/bench_mse_mean.py --out profiles/mse_mean_crossover_repeat.json
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

GRID = (16, 32, 64, 128, 256, 512, 1024)
BANKS = ((15625, 64), (250000, 4))
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
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtypes", default="float16,bfloat16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    D, k = a.dim, a.k
    for name in ("TOKEN_MSE_MEAN_PREFILTER_MIN_Q", "TOKEN_MSE_PREFILTER_MIN_Q_SMALL"):
        setattr(search, name, 1)                                  # the route under test decides by the switch alone
    rows, pool_ms = [], {}
    for N, P in BANKS:
        for dtype in a.dtypes.split(","):
            g = torch.Generator(device="cuda").manual_seed(0)
            # embedding-like rows: standardised features, tokens of an image share a direction (built in slices: no fp32 copy of the bank)
            bank = torch.empty(N, P, D, device="cuda", dtype=getattr(torch, dtype))
            for lo in range(0, N, 4096):
                n = min(4096, N - lo)
                bank[lo:lo + n] = (torch.randn(n, 1, D, device="cuda", generator=g) + 0.7 * torch.randn(n, P, D, device="cuda", generator=g)).to(bank.dtype)
            tb = search.TokenBank.resident(bank)
            timed(lambda: ops.token_mse_mean_pool(bank))          # warm-up: the first launch of the kernel
            builds = [timed(lambda: ops.token_mse_mean_pool(bank))[0] for _ in range(a.reps)]
            pool_ms[f"{N}x{P}/{dtype}"] = dict(median=statistics.median(builds), all=builds, bytes=2 * N * D + 8 * N)
            tb.prepare_mse_mean()
            for Q in GRID:
                idx = torch.randint(0, N, (Q,), device="cuda", generator=g)
                q = (bank[idx].float().mean(dim=1) + 0.3 * torch.randn(Q, D, device="cuda", generator=g)).contiguous()   # targets near images

                def grouped():
                    os.environ["SKYEMB_TOPK_PREFILTER"] = "0"
                    st = {}
                    out = search.distance_topk_tokens(q, tb, k, "MSE", "mean", stats=st)
                    assert st["path"] == "tokens"
                    return out, st

                def two_stage():
                    os.environ["SKYEMB_TOPK_PREFILTER"] = "1"
                    tb._stage1_mse_mean = None                    # the row-constants launch is part of the call
                    st = {}
                    out = search.distance_topk_tokens(q, tb, k, "MSE", "mean", stats=st)
                    assert st["path"] == "prefiltered" and st["combine"] == "mean", st
                    return out, st

                ref, _ = timed(grouped)[1]
                got, st = timed(two_stage)[1]
                same = bool(torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]))
                tg, tn = [], []
                for _ in range(a.reps):
                    tg.append(timed(grouped)[0])
                    tn.append(timed(two_stage)[0])
                row = dict(N=N, P=P, dtype=dtype, Q=Q, grouped_ms=statistics.median(tg), two_stage_ms=statistics.median(tn),
                           grouped_ms_all=tg, two_stage_ms_all=tn, redone=st["redone"], bit_equal=same)
                row["speedup"] = row["grouped_ms"] / row["two_stage_ms"]
                rows.append(row)
                print(json.dumps({kk: row[kk] for kk in ("N", "P", "dtype", "Q", "grouped_ms", "two_stage_ms", "speedup", "redone", "bit_equal")}),
                      flush=True)
            del tb, bank
            torch.cuda.empty_cache()
    per_leg = {f"{N}x{P}/{dt}": smallest_q([r for r in rows if (r["N"], r["dtype"]) == (N, dt)]) for N, P in BANKS for dt in a.dtypes.split(",")}
    min_q = smallest_q(rows)
    result = dict(shape=dict(banks=[dict(N=N, P=P) for N, P in BANKS], D=D, k=k, dtypes=a.dtypes.split(",")), reps=a.reps, margin=MARGIN,
                  device=torch.cuda.get_device_name(0), rows=rows, pool_ms=pool_ms, smallest_q_per_leg=per_leg,
                  constants=dict(TOKEN_MSE_MEAN_PREFILTER_MIN_Q=min_q),
                  note="two_stage_ms includes prepare_distance_weights, the query images, the first-threshold sample and the row-constants "
                       "launch; the pooled image is built once per bank (pool_ms) and is not part of it")
    print(json.dumps(dict(pool_ms={d: v["median"] for d, v in pool_ms.items()}, smallest_q_per_leg=per_leg, constants=result["constants"])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
