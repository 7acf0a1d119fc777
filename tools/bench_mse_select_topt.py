#!/usr/bin/env python
"""Where the two-stage weighted-MSE token route starts to pay under ``top_t`` and under a selection of images (the opt-in routes of
``distance_topk_tokens``: ``TokenBank.prepare_mse_top_t``, ``Selection.prepare_mse``): the bank of tools/mse_prefilter_crossover.py
-- N = 15 625 images x P = 64 tokens x D = 768, k = 100, fp16 and bf16 -- for Q in {32, 64, 128, 256, 512, 1024}, on four legs:

    topt            top_t = 4 under 'max' (stage 1 counts passing rows, stage 2 sorts the token distances)
    select_scatter  a 10 % selection of images drawn at random ('min' and 'max')
    select_runs     a 10 % selection in runs of 4096 token rows (64 images; 'min' and 'max')
    select_topt     both selections with top_t = 4 under 'max'

Every leg is timed against the grouped route (SKYEMB_TOPK_PREFILTER=0) on the same bank, with the same top_t and selection.  The
two-stage time INCLUDES its preparation: the row-constants launch and, under a selection, the masked constants and live tiles (both
are dropped before every timed call).  The two routes alternate inside one process, call by call; every call is timed by a host clock
around a device synchronise, one warm-up call per route and shape first; the table holds the median and all repeats.

``TOKEN_MSE_TOPT_PREFILTER_MIN_Q``, ``TOKEN_MSE_SELECT_PREFILTER_MIN_Q`` and ``TOKEN_MSE_SELECT_TOPT_PREFILTER_MIN_Q``
(sky_embeddings_amd/search.py) are, per route, the smallest Q of the grid from which the two-stage route is at least 10 % faster on
every leg that exercises the route, both dtypes, or 1024 when it wins nowhere.

    python tools/bench_mse_select_topt.py --out profiles/mse_select_topt_crossover.json
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
# leg -> (the constant it decides, [(combine, top_t, selection kind)])
LEGS = {
    "topt": ("TOKEN_MSE_TOPT_PREFILTER_MIN_Q", [("max", 4, None)]),
    "select_scatter": ("TOKEN_MSE_SELECT_PREFILTER_MIN_Q", [("min", None, "scatter"), ("max", None, "scatter")]),
    "select_runs": ("TOKEN_MSE_SELECT_PREFILTER_MIN_Q", [("min", None, "runs"), ("max", None, "runs")]),
    "select_topt": ("TOKEN_MSE_SELECT_TOPT_PREFILTER_MIN_Q", [("max", 4, "scatter"), ("max", 4, "runs")]),
}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def selection_flags(kind, N, P, g):
    """10 % of the images: at random, or in runs of 4096 token rows at random run positions."""
    flags = torch.zeros(N, dtype=torch.bool, device="cuda")
    if kind == "scatter":
        flags[torch.randperm(N, device="cuda", generator=g)[:N // 10]] = True
    else:
        run = 4096 // P
        starts = torch.randperm(N // run, device="cuda", generator=g)[:N // 10 // run]
        for s in starts.tolist():
            flags[s * run:(s + 1) * run] = True
    return flags


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
    for name in ("TOKEN_MSE_PREFILTER_MIN_Q", "TOKEN_MSE_PREFILTER_MIN_Q_SMALL", "TOKEN_MSE_TOPT_PREFILTER_MIN_Q",
                 "TOKEN_MSE_SELECT_PREFILTER_MIN_Q", "TOKEN_MSE_SELECT_TOPT_PREFILTER_MIN_Q"):
        setattr(search, name, 1)                                  # the routes under test decide by the switch alone
    rows = []
    for dtype in a.dtypes.split(","):
        g = torch.Generator(device="cuda").manual_seed(0)
        # embedding-like rows: standardised features, tokens of an image share a direction
        bank = (torch.randn(N, 1, D, device="cuda", generator=g) + 0.7 * torch.randn(N, P, D, device="cuda", generator=g)).to(getattr(torch, dtype))
        w = torch.rand(D, device="cuda", generator=g) + 0.1
        tb = search.TokenBank.resident(bank, w).prepare_mse_top_t()
        sels = {kind: search.Selection(selection_flags(kind, N, P, g)).prepare_mse(tb) for kind in ("scatter", "runs")}
        for leg, (_, cases) in LEGS.items():
            for combine, top_t, kind in cases:
                sel = sels.get(kind)
                for Q in GRID:
                    idx = torch.randint(0, N, (Q,), device="cuda", generator=g)
                    q = (bank[idx, 0].float() + 0.3 * torch.randn(Q, D, device="cuda", generator=g)).contiguous()   # targets near bank tokens

                    def grouped():
                        os.environ["SKYEMB_TOPK_PREFILTER"] = "0"
                        st = {}
                        out = search.distance_topk_tokens(q, tb, k, "MSE", combine, stats=st, top_t=top_t, select=sel)
                        assert st["path"] == "tokens"
                        return out

                    def two_stage():
                        os.environ["SKYEMB_TOPK_PREFILTER"] = "1"
                        tb._stage1_mse = None                     # the preparation is part of the call: the row constants ...
                        if sel is not None:
                            sel._mse[tb] = None                   # ... and the selection's masked copy and live tiles
                        st = {}
                        out = search.distance_topk_tokens(q, tb, k, "MSE", combine, stats=st, top_t=top_t, select=sel)
                        assert st["path"] == "prefiltered", st
                        return out, st

                    ref = timed(grouped)[1]
                    (got, st) = timed(two_stage)[1]
                    same = bool(torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]))
                    tg, tn = [], []
                    for _ in range(a.reps):
                        tg.append(timed(grouped)[0])
                        tn.append(timed(two_stage)[0])
                    row = dict(leg=leg, dtype=dtype, combine=combine, top_t=top_t, selection=kind, Q=Q, grouped_ms=statistics.median(tg),
                               two_stage_ms=statistics.median(tn), grouped_ms_all=tg, two_stage_ms_all=tn, redone=st["redone"],
                               selected=st.get("selected"), tiles=st.get("tiles"), bit_equal=same)
                    row["speedup"] = row["grouped_ms"] / row["two_stage_ms"]
                    rows.append(row)
                    print(json.dumps({kk: row[kk] for kk in ("leg", "dtype", "combine", "selection", "Q", "grouped_ms", "two_stage_ms", "speedup",
                                                             "redone", "bit_equal")}), flush=True)
        del tb, sels, bank
        torch.cuda.empty_cache()
    by_leg = {leg: smallest_q([r for r in rows if r["leg"] == leg]) for leg in LEGS}
    constants = {}
    for leg, (name, _) in LEGS.items():
        qs = [by_leg[l2] for l2, (n2, _) in LEGS.items() if n2 == name]
        constants[name] = None if any(v is None for v in qs) else max(qs)
    result = dict(shape=dict(N=N, P=P, D=D, k=k, dtypes=a.dtypes.split(",")), reps=a.reps, margin=MARGIN, device=torch.cuda.get_device_name(0),
                  rows=rows, min_q_by_leg=by_leg, constants=constants,
                  note="two_stage_ms includes the row-constants launch (skyemb_token_mse_rowp) and, under a selection, "
                       "skyemb_token_prefilter_select_prepare with its read-back")
    print(json.dumps(dict(min_q_by_leg=by_leg, constants=constants)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
