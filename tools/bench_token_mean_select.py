"""Many-query 'mean' combine under a selection of images over a resident token bank: the two-stage route over the compacted pooled
image (Selection.prepare_mean) against the grouped route (forced by SKYEMB_TOPK_PREFILTER=0), interleaved in one process.

  python tools/bench_token_mean_select.py [--shapes 15625x64,250000x16 --dim 768 --k 100 --queries 64,256,1024,10000
                                           --select 0.1,0.5 --dtypes f16,bf16 --reps 5 --out FILE]

Timing: the FIRST gather (Selection.prepare_mean: the bank's pooled image, if it is not there yet, and the compaction) is timed on
its own and reported per selection, never inside a search.  Then every route is warmed once (bootstrap sample, workspaces) and timed
`reps` times in alternation by HIP events around the whole public call (it ends in a host read of the redo flags, so the event pair
spans everything).  Reported per leg: median and spread (max - min) in milliseconds of both routes, `redone`, that the two results
are equal, and the live-tile counterfactual: the 256-row tiles of the pooled image that hold a selected image (what a live-tile
scheme would walk) against ceil(S / 256) (what the compacted image has).  The bank is embedding-like: unit-variance tokens around a
per-image centre, so images have a direction."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sky_embeddings_amd import search  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="15625x64,250000x16", help="images x tokens per image, comma separated")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", default="64,256,1024,10000")
    ap.add_argument("--dtypes", default="f16,bf16")
    ap.add_argument("--select", default="0.1,0.5", help="shares of the images selected at random")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    D, k = a.dim, a.k
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    saved = search.TOKEN_MEAN_SELECT_PREFILTER_MIN_Q
    search.TOKEN_MEAN_SELECT_PREFILTER_MIN_Q = 1
    for shape in a.shapes.split(","):
        N, P = (int(v) for v in shape.split("x"))
        for name in a.dtypes.split(","):
            dt = {"f16": torch.float16, "bf16": torch.bfloat16}[name]
            centre = torch.randn(N, 1, D, device=dev, generator=g)
            bank = torch.empty(N, P, D, device=dev, dtype=dt)
            step = max(1, 65536 // P)
            for lo in range(0, N, step):                         # in pieces: no fp32 copy of the whole bank
                c = centre[lo:lo + step]
                bank[lo:lo + step] = (c + torch.randn(c.shape[0], P, D, device=dev, generator=g)).to(dt)
            del centre
            w = torch.rand(D, device=dev, generator=g) + 0.5
            tb = search.TokenBank.resident(bank, w)
            pool_ms, _ = timed(tb.stage1_mean)                   # the bank's own pooled image: shared with the unselected search
            for share in [float(v) for v in a.select.split(",")]:
                sel = search.Selection(torch.rand(N, device=dev, generator=g) < share)
                if sel.count < 2048:                             # below the route's shape rule: the grouped route serves it, by rule
                    row = dict(dtype=name, N=N, P=P, D=D, k=k, share=share, selected=sel.count, refused="fewer than 2048 selected images")
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    continue
                gather_ms, _ = timed(lambda: sel.prepare_mean(tb))
                live = int(torch.unique(sel.indices() // 256).numel())
                for Q in [int(v) for v in a.queries.split(",")]:
                    pick = sel.indices()[torch.randint(0, sel.count, (Q,), device=dev, generator=g)]
                    q = bank[pick, 0].float() + 0.5 * torch.randn(Q, D, device=dev, generator=g)
                    st_new, st_old = {}, {}

                    def new():
                        os.environ.pop("SKYEMB_TOPK_PREFILTER", None)
                        return search.cosine_topk_tokens(q, tb, k, "mean", stats=st_new, select=sel)

                    def old():
                        os.environ["SKYEMB_TOPK_PREFILTER"] = "0"
                        try:
                            return search.cosine_topk_tokens(q, tb, k, "mean", stats=st_old, select=sel)
                        finally:
                            os.environ.pop("SKYEMB_TOPK_PREFILTER", None)

                    tm, res = {"new": [], "old": []}, {}
                    for rep in range(a.reps + 1):
                        for key, fn in (("new", new), ("old", old)):
                            ms, out = timed(fn)
                            if rep >= 1:
                                tm[key].append(ms)
                            res[key] = out
                    assert st_new["path"] == "prefiltered" and st_old["path"] == "tokens", (st_new, st_old)
                    med = {key: statistics.median(v) for key, v in tm.items()}
                    row = dict(dtype=name, N=N, P=P, D=D, k=k, Q=Q, share=share, selected=sel.count, reps=a.reps, pool_ms=pool_ms,
                               first_gather_ms=gather_ms, live_tiles_of_pooled=live, tiles_all=(N + 255) // 256,
                               tiles_compacted=(sel.count + 255) // 256, two_stage_ms=med["new"],
                               two_stage_spread_ms=max(tm["new"]) - min(tm["new"]), grouped_ms=med["old"],
                               grouped_spread_ms=max(tm["old"]) - min(tm["old"]), speedup=med["old"] / med["new"], redone=st_new["redone"],
                               equal=bool(torch.equal(res["new"][0], res["old"][0]) and torch.equal(res["new"][1], res["old"][1])))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del sel
            del tb, bank
            torch.cuda.empty_cache()
    search.TOKEN_MEAN_SELECT_PREFILTER_MIN_Q = saved
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/bench_token_mean_select.py", device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
