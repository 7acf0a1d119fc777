"""Many-query 'mean' combine over a resident token bank: the two-stage route against the grouped route (forced by
SKYEMB_TOPK_PREFILTER=0), interleaved in one process, and the min-combine two-stage route at the same shape for reference.

  python tools/bench_token_mean.py [--images 15625 --tokens 64 --dim 768 --k 100 --queries 16,64,256,1024,10000 --reps 5 --out FILE]

Timing: both routes are warmed twice (pooled image, row constants and bootstrap sample are built then, as in repeated use), then
timed `reps` times in alternation by CUDA events around the whole public call (it ends in a host read of the redo flags, so the
event pair spans everything).  Reported per route: the median and the spread (max - min) in milliseconds, `redone`, and that the
two results are equal.  The bank is embedding-like: unit-variance tokens around a per-image centre, so images have a direction."""
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
    ap.add_argument("--images", type=int, default=15625)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", default="16,64,256,1024,10000")
    ap.add_argument("--dtypes", default="f16,bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, P, D, k = a.images, a.tokens, a.dim, a.k
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for name in a.dtypes.split(","):
        dt = {"f16": torch.float16, "bf16": torch.bfloat16}[name]
        centre = torch.randn(N, 1, D, device=dev, generator=g)
        bank = torch.empty(N, P, D, device=dev, dtype=dt)
        for lo in range(0, N, 1024):                         # in pieces: no fp32 copy of the whole bank
            c = centre[lo:lo + 1024]
            bank[lo:lo + 1024] = (c + torch.randn(c.shape[0], P, D, device=dev, generator=g)).to(dt)
        del centre
        w = torch.rand(D, device=dev, generator=g) + 0.5
        tb = search.TokenBank.resident(bank, w)
        for Q in [int(v) for v in a.queries.split(",")]:
            pick = torch.randint(0, N, (Q,), device=dev, generator=g)
            q = bank[pick, 0].float() + 0.5 * torch.randn(Q, D, device=dev, generator=g)
            saved = (search.TOKEN_MEAN_PREFILTER_MIN_Q, search.TOKEN_PREFILTER_MIN_Q)
            search.TOKEN_MEAN_PREFILTER_MIN_Q = search.TOKEN_PREFILTER_MIN_Q = 1
            st_new, st_old, st_min = {}, {}, {}

            def new():
                os.environ.pop("SKYEMB_TOPK_PREFILTER", None)
                return search.cosine_topk_tokens(q, tb, k, "mean", stats=st_new)

            def old():
                os.environ["SKYEMB_TOPK_PREFILTER"] = "0"
                try:
                    return search.cosine_topk_tokens(q, tb, k, "mean", stats=st_old)
                finally:
                    os.environ.pop("SKYEMB_TOPK_PREFILTER", None)

            def mn():
                return search.cosine_topk_tokens(q, tb, k, "min", stats=st_min)

            t = {"new": [], "old": [], "min": []}
            for rep in range(a.reps + 2):
                for key, fn in (("new", new), ("old", old), ("min", mn)):
                    ms, out = timed(fn)
                    if rep >= 2:
                        t[key].append(ms)
                    if key == "new":
                        r_new = out
                    elif key == "old":
                        r_old = out
            search.TOKEN_MEAN_PREFILTER_MIN_Q, search.TOKEN_PREFILTER_MIN_Q = saved
            assert st_new["path"] == "prefiltered" and st_old["path"] == "tokens", (st_new, st_old)
            row = dict(dtype=name, N=N, P=P, D=D, k=k, Q=Q, reps=a.reps,
                       two_stage_mean_ms=statistics.median(t["new"]), two_stage_mean_spread_ms=max(t["new"]) - min(t["new"]),
                       grouped_mean_ms=statistics.median(t["old"]), grouped_mean_spread_ms=max(t["old"]) - min(t["old"]),
                       two_stage_min_ms=statistics.median(t["min"]), two_stage_min_path=st_min["path"],
                       redone=st_new["redone"], redone_min=st_min.get("redone"),
                       equal=bool(torch.equal(r_new[0], r_old[0]) and torch.equal(r_new[1], r_old[1])))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del tb, bank
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/bench_token_mean.py", device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
