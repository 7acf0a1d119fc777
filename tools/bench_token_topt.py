"""Many-query 'min' combine under top_t over a resident token bank: the two-stage route against the grouped route (forced by
SKYEMB_TOPK_PREFILTER=0), interleaved in one process; the plain-'min' two-stage search at the same shape prices the counting fold
against the AND fold; one leg under a random selection of the images.

  python tools/bench_token_topt.py [--images 250000 --tokens 16 --dim 768 --k 100 --top-t 2,4,8,15 --queries 64,256,1024,10000
                                    --select 0.1 --select-top-t 4 --reps 5 --out FILE]

Timing: every route is warmed once (row constants, bootstrap sample and the selection's state are built then, as in repeated use),
then timed `reps` times in alternation by CUDA events around the whole public call (it ends in a host read of the redo flags, so
the event pair spans everything).  Reported per leg: median and spread (max - min) in milliseconds of both routes, `redone`, that
the two results are equal, and the candidates of stage 1 -- read from one extra, untimed library call over a workspace pre-filled
with a marker: every slice writes a query's candidates from slot 0 on, so the marked-over slots per query are the candidates of its
FULLEST slice (mean and max over the queries), a lower bound of all it re-scored.  The bank is embedding-like: unit-variance tokens
around a per-image centre, so images have a direction."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sky_embeddings_amd import ops, search  # noqa: E402

MARK = 0xA5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def fullest_slice(q, tb, k, t, eps=1e-6):
    """(mean, max) over the queries of the candidates of each query's fullest slice, by one library call (no selection)."""
    rq = search._token_request("bench", q, tb, k, "min", search._COSINE, None, t if t else None, None)
    tw, qn = search.prepare_queries(q.float().contiguous(), tb.weights)
    thr0 = search._bootstrap_floor(rq, tw, qn, eps)
    Q, D = tw.shape
    ws = torch.full((ops.lib().skyemb_token_prefilter_ws_bytes(Q, D, k),), MARK, device=q.device, dtype=torch.uint8)
    out_s = torch.empty(Q, k, device=q.device)
    out_i = torch.empty(Q, k, device=q.device, dtype=torch.int64)
    redo = torch.empty(Q, device=q.device, dtype=torch.int32)
    tail, rowp = tb.stage1()
    ops.cosine_topk_tokens_prefiltered_top(tw, qn, tb.bank, tb.norms, tail, rowp, k, rq.combine, rq.top_t, eps, 0, out_s, out_i, redo, thr0, ws)
    lay = ops.token_prefilter_ws_layout(Q, D, k)
    cand = ws[lay["cand_i"]:lay["cand_i"] + Q * lay["cap"] * 4].view(torch.int32).view(Q, lay["cap"])
    marker = torch.tensor([MARK] * 4, dtype=torch.uint8).view(torch.int32).item()
    n = (cand != marker).sum(dim=1).float()
    return float(n.mean()), int(n.max()), lay["cap"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=250000)
    ap.add_argument("--tokens", type=int, default=16)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--top-t", default="2,4,8,15")
    ap.add_argument("--queries", default="64,256,1024,10000")
    ap.add_argument("--dtypes", default="f16,bf16")
    ap.add_argument("--select", type=float, default=0.1, help="share of images of the selected leg (0: no such leg)")
    ap.add_argument("--select-top-t", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, P, D, k = a.images, a.tokens, a.dim, a.k
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    saved = (search.TOKEN_TOPT_PREFILTER_MIN_Q, search.TOKEN_TOPT_PREFILTER_MIN_Q_SMALL, search.TOKEN_PREFILTER_MIN_Q)
    search.TOKEN_TOPT_PREFILTER_MIN_Q = search.TOKEN_TOPT_PREFILTER_MIN_Q_SMALL = search.TOKEN_PREFILTER_MIN_Q = 1
    for name in a.dtypes.split(","):
        dt = {"f16": torch.float16, "bf16": torch.bfloat16}[name]
        centre = torch.randn(N, 1, D, device=dev, generator=g)
        bank = torch.empty(N, P, D, device=dev, dtype=dt)
        for lo in range(0, N, 4096):                         # in pieces: no fp32 copy of the whole bank
            c = centre[lo:lo + 4096]
            bank[lo:lo + 4096] = (c + torch.randn(c.shape[0], P, D, device=dev, generator=g)).to(dt)
        del centre
        w = torch.rand(D, device=dev, generator=g) + 0.5
        tb = search.TokenBank.resident(bank, w)
        sel = search.Selection(torch.rand(N, device=dev, generator=g) < a.select) if a.select > 0 else None
        for Q in [int(v) for v in a.queries.split(",")]:
            pick = torch.randint(0, N, (Q,), device=dev, generator=g)
            q = bank[pick, 0].float() + 0.5 * torch.randn(Q, D, device=dev, generator=g)
            legs = [(int(t), None) for t in a.top_t.split(",")] + ([(a.select_top_t, sel)] if sel is not None else []) + [(0, None)]
            for t, s in legs:
                st_new, st_old = {}, {}
                kw = dict(top_t=t if t else None, select=s)

                def new():
                    os.environ.pop("SKYEMB_TOPK_PREFILTER", None)
                    return search.cosine_topk_tokens(q, tb, k, "min", stats=st_new, **kw)

                def old():
                    os.environ["SKYEMB_TOPK_PREFILTER"] = "0"
                    try:
                        return search.cosine_topk_tokens(q, tb, k, "min", stats=st_old, **kw)
                    finally:
                        os.environ.pop("SKYEMB_TOPK_PREFILTER", None)

                routes = (("new", new),) if t == 0 else (("new", new), ("old", old))     # the plain min: the two-stage time only
                tm = {"new": [], "old": []}
                res = {}
                for rep in range(a.reps + 1):
                    for key, fn in routes:
                        ms, out = timed(fn)
                        if rep >= 1:
                            tm[key].append(ms)
                        res[key] = out
                assert st_new["path"] == "prefiltered" and (t == 0 or st_old["path"] == "tokens"), (st_new, st_old)
                row = dict(dtype=name, N=N, P=P, D=D, k=k, Q=Q, top_t=t, selected=None if s is None else s.count, reps=a.reps,
                           two_stage_ms=statistics.median(tm["new"]), two_stage_spread_ms=max(tm["new"]) - min(tm["new"]),
                           redone=st_new["redone"])
                if t:
                    row.update(grouped_ms=statistics.median(tm["old"]), grouped_spread_ms=max(tm["old"]) - min(tm["old"]),
                               speedup=statistics.median(tm["old"]) / statistics.median(tm["new"]),
                               equal=bool(torch.equal(res["new"][0], res["old"][0]) and torch.equal(res["new"][1], res["old"][1])))
                if s is None:
                    mean_c, max_c, cap = fullest_slice(q, tb, k, t)
                    row.update(cand_fullest_slice_mean=mean_c, cand_fullest_slice_max=max_c, cap=cap)
                rows.append(row)
                print(json.dumps(row), flush=True)
        del tb, bank, sel
        torch.cuda.empty_cache()
    search.TOKEN_TOPT_PREFILTER_MIN_Q, search.TOKEN_TOPT_PREFILTER_MIN_Q_SMALL, search.TOKEN_PREFILTER_MIN_Q = saved
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/bench_token_topt.py", device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
