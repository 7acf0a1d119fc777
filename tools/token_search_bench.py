#!/usr/bin/env python3
"""Patch-token bank search: the fused pass (search.cosine_topk_tokens) against the best the one-vector API offers for the same
answer (search.cosine_scores over the token rows in chunks the streaming score kernel takes, then torch amin + topk), and the
one-vector streaming top-k over a bank of the same byte size.  HIP-event timing, the variants interleaved in one process.

usage: python tools/token_search_bench.py [--images 250000] [--tokens 16] [--dim 768] [--k 100] [--iters 10] [--out FILE]
                                         [--bank-dtype f32 | f16 | bf16 | a comma list, e.g. f32,f16,bf16]
                                         [--combine min | mean | max | a comma list] [--top-t T | a comma list, e.g. 4,16]
--bank-dtype: element type(s) of the resident token bank the fused pass runs on (16-bit banks: the fp32 bank rounded to nearest);
the fused variants of every listed type run interleaved in the same rounds, named fused_tokens[f16] etc.; the comparison variants
(baseline and one-vector) need the fp32 bank and run when f32 is listed.
--top-t: for every listed T and every listed bank type the fused pass with top_t=T (fused_tokens_top4 etc.: only the T best
token scores of an image count) and, with f32 listed, the unfused route to the same result (unfused_top4: cosine_scores over the
token rows, torch.topk over the P scores of every image, the reduce, torch.topk), in the same interleaved rounds.
"fused_equals_baseline" compares the fused result with the baseline's torch.topk, whose order among equal scores is unspecified:
False may come from exact ties alone and is not by itself a mismatch (the tests compare against the CPU restatement).
Bytes counted per pass: images x tokens x dim x element size (the bank; norms and lists are under 0.4 % of it).  Peak: 8.0 TB/s
(spec)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sky_embeddings_amd import search  # noqa: E402

HBM_PEAK = 8.0e12
BANK_DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def bank_dtypes(text):
    names = [t.strip() for t in text.split(",") if t.strip()]
    if not names or any(n not in BANK_DTYPES for n in names) or len(set(names)) != len(names):
        raise argparse.ArgumentTypeError(f"expected f32, f16, bf16 or a comma list of them, got {text!r}")
    return names


def int_list(text):
    try:
        vals = [int(t) for t in text.split(",") if t.strip()]
    except ValueError:
        vals = []
    if not vals or min(vals) < 1:
        raise argparse.ArgumentTypeError(f"expected a positive integer or a comma list of them, got {text!r}")
    return vals


def combines(text):
    names = [t.strip() for t in text.split(",") if t.strip()]
    if not names or any(n not in ("min", "mean", "max") for n in names):
        raise argparse.ArgumentTypeError(f"expected min, mean, max or a comma list of them, got {text!r}")
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=250_000)
    ap.add_argument("--tokens", type=int, default=16)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--combine", type=combines, default=["min"])
    ap.add_argument("--top-t", type=int_list, default=[])
    ap.add_argument("--out", default=None)
    ap.add_argument("--bank-dtype", type=bank_dtypes, default=["f32"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("token_search_bench.py needs a GPU")
    N, P, D, k = a.images, a.tokens, a.dim, a.k
    g = torch.Generator(device="cuda").manual_seed(2024)
    bank = torch.empty(N, P, D, device="cuda")
    for s in range(0, N, 5_000):
        bank[s:s + 5_000] = torch.randn(min(5_000, N - s), P, D, device="cuda", generator=g)
    w = 1.0 / (torch.rand(D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) + 0.5) ** 2
    w = w / w.sum()
    rows = bank.view(N * P, D)
    with_f32 = "f32" in a.bank_dtype
    lp_banks = {}
    for name in a.bank_dtype:
        if name != "f32":
            lp = torch.empty(N, P, D, device="cuda", dtype=BANK_DTYPES[name])
            for s in range(0, N, 5_000):
                lp[s:s + 5_000] = bank[s:s + 5_000]         # rounds to nearest-even
            lp_banks[name] = search.TokenBank(lp, w)
    chunk = (1 << 20) // P * P                              # rows per cosine_scores call (streaming score kernel: <= 2^20 rows)
    if with_f32:
        tb = search.TokenBank(bank, w)
        pb = search.PreparedBank(rows, w)                   # the same bytes as a one-vector bank of N * P rows
        chunks = [search.PreparedBank(rows[s:s + chunk], w) for s in range(0, N * P, chunk)]
    else:
        del bank, rows
    reducers = {"min": torch.amin, "max": torch.amax, "mean": torch.mean}
    elems = N * P * D
    results = []
    for Q in (1, 16):
        q = torch.randn(Q, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2025 + Q))

        def baseline(combine, top_t=None):
            parts = []
            for c in chunks:
                sc = search.cosine_scores(q, c).view(Q, -1, P)
                if top_t is not None:
                    sc = torch.topk(sc, top_t, dim=2).values
                parts.append(reducers[combine](sc, dim=2))
            return torch.topk(torch.cat(parts, dim=1), k, dim=1)

        variants, nbytes, same, combine_of = {}, {}, {}, {}
        for combine in a.combine:
            tag = "" if len(a.combine) == 1 else f"/{combine}"
            mine = {}
            if with_f32:
                mine = {
                    "baseline_scores_amin_topk": lambda c=combine: baseline(c),
                    "fused_tokens": lambda c=combine: search.cosine_topk_tokens(q, tb, k, c),
                    "fused_tokens_no_floor": lambda c=combine: search.cosine_topk_tokens(q, tb, k, c, prune=False),
                }
                if combine == a.combine[0]:
                    mine["one_vector_stream_same_bytes"] = lambda: search.cosine_topk(q, pb, k)
                    mine["one_vector_stream_no_floor"] = lambda: search.cosine_topk(q, pb, k, prune=False)
                for t in a.top_t:
                    mine[f"unfused_top{t}"] = lambda c=combine, t=t: baseline(c, t)
                    mine[f"fused_tokens_top{t}"] = lambda c=combine, t=t: search.cosine_topk_tokens(q, tb, k, c, top_t=t)
                bs, bi = baseline(combine)
                fs, fi = mine["fused_tokens"]()
                same[combine] = bool(torch.equal(fi, bi)) and bool(torch.equal(fs, bs))
            for name, lpb in lp_banks.items():
                lp = {f"fused_tokens[{name}]": lambda lpb=lpb, c=combine: search.cosine_topk_tokens(q, lpb, k, c),
                      f"fused_tokens_no_floor[{name}]": lambda lpb=lpb, c=combine: search.cosine_topk_tokens(q, lpb, k, c, prune=False)}
                for t in a.top_t:
                    lp[f"fused_tokens_top{t}[{name}]"] = lambda lpb=lpb, c=combine, t=t: search.cosine_topk_tokens(q, lpb, k, c, top_t=t)
                for v in lp:
                    nbytes[v + tag] = elems * lpb.bank.element_size()
                mine.update(lp)
            for v, fn in mine.items():
                variants[v + tag] = fn
                combine_of[v + tag] = combine
        times = {name: [] for name in variants}
        for it in range(a.warmup + a.iters):
            for name, fn in variants.items():                # interleaved: every variant once per round
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    times[name].append(e0.elapsed_time(e1))
        for name, ts in times.items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            nb = nbytes.get(name, elems * 4)
            results.append(dict(Q=Q, images=N, tokens=P, dim=D, k=k, combine=combine_of[name], variant=name, ms_median=round(med, 4),
                                ms_min=round(ts[0], 4), ms_max=round(ts[-1], 4), bank_bytes=nb,
                                tb_per_s=round(nb / (med * 1e-3) / 1e12, 3), hbm_peak_fraction=round(nb / (med * 1e-3) / HBM_PEAK, 4),
                                fused_equals_baseline=same.get(combine_of[name])))
            print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
