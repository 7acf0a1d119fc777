#!/usr/bin/env python3
"""Patch-token bank search: the fused pass (search.cosine_topk_tokens) against the best the one-vector API offers for the same
answer (search.cosine_scores over the token rows in chunks the streaming score kernel takes, then torch amin + topk), and the
one-vector streaming top-k over a bank of the same byte size.  HIP-event timing, the variants interleaved in one process.

usage: python tools/token_search_bench.py [--images 250000] [--tokens 16] [--dim 768] [--k 100] [--iters 10] [--out FILE]
                                         [--bank-dtype f32 | f16 | bf16 | a comma list, e.g. f32,f16,bf16]
                                         [--combine min | mean | max | a comma list] [--top-t T | a comma list, e.g. 4,16]
                                         [--select-frac F | a comma list, e.g. 1.0,0.5,0.1] [--select-pattern random | runs]
                                         [--fused-only] [--metric MAE | MSE | a comma list] [--many-query Q | a comma list] [--select]
--many-query: for every listed Q and every listed 16-bit bank type, interleaved in the same rounds, the grouped route
(grouped[f16]: search.cosine_topk_tokens over a plain TokenBank, ceil(Q / 16) passes) and the two-stage route (two_stage[f16]: the
same call over TokenBank.resident with search.TOKEN_PREFILTER_MIN_Q set to 17), combine as --combine; "redone" is the two-stage
call's count of re-run queries, "equal" whether both returned the same bits.  Nothing else runs in this mode.
--select (with --many-query): besides the unselected pair, both routes under four selections of images, all interleaved in the same
rounds -- all True (sel_all: the cost of the mask), 50 % and 10 % Bernoulli per image (sel_0.5, sel_0.1) and 10 % in runs of whole
256-row tiles (sel_0.1_runs: a tile's 256 / tokens images selected together with probability 0.1).  Each Selection is packed and
its per-bank state built once, outside the timed region; a leg reports "selected" and "tiles" = (live tiles, all tiles).
--bank-dtype: element type(s) of the resident token bank the fused pass runs on (16-bit banks: the fp32 bank rounded to nearest);
the fused variants of every listed type run interleaved in the same rounds, named fused_tokens[f16] etc.; the comparison variants
(baseline and one-vector) need the fp32 bank and run when f32 is listed.
--top-t: for every listed T and every listed bank type the fused pass with top_t=T (fused_tokens_top4 etc.: only the T best
token scores of an image count) and, with f32 listed, the unfused route to the same result (unfused_top4: cosine_scores over the
token rows, torch.topk over the P scores of every image, the reduce, torch.topk), in the same interleaved rounds.
"fused_equals_baseline" compares the fused result with the baseline's torch.topk, whose order among equal scores is unspecified:
False may come from exact ties alone and is not by itself a mismatch (the tests compare against the CPU restatement).
--select-frac: for every listed fraction F and every listed bank type, in the same interleaved rounds, the fused pass under a
selection of about F x images (fused_tokens_sel0.5 etc.: search.cosine_topk_tokens(select=), the Selection packed once outside the
timed region) and the plain fused pass over a PRE-COMPACTED bank of the same selected images (fused_tokens_compact0.5: what the
caller would run after bank[sel].contiguous(); the copy is not in that figure and is timed once on its own as "compact_ms", with
the norms of the copy in "compact_norms_ms"; at F = 1.0 also fused_tokens_sel1_no_floor, against fused_tokens_no_floor the cost
of the kernel's switch alone).  --select-pattern random: Bernoulli(F) per image, fixed seed; runs: runs of 64
images, a run selected with probability F.  "bank_bytes" of a _sel leg counts the selected images only (the bytes the kernel has
to read when P is a multiple of 16); "equals_compact" says whether the two legs returned the same lists (indices mapped back).
--fused-only leaves out the comparison variants (baseline, one-vector): memory for the compacted banks.
--metric: for every listed distance metric and every listed bank type, in the same interleaved rounds, the fused distance pass
(fused_distance[MAE] etc.: search.distance_topk_tokens, combine as --combine, with its pruning floor; fused_distance_no_floor[MAE]
without) and, with f32 listed and no --fused-only, the torch formula on the same resident bank (torch_distance[MAE]:
utils.similarity.weighted_MAE / weighted_MSE per query over slabs of images -- the elementwise temporaries of the whole bank would
not fit next to it --, the reduce over the P tokens, torch.topk(largest=False)).  "fused_equals_baseline" of these legs compares
indices exactly and distances to 1e-5 relative (torch's summation order differs from the contract's).
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


def metrics(text):
    names = [t.strip() for t in text.split(",") if t.strip()]
    if not names or any(n not in ("MAE", "MSE") for n in names):
        raise argparse.ArgumentTypeError(f"expected MAE, MSE or a comma list of them, got {text!r}")
    return names


def float_list(text):
    try:
        vals = [float(t) for t in text.split(",") if t.strip()]
    except ValueError:
        vals = []
    if not vals or min(vals) <= 0 or max(vals) > 1:
        raise argparse.ArgumentTypeError(f"expected a fraction in (0, 1] or a comma list of them, got {text!r}")
    return vals


def selection_flags(N, frac, pattern):
    g = torch.Generator(device="cuda").manual_seed(int(frac * 1000) + 31)
    if pattern == "random":
        return torch.rand(N, device="cuda", generator=g) < frac
    runs = torch.rand((N + 63) // 64, device="cuda", generator=g) < frac
    return runs.repeat_interleave(64)[:N].contiguous()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def many_query_selections(N, P):
    """--select: name -> Selection (None: the unselected pair)."""
    g = torch.Generator(device="cuda").manual_seed(97)
    per_tile = max(1, 256 // P)
    runs = torch.rand((N + per_tile - 1) // per_tile, device="cuda", generator=g) < 0.1
    flags = {"sel_all": torch.ones(N, device="cuda", dtype=torch.bool),
             "sel_0.5": torch.rand(N, device="cuda", generator=g) < 0.5,
             "sel_0.1": torch.rand(N, device="cuda", generator=g) < 0.1,
             "sel_0.1_runs": runs.repeat_interleave(per_tile)[:N].contiguous()}
    return dict({"": None}, **{name: search.Selection(f) for name, f in flags.items()})


def many_query(a, lp_banks, w):
    """--many-query: grouped against two-stage over the same resident 16-bit banks; --select: under selections too."""
    search.TOKEN_PREFILTER_MIN_Q = 17
    N, P, D, k = a.images, a.tokens, a.dim, a.k
    resident = {name: search.TokenBank.resident(tb.bank, w) for name, tb in lp_banks.items()}
    sels = many_query_selections(N, P) if a.select else {"": None}
    results = []
    for Q in a.many_query:
        q = torch.randn(Q, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2025 + Q))
        variants, info = {}, {}
        for combine in a.combine:
            for (name, tb), (sname, sel) in ((b, s) for b in lp_banks.items() for s in sels.items()):
                tag = f"[{name}]" + ("" if len(a.combine) == 1 else f"/{combine}") + (f"/{sname}" if sname else "")
                variants["grouped" + tag] = lambda tb=tb, c=combine, sel=sel: search.cosine_topk_tokens(q, tb, k, c, select=sel)
                variants["two_stage" + tag] = lambda rb=resident[name], c=combine, sel=sel: search.cosine_topk_tokens(q, rb, k, c, select=sel)
                st = {}
                (gs, gi), (ts_, ti) = variants["grouped" + tag](), search.cosine_topk_tokens(q, resident[name], k, combine, stats=st, select=sel)
                info["two_stage" + tag] = dict(path=st.get("path"), redone=st.get("redone"),
                                               equal=bool(torch.equal(gs, ts_)) and bool(torch.equal(gi, ti)))
                info["grouped" + tag] = dict(path="tokens")
                if sel is not None:
                    for v in ("grouped", "two_stage"):
                        info[v + tag].update(selected=sel.count, tiles=st.get("tiles"))
        times = {name: [] for name in variants}
        for it in range(a.warmup + a.iters):
            for name, fn in variants.items():                # interleaved: every variant once per round
                _, ms = timed(fn)
                if it >= a.warmup:
                    times[name].append(ms)
        for name, ts in times.items():
            ts = sorted(ts)
            results.append(dict(Q=Q, images=N, tokens=P, dim=D, k=k, variant=name, ms_median=round(ts[len(ts) // 2], 4),
                                ms_min=round(ts[0], 4), ms_max=round(ts[-1], 4), iters=len(ts), **info[name]))
            print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


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
    ap.add_argument("--select-frac", type=float_list, default=[])
    ap.add_argument("--select-pattern", choices=("random", "runs"), default="random")
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--metric", type=metrics, default=[])
    ap.add_argument("--many-query", type=int_list, default=[])
    ap.add_argument("--select", action="store_true")
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
    if a.many_query:
        return many_query(a, lp_banks, w)
    chunk = (1 << 20) // P * P                              # rows per cosine_scores call (streaming score kernel: <= 2^20 rows)
    if with_f32:
        tb = search.TokenBank(bank, w)
        if not a.fused_only:
            pb = search.PreparedBank(rows, w)               # the same bytes as a one-vector bank of N * P rows
            chunks = [search.PreparedBank(rows[s:s + chunk], w) for s in range(0, N * P, chunk)]
    else:
        del bank, rows
    # selections: packed once; the compacted twin of every bank (the copy and its norms timed once, outside the rounds)
    banks = dict(lp_banks, **({"f32": tb} if with_f32 else {}))
    sels, compact, extra = {}, {}, {}
    for frac in a.select_frac:
        flags = selection_flags(N, frac, a.select_pattern)
        sels[frac] = search.Selection(flags)
        for name, b in banks.items():
            cb, ms_copy = timed(lambda: b.bank[flags].contiguous())
            ctb, ms_norms = timed(lambda: search.TokenBank(cb, w))
            compact[frac, name] = ctb
            extra[frac, name] = dict(selected=sels[frac].count, compact_ms=round(ms_copy, 4), compact_norms_ms=round(ms_norms, 4))
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

        def torch_distance(metric, combine):
            from sky_embeddings_amd.utils.similarity import weighted_MAE, weighted_MSE
            fn = weighted_MAE if metric == "MAE" else weighted_MSE
            slab = max(1, (1 << 27) // (P * D))             # images per slab: 512 MiB of fp32 temporaries per elementwise step
            parts = []
            for s in range(0, N, slab):
                d = torch.stack([fn(q[j], bank[s:s + slab], w) for j in range(Q)])      # [Q, slab, P]
                parts.append(reducers[combine](d, dim=2))
            return torch.topk(torch.cat(parts, dim=1), k, dim=1, largest=False)

        variants, nbytes, same, combine_of, more = {}, {}, {}, {}, {}
        for combine in a.combine:
            tag = "" if len(a.combine) == 1 else f"/{combine}"
            mine = {}
            if with_f32:
                if not a.fused_only:
                    mine["baseline_scores_amin_topk"] = lambda c=combine: baseline(c)
                mine["fused_tokens"] = lambda c=combine: search.cosine_topk_tokens(q, tb, k, c)
                mine["fused_tokens_no_floor"] = lambda c=combine: search.cosine_topk_tokens(q, tb, k, c, prune=False)
                if combine == a.combine[0] and not a.fused_only:
                    mine["one_vector_stream_same_bytes"] = lambda: search.cosine_topk(q, pb, k)
                    mine["one_vector_stream_no_floor"] = lambda: search.cosine_topk(q, pb, k, prune=False)
                for t in a.top_t:
                    if not a.fused_only:
                        mine[f"unfused_top{t}"] = lambda c=combine, t=t: baseline(c, t)
                    mine[f"fused_tokens_top{t}"] = lambda c=combine, t=t: search.cosine_topk_tokens(q, tb, k, c, top_t=t)
                if not a.fused_only:
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
            for (frac, name), ctb in compact.items():
                sfx = "" if name == "f32" else f"[{name}]"
                b, sel = banks[name], sels[frac]
                pair = {f"fused_tokens_sel{frac:g}{sfx}": lambda b=b, sel=sel, c=combine: search.cosine_topk_tokens(q, b, k, c, select=sel),
                        f"fused_tokens_compact{frac:g}{sfx}": lambda ctb=ctb, c=combine: search.cosine_topk_tokens(q, ctb, k, c)}
                if frac == 1.0:                              # the switch alone: all ones, no floor, against fused_tokens_no_floor
                    pair[f"fused_tokens_sel1_no_floor{sfx}"] = lambda b=b, sel=sel, c=combine: search.cosine_topk_tokens(q, b, k, c, prune=False, select=sel)
                (ss, si), (cs, ci) = (fn() for fn in list(pair.values())[:2])
                back = torch.where(ci >= 0, sel.indices()[ci.clamp(min=0)], ci)
                for v in pair:
                    nbytes[v + tag] = sel.count * P * D * b.bank.element_size()
                    more[v + tag] = dict(extra[frac, name], equals_compact=bool(torch.equal(ss, cs)) and bool(torch.equal(si, back)))
                mine.update(pair)
            for metric in a.metric:
                for name, b in banks.items():
                    sfx = f"[{metric}]" if name == "f32" else f"[{metric},{name}]"
                    pair = {f"fused_distance{sfx}": lambda b=b, m=metric, c=combine: search.distance_topk_tokens(q, b, k, m, c),
                            f"fused_distance_no_floor{sfx}": lambda b=b, m=metric, c=combine: search.distance_topk_tokens(q, b, k, m, c, prune=False)}
                    for v in pair:
                        nbytes[v + tag] = elems * b.bank.element_size()
                    mine.update(pair)
                if with_f32 and not a.fused_only:
                    mine[f"torch_distance[{metric}]"] = lambda m=metric, c=combine: torch_distance(m, c)
                    (ts_, ti_), (fs_, fi_) = torch_distance(metric, combine), search.distance_topk_tokens(q, tb, k, metric, combine)
                    agree = bool(torch.equal(fi_, ti_)) and bool(torch.allclose(fs_, ts_, rtol=1e-5, atol=0))
                    for v in (f"fused_distance[{metric}]", f"fused_distance_no_floor[{metric}]", f"torch_distance[{metric}]"):
                        more[v + tag] = dict(more.get(v + tag, {}), fused_equals_baseline=agree)
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
                                **dict(dict(fused_equals_baseline=same.get(combine_of[name])), **more.get(name, {}))))
            print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
