#!/usr/bin/env python3
"""One call of a two-stage search entry point (csrc/topk_prefilter.hip) per case of tests/prefilter_plan_cases.py, in case order,
in one process.  The launches of a call depend on its shape alone, so the operands are random.  Use, on any build of the library:

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/prefilter_launch_record.py
      every search call starts with query16_kernel; tests/golden/make_prefilter_launch_golden.py cuts the trace there, drops the
      preparation kernels and torch's own, and writes tests/golden/prefilter_launches.json or compares two traces.

SKYEMB_PREFILTER_LO is set per case (the library reads it on every call)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sky_embeddings_amd import ops  # noqa: E402
from tests import prefilter_plan_cases as pc  # noqa: E402

EPS = 1e-6


def floor_of(scores, k):
    """A valid floor [Q]: just below the k-th best of a sample's scores [Q, S]."""
    kth = scores.topk(k, dim=1).values[:, k - 1]
    return (kth - 1e-3 * kth.abs() - 1e-6).contiguous()


def run(c, dev):
    g = torch.Generator(device="cpu").manual_seed(len(c["id"]))
    Q, D, N, P, k = c["Q"], c["D"], c["N"], c["P"], c["k"]
    tw = torch.randn(Q, D, generator=g).to(dev)
    qn = tw.norm(dim=1).contiguous()
    rows = pc.stage1_rows(c) if c["kind"] != "mean" else N * P
    x = torch.randn(rows, D, generator=g).to(dev)
    dtype = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[c["bank"]]
    bank = x.to(dtype)
    xn = bank.float().norm(dim=1).contiguous()
    out_s = torch.empty(Q, k, device=dev)
    out_i = torch.empty(Q, k, device=dev, dtype=torch.int64)
    redo = torch.empty(Q, device=dev, dtype=torch.int32)
    S = 2048                                                     # sample rows of the floor
    sample = (tw @ bank[:S * (P if c["kind"] != "rows" else 1)].float().T) / (qn[:, None] * xn[None, :S * (P if c["kind"] != "rows" else 1)] + EPS)
    if c["lo"] is None:
        os.environ.pop("SKYEMB_PREFILTER_LO", None)
    else:
        os.environ["SKYEMB_PREFILTER_LO"] = c["lo"]
    words = None
    if c["dead"] is not None:
        flags = torch.from_numpy(pc.selection_flags(c)).to(torch.uint8).to(dev)
        words = torch.zeros((flags.shape[0] + 31) // 32, device=dev, dtype=torch.int32)
        ops.pack_select(flags, words)
    if c["kind"] == "rows":
        thr0 = floor_of(sample, k) if c["thr0"] else None
        if c["bank"] == "f32":
            bank16, rowp = ops.bank16_prepare(bank, xn)
            tail = None
        else:
            tail, rowp = ops.resident_rowp(bank, xn)
        torch.cuda.synchronize()
        if words is not None:
            prepared = ops.prefilter_select_prepare(words, N, rowp)
            assert prepared[2:] == pc.selection_info(c), (c["id"], prepared[2:])
            if c["bank"] == "f32":
                ops.cosine_topk_prefiltered_sel(tw, qn, bank, xn, bank16, None, prepared, k, EPS, 0, out_s, out_i, redo)
            else:
                ops.cosine_topk_prefiltered_sel(tw, qn, None, xn, bank, tail, prepared, k, EPS, 0, out_s, out_i, redo)
        elif c["bank"] == "f32":
            ops.cosine_topk_prefiltered(tw, qn, bank, xn, bank16, rowp, k, EPS, 0, out_s, out_i, redo, thr0=thr0)
        else:
            ops.cosine_topk_prefiltered_resident(tw, qn, bank, xn, tail, rowp, k, EPS, 0, out_s, out_i, redo, thr0=thr0)
    else:
        tokens = bank.view(N, P, D)
        per_image = sample.view(Q, -1, P)
        combined = {"min": per_image.min(dim=2).values, "max": per_image.max(dim=2).values, "mean": per_image.mean(dim=2)}[c["combine"]]
        if c["top_t"] and c["combine"] == "min":
            combined = per_image.sort(dim=2, descending=True).values[:, :, c["top_t"] - 1]
        thr0 = floor_of(combined, k) if c["thr0"] else None
        code = ops.COMBINE_CODES[c["combine"]]
        if c["kind"] == "mean":
            pooled, tail, rowp = ops.token_mean_pool(tokens, xn)
            ops.cosine_topk_tokens_mean_prefiltered(tw, qn, tokens, xn, pooled, tail, rowp, k, EPS, 0, out_s, out_i, redo, thr0=thr0)
        else:
            tail, rowp = ops.resident_rowp(bank, xn)
            if words is not None:
                prepared = ops.token_prefilter_select_prepare(words, N, P, rowp)
                assert tuple(prepared[2:4]) == pc.selection_info(c), (c["id"], prepared[2:4])
                ops.cosine_topk_tokens_prefiltered_top_sel(tw, qn, tokens, xn, tail, prepared, c["direct_sel"], k, code, c["top_t"], EPS, 0,
                                                           out_s, out_i, redo, thr0=thr0)
            else:
                ops.cosine_topk_tokens_prefiltered_top(tw, qn, tokens, xn, tail, rowp, k, code, c["top_t"], EPS, 0, out_s, out_i, redo,
                                                       thr0=thr0)
    torch.cuda.synchronize()


def main():
    ops.lib()
    dev = torch.device("cuda")
    for c in pc.CASES:
        run(c, dev)
    os.environ.pop("SKYEMB_PREFILTER_LO", None)
    print(f"prefilter_launch_record: {len(pc.CASES)} cases", file=sys.stderr)


if __name__ == "__main__":
    main()
