#!/usr/bin/env python3
"""Long-sequence attention on one MI355X: per-call forward / backward time of the streaming MFMA kernels
(csrc/attention_mfma.hip, N > 128) against torch.nn.functional.scaled_dot_product_attention in the same process, and the step
time of SimMIM ViT-B/8 on 5 x 128 x 128 cutouts (257 tokens) at B = 128, eager and graph.
Device-event timing after warm-up; the median of `reps` calls.  FLOPs counted from the shapes: 4 B H N^2 hd forward, 2.5x that
backward.  Peak: 2.5 PFLOP/s dense bf16 MFMA (spec).
usage: python tools/long_attention_bench.py [--reps 50] [--no-step] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sky_embeddings_amd import ops  # noqa: E402

PEAK = 2.5e15
SHAPES = [(128, 257, 12, 64), (128, 257, 16, 32), (32, 1025, 12, 64)]


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def attention_row(B, N, H, hd, reps):
    D = H * hd
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B, N, 3 * D, device="cuda", generator=g).bfloat16()
    dout = torch.randn(B, N, D, device="cuda", generator=g).bfloat16()
    out = torch.empty(B, N, D, device="cuda", dtype=torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    fwd = timed(lambda: ops.mha_fwd(qkv, out, B, N, H, hd), reps)
    bwd = timed(lambda: ops.mha_bwd(qkv, dout, dqkv, B, N, H, hd), reps)
    # SDPA on the same operands ([B, H, N, hd] views of qkv), forward and forward + backward through autograd
    t = qkv.view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = (t[i].detach().requires_grad_(True) for i in range(3))
    do = dout.view(B, N, H, hd).transpose(1, 2)
    s_fwd = timed(lambda: F.scaled_dot_product_attention(q, k, v), reps)

    def fb():
        o = F.scaled_dot_product_attention(q, k, v)
        torch.autograd.grad(o, (q, k, v), do)
    s_fb = timed(fb, reps)
    flop_f = 4.0 * B * H * N * N * hd
    row = dict(B=B, N=N, H=H, hd=hd, fwd_us=round(fwd, 1), bwd_us=round(bwd, 1), fwd_bwd_us=round(fwd + bwd, 1),
               fwd_tflops=round(flop_f / fwd / 1e6, 1), bwd_tflops=round(2.5 * flop_f / bwd / 1e6, 1),
               fwd_peak_share=round(flop_f / fwd / 1e-6 / PEAK, 4), bwd_peak_share=round(2.5 * flop_f / bwd / 1e-6 / PEAK, 4),
               sdpa_fwd_us=round(s_fwd, 1), sdpa_fwd_bwd_us=round(s_fb, 1),
               sdpa_backend=torch.backends.cuda.preferred_rocm_fa_library().name
               if hasattr(torch.backends.cuda, "preferred_rocm_fa_library") else "default")
    return row


def simmim_step(B, reps):
    from sky_embeddings_amd.model_config import config_for
    from sky_embeddings_amd.optim import CosineLR, FusedAdamW
    from sky_embeddings_amd.simmim_engine import SimMIMEngine
    from sky_embeddings_amd.train_step import TrainStep
    cfg = config_for("simmim", img_size=128, patch_size=8, in_chans=5, embed_dim=768, norm_pix_loss=True, loss_fn="L1")
    res = {}
    for graph in (False, True):
        eng = SimMIMEngine(cfg, device="cuda", compute_dtype=torch.bfloat16, seed=0)
        opt = FusedAdamW(eng, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05)
        step = TrainStep(eng, opt, CosineLR(opt, 1_000_000), B, use_graph=graph)
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, 5, 128, 128, device="cuda", generator=g).clamp_(min=-3.0)
        m = (torch.rand(B, 5, 16, 16, device="cuda", generator=g) < 0.45).float()
        m = m.repeat_interleave(8, 2).repeat_interleave(8, 3).contiguous()
        for _ in range(3):
            loss = step(x, m)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            loss = step(x, m)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        res["graph" if graph else "eager"] = dict(ms_per_step=round(dt * 1e3, 2), img_per_s=round(B / dt), loss=round(float(loss), 5))
        del step, opt, eng
        torch.cuda.empty_cache()
    return dict(model="SimMIM ViT-B/8, 5 x 128 x 128 (257 tokens), bf16", B=B, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "attention": []}
    for shp in SHAPES:
        row = attention_row(*shp, a.reps)
        print(json.dumps(row), flush=True)
        result["attention"].append(row)
    if not a.no_step:
        result["simmim_step"] = simmim_step(128, 10)
        print(json.dumps(result["simmim_step"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
