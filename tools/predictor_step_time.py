"""Times the downstream predictor's fine-tuning step of DESIGN.md section 7 with the per-tensor AdamW launches
(PredictorOptimizer(segmented=False)) and with one segmented launch per flat buffer (segmented=True), alternating in one process.

Configuration: ViT-B, img 64, patch 8, 5 channels, batch 128, `map` pooling, MSE, layer-wise lr decay (28 parameter groups).
Per round and mode: the mean of --steps whole steps (forward, loss, backward, optimiser, scheduler) after --warmup, between HIP
events; then the same for optimizer.step() alone on the gradients the last backward left.  Both modes run on ONE model: the step
is bit-identical between them, so they see the same weights.  Prints and writes one JSON document; fails without a GPU.

usage: python tools/predictor_step_time.py [--rounds 3] [--steps 20] [--warmup 5] [--dtype bf16|f16|f32] [--out FILE]
(SKYEMB_LIB selects a library built with another -DSKY_ADAMW_CHUNK: tools/build_variant.sh)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    from sky_embeddings_amd import ops
    from sky_embeddings_amd.model_config import config_for
    from sky_embeddings_amd.utils.vit import LinearLR, VisionTransformer, apply_onecycle_side_effects, build_optimizer

    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    cfg = config_for("base", img_size=64, patch_size=8, in_chans=5)
    model = VisionTransformer(cfg, "cuda", dtype, num_classes=1, global_pool="map", seed=0,
                              loss_scale="dynamic" if a.dtype == "f16" else None)
    model.train(True)
    opts = {}
    for segmented in (False, True):
        opt = build_optimizer(model, "ft", 1e-4, 0.05, 0.75, segmented=segmented)
        apply_onecycle_side_effects(opt, [g["lr"] for g in opt.param_groups])
        opts[segmented] = (opt, LinearLR(opt, start_factor=1.0, end_factor=0.1, total_iters=10 ** 6))
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(a.batch, 5, 64, 64, device="cuda", generator=gen)
    y = torch.randn(a.batch, 1, device="cuda", generator=gen)
    loss_fn = torch.nn.MSELoss()

    def whole_step(opt, sched):
        loss = loss_fn(model(x), y)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        sched.step()

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    rounds = {False: [], True: []}
    for r in range(a.rounds):
        for segmented in (False, True):
            opt, sched = opts[segmented]
            for _ in range(a.warmup):
                whole_step(opt, sched)
            torch.cuda.synchronize()
            step_ms = timed(lambda: whole_step(opt, sched), a.steps)
            for _ in range(a.warmup):
                opt.step()
            torch.cuda.synchronize()
            opt_ms = timed(opt.step, a.steps)
            rounds[segmented].append({"step_ms": step_ms, "optimizer_ms": opt_ms, "adamw_launches": opt.last_step_launches})
            print(f"round {r} segmented={segmented}: step {step_ms:.3f} ms, optimiser alone {opt_ms:.3f} ms, "
                  f"{opt.last_step_launches} AdamW launches", flush=True)

    def summary(rs):
        s = [r["step_ms"] for r in rs]
        o = [r["optimizer_ms"] for r in rs]
        return {"step_ms_mean": sum(s) / len(s), "step_ms_min": min(s), "step_ms_max": max(s), "optimizer_ms_mean": sum(o) / len(o),
                "optimizer_ms_min": min(o), "optimizer_ms_max": max(o), "adamw_launches": rs[-1]["adamw_launches"], "rounds": rs}
    per_tensor, segmented = summary(rounds[False]), summary(rounds[True])
    spread = per_tensor["step_ms_max"] - per_tensor["step_ms_min"]
    stepped = sum(opts[True][0]._buffers(n)[0][0].numel() for n in opts[True][0]._names())
    out = {"what": "ViT-B predictor fine-tuning step, img 64, patch 8, 5 channels, map pooling, MSE; HIP events",
           "device": torch.cuda.get_device_name(0), "dtype": a.dtype, "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
           "limits": dict(zip(("max_groups", "chunk_elems", "max_grid"), ops.adamw_segments_limits())),
           "library": os.path.basename(os.environ.get("SKYEMB_LIB") or "libskyemb.so"), "stepped_elements": stepped,
           "param_groups": len(opts[True][0].param_groups), "per_tensor": per_tensor, "segmented": segmented,
           "per_tensor_spread_ms": spread, "segmented_minus_per_tensor_ms": segmented["step_ms_mean"] - per_tensor["step_ms_mean"],
           "segmented_not_slower_than_spread": segmented["step_ms_mean"] - per_tensor["step_ms_mean"] <= spread,
           # bytes the optimiser moves per stepped element: p, g, m, v read, p, m, v written (fp32) + the shadow
           "segmented_optimizer_tb_s": stepped * (28 + (4 if a.dtype == "f32" else 2)) / (segmented["optimizer_ms_mean"] * 1e-3) / 1e12}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
