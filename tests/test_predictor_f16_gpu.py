"""GPU: the downstream predictor with a loss scale (utils.vit ``loss_scale=``) -- the mode that lets it run in fp16 -- against the
goldens of tests/golden/predictor.npz: opt-in, fp16 forward parity (held to bf16's measured error), the scale's transparency in
fp32 (the golden training bars of tests/test_predictor_gpu.py), fp16 gradients against fp32 (held to bf16's), a numeric overflow
that is skipped and recovered from, and a frozen-encoder run."""
import configparser
import os
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"lp_token_ce": ("lp", "token", "crossentropy"), "ft_avg_mse": ("ft", "avg", "mse"), "fs_token_mse": ("fs", "token", "mse"),
         "lp_map_ce": ("lp", "map", "crossentropy"), "ft_map_mse": ("ft", "map", "mse"),
         "lp_map_ce_oc": ("lp", "map", "crossentropy"), "ft_map_mse_oc": ("ft", "map", "mse")}


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "predictor.npz"))


def build(z, case, dtype, loss_scale=None):
    from sky_embeddings_amd.model_config import MAEConfig
    from sky_embeddings_amd.utils.mim_vit import _DataParallelShim
    from sky_embeddings_amd.utils.vit import VisionTransformer
    img, patch, C, D, depth, heads, ncls = [int(v) for v in z[f"{case}/cfg"]]
    cfg = MAEConfig(img_size=img, patch_size=patch, in_chans=C, embed_dim=D, depth=depth, num_heads=heads, decoder_embed_dim=16,
                    decoder_depth=1, decoder_num_heads=2, pixel_mean=0.1, pixel_std=1.7)
    m = VisionTransformer(cfg, "cuda", dtype, num_classes=ncls, global_pool=CASES[case][1],
                          label_means=z[f"{case}/label_means"].tolist(), label_stds=z[f"{case}/label_stds"].tolist(), loss_scale=loss_scale)
    pre = f"{case}/state/"
    m.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)})
    return _DataParallelShim(m), m


def optimiser(z, case, m):
    from sky_embeddings_amd.utils.vit import LinearLR, build_optimizer
    init_lr, wd, layer_decay, total, flf = [float(v) for v in z[f"{case}/hyper"]]
    opt = build_optimizer(m, CASES[case][0], init_lr, wd, layer_decay)
    return opt, LinearLR(opt, start_factor=1.0, end_factor=1 / flf, total_iters=int(total))


def optimiser_state(m):
    """Every parameter, shadow and Adam moment of the model (engine and head): the flat buffers, as integers (NaN-safe compare)."""
    out = {}
    for tag, st in (("engine", m.engine.store), ("head", m._head_mod.store)):
        for name in ("p", "m", "v", "p_lp"):
            buf = getattr(st, name)
            out[f"{tag}.{name}"] = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16).clone()
    return out


# ---- 1. opt-in -----------------------------------------------------------------------------------------------------------------------
def test_fp16_is_opt_in(z, monkeypatch, tmp_path):
    from sky_embeddings_amd.loss_scale import LossScaler
    from sky_embeddings_amd.utils.vit import build_model
    monkeypatch.delenv("SKYEMB_DTYPE", raising=False)
    with pytest.raises(NotImplementedError):
        build(z, "fs_token_mse", torch.float16)
    _, m = build(z, "fs_token_mse", torch.float16, loss_scale="dynamic")
    assert m.scaler.dynamic and m.scaler.scale == 2.0 ** 16 and m.engine.dtype == torch.float16
    assert m.engine.loss_scale == 1.0 and m.engine.plan_loss_scale(10 ** 6) == 1.0          # the scaler owns the factor
    _, m = build(z, "fs_token_mse", torch.float16, loss_scale=2 ** 12)
    assert not m.scaler.dynamic and m.scaler.scale == 4096.0
    mine = LossScaler(init_scale=2.0 ** 8, growth_interval=5)
    assert build(z, "fs_token_mse", torch.bfloat16, loss_scale=mine)[1].scaler is mine       # any compute dtype
    assert build(z, "fs_token_mse", torch.float32)[1].scaler is None
    with pytest.raises(ValueError):
        build(z, "fs_token_mse", torch.float16, loss_scale=1000)

    def configs(mae_dtype, **training):
        mae_cfg = configparser.ConfigParser()
        mae_cfg.read(os.path.join(ROOT, "configs", "mim_1.ini"))
        mae_cfg["TRAINING"]["compute_dtype"] = mae_dtype
        cfg = configparser.ConfigParser()
        cfg["ARCHITECTURE"] = {"img_size": "32", "global_pool": "token", "dropout": "0.0"}
        cfg["DATA"] = {"num_classes": "3", "label_means": "[0]", "label_stds": "[1]"}
        cfg["TRAINING"] = training
        return cfg, mae_cfg
    none = str(tmp_path / "none.pth.tar")
    for mae_dtype, training, want_dtype, want_scale in (
            ("bf16", {"loss_scale": "dynamic", "compute_dtype": "f16"}, torch.float16, ("dynamic", 2.0 ** 16)),
            ("f16", {"loss_scale": "1024"}, torch.float16, ("fixed", 1024.0)),          # compute_dtype falls back to the MAE ini
            ("f16", {"loss_scale": "dynamic", "compute_dtype": "bf16"}, torch.bfloat16, ("dynamic", 2.0 ** 16)),
            ("f16", {}, torch.bfloat16, None),                                          # no key: the fallback of before
            ("f32", {}, torch.float32, None)):
        model, _, _ = build_model(*configs(mae_dtype, **training), none, "None", torch.device("cuda"))
        mm = model.module
        assert mm.engine.dtype == want_dtype, (mae_dtype, training)
        if want_scale is None:
            assert mm.scaler is None
        else:
            assert ("dynamic" if mm.scaler.dynamic else "fixed", mm.scaler.scale) == want_scale


# ---- 2. forward ----------------------------------------------------------------------------------------------------------------------
def test_fp16_forward_matches_reference_no_worse_than_bf16(z):
    worst = {}
    for dtype, scale in ((torch.float16, "dynamic"), (torch.bfloat16, None)):
        errs = {}
        for case in CASES:
            model, m = build(z, case, dtype, loss_scale=scale)
            model.eval()
            out = model(torch.from_numpy(z[f"{case}/x"][0]).cuda()).cpu().numpy()
            ref = z[f"{case}/logits0"]
            errs[case] = float(np.abs(out - ref).max()) / max(float(np.abs(ref).max()), 1e-6)
        print(dtype, {k: f"{v:.3e}" for k, v in errs.items()})
        worst[dtype] = max(errs.values())
        if dtype == torch.float16:
            for case, err in errs.items():
                assert err < 3e-2, (case, err)
    print(f"forward relative error, worst of {len(CASES)} cases: fp16 {worst[torch.float16]:.3e}  bf16 {worst[torch.bfloat16]:.3e}")
    assert worst[torch.float16] <= worst[torch.bfloat16], worst


# ---- 3. the scale is transparent -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lp_map_ce", "ft_avg_mse", "fs_token_mse", "ft_map_mse"])
def test_fixed_scale_in_fp32_meets_the_golden_training_bars(z, case):
    from sky_embeddings_amd.utils.predictor_training_fns import run_iter
    method, pool, loss_fn = CASES[case]
    model, m = build(z, case, torch.float32, loss_scale=2 ** 10)
    opt, sched = optimiser(z, case, m)
    x, labels = torch.from_numpy(z[f"{case}/x"]), torch.from_numpy(z[f"{case}/labels"])
    cp = defaultdict(list)
    for it in range(3):
        model, opt, sched, cp = run_iter(model, x[it].cuda(), None, None, labels[it].cuda(), opt, sched, cp, loss_fn=loss_fn, mode="train")
        assert m._backward_scale == 1024.0
        assert abs(cp["train_loss"][-1] - float(z[f"{case}/train_loss"][it])) <= 5e-5 * abs(float(z[f"{case}/train_loss"][it])), (it, cp["train_loss"])
        if it in (0, 2):
            sd = m.state_dict()
            for k, v in sd.items():
                ref = z[f"{case}/step{it}/{k}"]
                lr_k = max(g["initial_lr"] for g in opt.param_groups if k in g["params"]) if any(k in g["params"] for g in opt.param_groups) else 0.0
                # (the bars of tests/test_predictor_gpu.py::test_predictor_training_steps_match_reference, key-bias carve-out included)
                tol = 5e-6 * max(float(np.abs(ref).max()), 1e-3) + 3e-2 * lr_k
                diff = np.abs(v.detach().cpu().numpy().reshape(ref.shape) - ref)
                if k.endswith("attn.qkv.bias") or k == "attn_pool.kv.bias":
                    D = ref.shape[0] // (3 if k.endswith("qkv.bias") else 2)
                    lo = D if k.endswith("qkv.bias") else 0            # [q | k | v] and [k | v]
                    assert float(diff[lo:lo + D].max()) <= 1.5 * (it + 1) * lr_k, (it, k)
                    diff = np.concatenate([diff[:lo], diff[lo + D:]])
                assert float(diff.max()) <= tol, (it, k, float(diff.max()), tol)
    assert m.scaler.skipped_steps == 0 and opt.step_count == 3 and m.scaler.scale == 1024.0
    assert m.scaler.last_absmax > 0.0 and np.isfinite(m.scaler.last_absmax)
    # the largest |gradient| the probe saw: the largest of the runs it read (the step leaves the gradients in place), scale divided out
    assert m.scaler.last_absmax == max(float(r.abs().max()) for r in opt._probe_ranges()) / 1024.0
    assert m.scaler.last_absmax >= max(float(m.unscaled_grad(k).abs().max()) for g in opt.param_groups for k in g["params"])
    assert sorted(opt.state_dict()["loss_scaler"]) == ["growth_tracker", "scale", "skipped_steps"]


# ---- 4. fp16 gradients ---------------------------------------------------------------------------------------------------------------
def first_backward_gradients(z, case, dtype, loss_scale):
    """d loss / d every trainable tensor after the first backward of `case` (no optimiser step), loss scale divided out.  With a
    dynamic scale the backward is repeated at the backed-off scale while the probe reports an overflow, as training would."""
    method, pool, loss_fn = CASES[case]
    model, m = build(z, case, dtype, loss_scale=loss_scale)
    opt, _ = optimiser(z, case, m)                       # (sets what is trainable)
    names = [n for g in opt.param_groups for n in g["params"]]
    x, labels = torch.from_numpy(z[f"{case}/x"][0]).cuda(), torch.from_numpy(z[f"{case}/labels"][0]).cuda()
    model.train(True)
    for _ in range(17):
        loss = torch.nn.MSELoss()(model(x), m.normalize_labels(labels))
        loss.backward()
        if m.scaler is None:
            break
        m.scaler.begin_step()
        for r in opt._probe_ranges():
            m.scaler.probe(r)
        if m.scaler.finish_step():
            break
    else:
        raise AssertionError("the gradients overflow at every scale")
    return {n: m.unscaled_grad(n).double().cpu() for n in names}, (m.scaler.state_dict() if m.scaler else None)


@pytest.mark.parametrize("case", ["ft_map_mse", "fs_token_mse"])
def test_fp16_gradients_no_worse_than_bf16(z, case):
    ref, _ = first_backward_gradients(z, case, torch.float32, None)
    norm = sum(float((v ** 2).sum()) for v in ref.values()) ** 0.5
    assert norm > 0
    err = {}
    for dtype, scale in ((torch.float16, "dynamic"), (torch.bfloat16, None)):
        got, sd = first_backward_gradients(z, case, dtype, scale)
        assert sorted(got) == sorted(ref) and all(bool(torch.isfinite(v).all()) for v in got.values())
        err[dtype] = sum(float(((got[k] - ref[k]) ** 2).sum()) for k in ref) ** 0.5 / norm
        print(case, dtype, f"global relative L2 of the gradients against fp32: {err[dtype]:.3e}", sd)
    assert err[torch.float16] <= err[torch.bfloat16], err


# ---- 5. overflow ---------------------------------------------------------------------------------------------------------------------
def test_overflow_is_skipped_and_recovered_from(z):
    from sky_embeddings_amd.loss_scale import LossScaler
    from sky_embeddings_amd.utils.predictor_training_fns import run_iter
    case = "fs_token_mse"
    model, m = build(z, case, torch.float16, loss_scale=LossScaler(growth_interval=2))
    opt, sched = optimiser(z, case, m)
    x, labels = torch.from_numpy(z[f"{case}/x"]), torch.from_numpy(z[f"{case}/labels"])
    huge = labels[0].clone()
    huge.view(-1)[0] = 1e38                        # d loss / d predictions x 2^16 is inf in fp32 already: numeric overflow, nothing else
    before = optimiser_state(m)
    lr0 = sched.get_last_lr()
    cp = defaultdict(list)
    run_iter(model, x[0].cuda(), None, None, huge.cuda(), opt, sched, cp, loss_fn="mse", mode="train")
    after = optimiser_state(m)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert opt.step_count == 0 and m.scaler.scale == 2.0 ** 15 and m.scaler.skipped_steps == 1 and m.scaler.growth_tracker == 0
    assert sched.last_epoch == 1 and sched.get_last_lr() != lr0          # the lr schedule moves on, as with torch's scaler
    assert opt.state_dict()["state"] == {}                              # nothing stepped yet
    for it in (1, 2):
        run_iter(model, x[it].cuda(), None, None, labels[it].cuda(), opt, sched, cp, loss_fn="mse", mode="train")
        assert opt.step_count == it and m.scaler.skipped_steps == 1
        assert np.isfinite(m.scaler.last_absmax) and m.scaler.last_absmax > 0.0
    assert np.isfinite(cp["train_loss"][1:]).all()
    final = optimiser_state(m)
    for tag, st in (("engine", m.engine.store), ("head", m._head_mod.store)):
        for name in ("p", "m", "v", "p_lp"):
            assert bool(torch.isfinite(getattr(st, name).float()).all()), (tag, name)
    assert not torch.equal(final["engine.p"], before["engine.p"]) and not torch.equal(final["head.p"], before["head.p"])
    assert m.scaler.scale == 2.0 ** 16 and m.scaler.growth_tracker == 0          # two good steps at growth_interval 2: doubled back
    # checkpoint and resume into a fresh model + optimiser: scale, tracker, step count continue
    run_iter(model, x[0].cuda(), None, None, labels[0].cuda(), opt, sched, cp, loss_fn="mse", mode="train")
    assert (opt.step_count, m.scaler.growth_tracker) == (3, 1)
    sd_o, sd_s, sd_m = opt.state_dict(), sched.state_dict(), {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert sd_o["loss_scaler"] == {"scale": 2.0 ** 16, "growth_tracker": 1, "skipped_steps": 1}
    model2, m2 = build(z, case, torch.float16, loss_scale=LossScaler(growth_interval=2))
    opt2, sched2 = optimiser(z, case, m2)
    m2.load_state_dict(sd_m)
    opt2.load_state_dict(sd_o)
    sched2.load_state_dict(sd_s)
    assert opt2.step_count == 3 and m2.scaler.state_dict() == m.scaler.state_dict()
    for mdl, o, s in ((model, opt, sched), (model2, opt2, sched2)):
        run_iter(mdl, x[1].cuda(), None, None, labels[1].cuda(), o, s, defaultdict(list), loss_fn="mse", mode="train")
    assert opt2.step_count == opt.step_count == 4
    assert m2.scaler.state_dict() == m.scaler.state_dict() == {"scale": 2.0 ** 17, "growth_tracker": 0, "skipped_steps": 1}
    a, b = optimiser_state(m), optimiser_state(m2)
    for k in a:
        assert torch.equal(a[k], b[k]), k              # the resumed run IS the original one


# ---- 6. frozen encoder ---------------------------------------------------------------------------------------------------------------
def test_fp16_linear_probe_with_attention_pool_runs(z):
    from sky_embeddings_amd.utils.predictor_training_fns import run_iter
    case = "lp_map_ce"
    model, m = build(z, case, torch.float16, loss_scale="dynamic")
    opt, sched = optimiser(z, case, m)
    assert m.frozen_encoder
    # the probe reads the stepped tensors only -- a few joined runs, not one per tensor, and nothing of the frozen encoder
    ranges = opt._probe_ranges()
    assert sum(r.numel() for r in ranges) == sum(opt._buffers(n)[0][1].numel() for n in opt._names())
    assert len(ranges) < len(opt._names()) / 2
    frozen = m.engine.store.param("blocks.0.attn.qkv.weight").clone()
    x, labels = torch.from_numpy(z[f"{case}/x"]), torch.from_numpy(z[f"{case}/labels"])
    cp = defaultdict(list)
    for it in range(3):
        run_iter(model, x[it].cuda(), None, None, labels[it].cuda(), opt, sched, cp, loss_fn="crossentropy", mode="train")
    assert np.isfinite(cp["train_loss"]).all() and len(cp["train_loss"]) == 3
    assert opt.step_count + m.scaler.skipped_steps == 3 and opt.step_count >= 1
    assert torch.equal(frozen, m.engine.store.param("blocks.0.attn.qkv.weight"))
    assert bool(torch.isfinite(m._head_mod.store.p).all())
