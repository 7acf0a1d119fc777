"""CPU: the float64 statements of tests/head_reference.py against sources already trusted (the reference goldens and
oracle/mae_oracle.py), so that the head-kernel tests cannot agree with a wrong yardstick."""
import numpy as np
import pytest
import torch

from oracle import mae_oracle as mo
from tests import head_reference as hr
from tests.helpers import load_simmim_case


@pytest.mark.parametrize("name,extra", [("simmim_tiny_F_l1_nan", 2), ("simmim_tiny_G_mse", 1), ("simmim_tiny_J_attnpool", 0)])
def test_pixel_loss_statement_reproduces_golden_loss(name, extra):
    z, cfg, _, imgs, pixel_mask, _ = load_simmim_case(name)
    pred = torch.from_numpy(z["pred"].copy())
    p, pooled = cfg.patch_size, name.endswith("attnpool")
    if pooled:     # the attention-pool head predicts the image itself
        arg = pred
    else:          # token rows behind `extra` cls / RA-Dec rows (junk: they must not take part)
        tok = hr.image_to_tokens(pred, p)
        arg = torch.cat([torch.full((tok.shape[0], extra, tok.shape[2]), 1e3, dtype=tok.dtype), tok], 1)
        assert torch.equal(hr.tokens_to_image(arg, cfg.in_chans, imgs.shape[2], imgs.shape[3], p, extra), pred)
    loss, dpred, _ = hr.simmim_pixel_loss(imgs, arg, pixel_mask, p, cfg.pixel_mean, cfg.pixel_std, cfg.norm_pix_loss,
                                          cfg.loss_fn != "mse", extra=extra, pooled=pooled)
    assert np.isnan(z["imgs"]).any() == name.endswith(("nan", "attnpool"))
    assert abs(float(loss) - float(z["loss"])) <= 2e-6 * abs(float(z["loss"])), (float(loss), float(z["loss"]))
    assert bool(torch.isfinite(dpred).all())
    if not pooled:
        assert bool((dpred[:, :extra] == 0).all())
    # ... and agrees with the oracle's own forward_loss (the float32 restatement the end-to-end tests rest on)
    ref = mo.forward_loss(mo.norm_inputs(imgs, cfg), pred, pixel_mask, cfg, nan_safe=True)
    assert abs(float(loss) - float(ref)) <= 2e-6 * abs(float(ref))


def test_spherical_harmonics_statement_reproduces_golden():
    z, cfg, state, _, _, ra_dec = load_simmim_case("simmim_tiny_H_radec")
    sh = hr.spherical_harmonics(ra_dec)
    ref = torch.from_numpy(z["sh_features"].copy()).double()
    assert float((sh - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    tok, _ = hr.radec_token(sh, state["ra_dec_embed.neural_network.layers.0.weight"],
                            state["ra_dec_embed.neural_network.layers.0.bias"],
                            state["ra_dec_embed.neural_network.last_layer.weight"],
                            state["ra_dec_embed.neural_network.last_layer.bias"])
    ref_tok = torch.from_numpy(z["ra_dec_token"].copy()).double()
    assert float((tok - ref_tok).abs().max()) <= 1e-5 * float(ref_tok.abs().max())
    # the oracle's closed form in float64 from float64 angles: the same function, off only by the fp32 angle
    assert float((sh - mo.spherical_harmonics(ra_dec.double())).abs().max()) <= 1e-5
    # the poles, where the Legendre factor sqrt((1 - x)(1 + x)) is 0: every m != 0 harmonic vanishes
    poles = hr.spherical_harmonics(torch.tensor([[0.0, 90.0], [359.999, -90.0]]))
    m_nonzero = [l * l + l + m for l in range(mo.SH_L) for m in range(-l, l + 1) if m != 0]
    assert float(poles[:, m_nonzero].abs().max()) < 1e-6
    assert bool(torch.isfinite(poles).all())


def test_attention_pool_core_matches_oracle():
    g = torch.Generator().manual_seed(5)
    B, N, D, H = 3, 11, 24, 2
    hd = D // H
    st = {"attn_pool.latent": torch.randn(1, 1, D, generator=g), "attn_pool.q.weight": torch.randn(D, D, generator=g) / 5,
          "attn_pool.q.bias": torch.randn(D, generator=g), "attn_pool.kv.weight": torch.randn(2 * D, D, generator=g) / 5,
          "attn_pool.kv.bias": torch.randn(2 * D, generator=g),
          # proj = identity and a zero last MLP layer: the block returns the pooled token o itself
          "attn_pool.proj.weight": torch.eye(D), "attn_pool.proj.bias": torch.zeros(D),
          "attn_pool.norm.weight": torch.ones(D), "attn_pool.norm.bias": torch.zeros(D),
          "attn_pool.mlp.fc1.weight": torch.randn(4 * D, D, generator=g), "attn_pool.mlp.fc1.bias": torch.zeros(4 * D),
          "attn_pool.mlp.fc2.weight": torch.zeros(D, 4 * D), "attn_pool.mlp.fc2.bias": torch.zeros(D)}
    st = {k: v.double() for k, v in st.items()}
    x = torch.randn(B, N, D, generator=g, dtype=torch.float64)
    ref = mo.attention_pool_latent(x, st, H, 1e-6)
    q = st["attn_pool.q.weight"] @ st["attn_pool.latent"].reshape(D) + st["attn_pool.q.bias"]
    kv = (x @ st["attn_pool.kv.weight"].T + st["attn_pool.kv.bias"]).reshape(B, N, 2, H, hd)
    o, prob = hr.attnpool_core(q.reshape(H, hd), kv[:, :, 0], kv[:, :, 1])
    assert float((o.reshape(B, D) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert torch.allclose(prob.sum(-1), torch.ones(B, H, dtype=torch.float64))
    # the gradient statement: the per-sample dq and dkv of the same forward
    dout = torch.randn(B, D, generator=g, dtype=torch.float64)
    out, prob2, dkv, dq, dq_mag = hr.attnpool_grads(q, kv, dout, H)
    assert bool((dq_mag >= dq.abs()).all())
    assert torch.equal(out, o.reshape(B, D)) and torch.equal(prob2, prob)
    ql = q.clone().requires_grad_(True)
    kvl = kv.clone().requires_grad_(True)
    o2, _ = hr.attnpool_core(ql.reshape(H, hd), kvl[:, :, 0], kvl[:, :, 1])
    (o2.reshape(B, D) * dout).sum().backward()
    assert torch.allclose(dq.sum(0), ql.grad, rtol=1e-12, atol=1e-14) and torch.allclose(dkv, kvl.grad, rtol=1e-12, atol=1e-14)
