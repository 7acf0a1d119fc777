"""Float64 statements of the SimMIM / downstream-head operations (attention pool, SimMIM pixel loss, blended patch gather,
RA/Dec token), the yardsticks of tests/test_head_kernels_gpu.py.  tests/test_head_reference_cpu.py pins them against the
reference goldens and the oracle, so that a kernel test cannot agree with a wrong statement.

Every function takes CPU tensors and computes in float64 from whatever values it is given: the tests pass the operands the
kernel read (16-bit operands already rounded)."""
import math

import torch
import torch.nn.functional as F

from oracle import mae_oracle as mo


# ------------------------------------------------------------------------------------ attention pool
def attnpool_core(q, k, v):
    """timm AttentionPoolLatent's core with one query: q [H, hd] (shared by the batch) or [B, H, hd]; k, v [B, N, H, hd]
    -> (o [B, H, hd], prob [B, H, N]).  softmax(q k^T / sqrt(hd)) v."""
    hd = k.shape[-1]
    qb = q.expand(k.shape[0], -1, -1) if q.dim() == 2 else q
    s = torch.einsum("bhd,bnhd->bhn", qb, k) * hd ** -0.5
    prob = torch.softmax(s, dim=-1)
    return torch.einsum("bhn,bnhd->bhd", prob, v), prob


def attnpool_grads(q, kv, dout, H):
    """fp64 autograd of attnpool_core: q [D] (fp32 query), kv [B, N, 2, H, hd], dout [B, D]
    -> (out [B, D], prob [B, H, N], dkv [B, N, 2, H, hd], dq per sample [B, D], dq_mag [B, D]).
    dq = sum_j p_j (dp_j - sum_i p_i dp_i) k_j / sqrt(hd) cancels (to nothing when the attention is one-hot); dq_mag is the
    same sum over the magnitudes of its parts, p_j (|dp_j| + |sum_i p_i dp_i|) |k_j| / sqrt(hd), the size an fp32 error is
    relative to."""
    B, N, _, _, hd = kv.shape
    qs = q.double().reshape(1, H, hd).repeat(B, 1, 1).requires_grad_(True)    # one leaf per sample: dq_part
    kvl = kv.double().clone().requires_grad_(True)
    o, prob = attnpool_core(qs, kvl[:, :, 0], kvl[:, :, 1])
    o = o.reshape(B, H * hd)
    (o * dout.double()).sum().backward()
    k, v, prob = kv.double()[:, :, 0], kv.double()[:, :, 1], prob.detach()
    dp = torch.einsum("bhd,bnhd->bhn", dout.double().reshape(B, H, hd), v)
    rs = (prob * dp).sum(-1, keepdim=True)
    mag = torch.einsum("bhn,bnhd->bhd", prob * (dp.abs() + rs.abs()), k.abs()) * hd ** -0.5
    return o.detach(), prob.detach(), kvl.grad, qs.grad.reshape(B, H * hd), mag.reshape(B, H * hd)


# ------------------------------------------------------------------------------------ SimMIM pixel loss
def tokens_to_image(pred_tok, C, H, W, p, extra):
    """SimMIM's head output: token rows [B, extra + L, C p p] (Conv1x1 channel c p^2 + i p + j) -> PixelShuffle(p) ->
    [B, C, H, W] (utils/mim_vit.py:254-261, 469)."""
    B = pred_tok.shape[0]
    rows = pred_tok[:, extra:]
    return F.pixel_shuffle(rows.transpose(1, 2).reshape(B, C * p * p, H // p, W // p), p)


def image_to_tokens(img, p):
    """The inverse of tokens_to_image with extra = 0: [B, C, H, W] -> [B, L, C p p]."""
    B = img.shape[0]
    return F.pixel_unshuffle(img, p).reshape(B, img.shape[1] * p * p, -1).transpose(1, 2)


def simmim_target(imgs, p, pixel_mean, pixel_std, norm_pix):
    """The SimMIM loss's target image: input-normalised, then (norm-pix) per-patch NaN-aware mean / biased variance
    normalisation (utils/mim_vit.py:480-493, patch_mean_and_var :614-627)."""
    x = (imgs.double() - pixel_mean) / pixel_std
    if not norm_pix:
        return x
    B, C, H, W = x.shape
    pat = F.pixel_unshuffle(x, p).reshape(B, C, p * p, -1)                       # [B, C, p p, L]
    pat = pat.permute(0, 3, 1, 2).reshape(B, -1, C * p * p)                      # [B, L, C p p]: one patch vector per row
    ok = ~torch.isnan(pat)
    n = ok.sum(-1, keepdim=True)
    mean = torch.where(ok, pat, torch.zeros_like(pat)).sum(-1, keepdim=True) / n
    var = (torch.where(ok, pat - mean, torch.zeros_like(pat)) ** 2).sum(-1, keepdim=True) / n
    pat = (pat - mean) / (var + 1.0e-6) ** 0.5
    pat = pat.reshape(B, -1, C, p * p).permute(0, 2, 3, 1).reshape(B, C * p * p, -1)
    return F.pixel_shuffle(pat.reshape(B, C * p * p, H // p, W // p), p)


def simmim_pixel_loss(imgs, pred, pixel_mask, p, pixel_mean, pixel_std, norm_pix, loss_l1, extra=0, pooled=False):
    """The SimMIM branch of forward_loss (utils/mim_vit.py:480-520) in float64 with its gradient:
    loss = sum(w l) / (sum(w) + 1e-5), w = pixel_mask where the element loss is not NaN (else 0), l = (t - pred)^2 or |t - pred|.
    pred: token rows [B, extra + L, C p p], or the image [B, C, H, W] when pooled.  -> (loss, dpred shaped like pred, t)."""
    B, C, H, W = imgs.shape
    t = simmim_target(imgs, p, pixel_mean, pixel_std, norm_pix)
    pl = pred.double().clone().requires_grad_(True)
    img = pl if pooled else tokens_to_image(pl, C, H, W, p, extra)
    d = t - img
    ok = ~torch.isnan(d)
    d = torch.where(ok, d, torch.zeros_like(d))         # NaN elements leave numerator and denominator (mim_vit.py:509-515)
    w = torch.where(ok, pixel_mask.double(), torch.zeros_like(d))
    ell = d.abs() if loss_l1 else d * d
    loss = (w * ell).sum() / (w.sum() + 1e-5)
    loss.backward()
    return loss.detach(), pl.grad, t


# ------------------------------------------------------------------------------------ blended patch gather
def patch_rows_blend(imgs, pmv, pixel_mask, p, pixel_mean, pixel_std):
    """SimMIM's embedding input (utils/mim_vit.py:385-399) as the rows of the patch-embedding GEMM: normalise, NaN -> the
    learned patch_mask_values, x (1 - m) + pmv m (no blend when pixel_mask is None); -> [B L, C p p] in (c, py, px) order."""
    B, C, H, W = imgs.shape
    x = (imgs.double() - pixel_mean) / pixel_std
    fill = pmv.double().repeat(1, H // p, W // p).expand(B, -1, -1, -1)
    x = torch.where(torch.isnan(x), fill, x)
    if pixel_mask is not None:
        m = pixel_mask.double()
        x = x * (1 - m) + fill * m
    return image_to_tokens(x, p).reshape(B * (H // p) * (W // p), -1)


def patch_mask_values_grad(imgs, pixel_mask, drows, p):
    """d loss / d patch_mask_values [C, p, p] from the rows' gradient drows [B L, C p p]: sum of w drows, w = 1 at NaN
    pixels (the fill), else the pixel mask (the blend)."""
    B, C, H, W = imgs.shape
    w = torch.where(torch.isnan(imgs), torch.ones_like(imgs, dtype=torch.float64), pixel_mask.double())
    return (image_to_tokens(w, p).reshape(B * (H // p) * (W // p), -1) * drows.double()).sum(0).reshape(C, p, p)


# ------------------------------------------------------------------------------------ RA/Dec token
def radec_angles(ra_dec):
    """phi, theta as the reference computes them from its fp32 coordinates (torch.deg2rad on fp32: x * fl32(pi / 180);
    utils/location_encoder.py:161-163)."""
    rd = ra_dec.float()
    return torch.deg2rad(rd[:, 0]), torch.deg2rad(rd[:, 1] + 90)


def spherical_harmonics(ra_dec, dx=0.0):
    """oracle/mae_oracle.py spherical_harmonics in float64 from the reference's fp32 angles (radec_angles): the oracle's
    own function would convert degrees in float64 too, a different input.  -> [B, 25], l = 0..4, m = -l..l.
    dx: evaluated at cos(theta) + dx (clamped to [-1, 1]) -- the sensitivity to an error in the cosine."""
    phi, theta = (a.double() for a in radec_angles(ra_dec))
    ct = (torch.cos(theta) + dx).clamp(-1.0, 1.0)
    Y = []
    for l in range(mo.SH_L):
        for m in range(-l, l + 1):
            P = mo._assoc_legendre(l, abs(m), ct)
            if m == 0:
                Y.append(mo._sh_norm(l, 0) * P)
            elif m > 0:
                Y.append(math.sqrt(2.0) * mo._sh_norm(l, m) * torch.cos(m * phi) * P)
            else:
                Y.append(math.sqrt(2.0) * mo._sh_norm(l, -m) * torch.sin(-m * phi) * P)
    return torch.stack(Y, dim=-1)


def radec_token(sh, W0, b0, W1, b1, pos=None):
    """location_encoder after the harmonics (SirenNet, one hidden layer of 8): z = W0 sh + b0, token = W1 sin(30 z) + b1
    (+ pos_embed[1]).  -> (token [B, D], z [B, 8])."""
    z = sh.double() @ W0.double().T + b0.double()
    tok = torch.sin(mo.SIREN_W0_FIRST * z) @ W1.double().T + b1.double()
    return (tok if pos is None else tok + pos.double()), z
