"""GPU parity of the SimMIM / downstream-head kernels one entry point at a time: the attention pool (csrc/attnpool.hip), the
SimMIM pixel loss (csrc/loss.hip), the blended patch gather (csrc/frontend.hip) and the RA/Dec token (csrc/radec.hip),
called through sky_embeddings_amd.ops at the shapes and edges the end-to-end goldens never reach, against the float64
statements of tests/head_reference.py (pinned on the CPU by tests/test_head_reference_cpu.py) computed from the very
operands the kernel read.

Bars (`bar` below):
- fp32 outputs: ACC = 4e-6 of the reference's max-abs (for the attention pool's dq, a sum that cancels, of the max-abs of
  its terms' magnitudes).
- 16-bit outputs: the kernels compute in fp32 (|y32 - r| <= delta = ACC max|r|) and round to nearest even once, which moves
  a normal value by at most half an ulp, h |y32| with h = 2^-8 (bf16: 8 significant bits) or 2^-11 (fp16: 11), and an fp16
  subnormal by at most 2^-25.  So |y - r| <= h |y32| + delta <= h |r| + (1 + h) delta, bounded by h |r| + 2 delta (+ 2^-25).
- the RA/Dec harmonics add the spread of the fp64 statement over cos(theta) +- 2^-23 (two ulps of the fp32 cosine the
  kernel, like the reference, feeds to sqrt((1 - x)(1 + x)): within a degree of a pole that cancels, 0.4 % relative at
  dec = 89.91).
- exact contracts (layouts, zero rows, sentinels, the loss scale, the unblended gather): bit-exact.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import head_reference as hr
from tests.helpers import record_parity

DEV = "cuda"
NAN = float("nan")
ACC = 4e-6
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()  # fail loudly if libskyemb.so is missing
    return _ops


def dev(t, dtype=None):
    t = t.to(DEV)
    return t.to(dtype) if dtype is not None else t


def bar(ref, dtype, mag=None):
    """Elementwise bound on |kernel - ref| for an output stored in `dtype` (module docstring); mag: the magnitude of the
    terms of a sum that cancels, in place of |ref|."""
    delta = ACC * float((ref if mag is None else mag).abs().max())
    if dtype == torch.float32:
        return torch.full_like(ref, delta)
    return HALF_ULP[dtype] * ref.abs() + 2 * delta + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def close(errs, name, out, ref, dtype=torch.float32, mag=None, extra=None):
    """Asserts |out - ref| <= bar elementwise (a NaN, e.g. an element never written, fails) and notes the worst
    error as a fraction of its bar in `errs`."""
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    b = bar(ref, dtype, mag) + (0.0 if extra is None else extra.double())
    err = (out - ref).abs()
    ok = err <= b
    if not bool(ok.all()):
        i = int((~ok).reshape(-1).nonzero()[0])
        raise AssertionError(f"{name}: {int((~ok).sum())} of {ok.numel()} elements off; first at {i}: kernel "
                             f"{float(out.reshape(-1)[i])} fp64 {float(ref.reshape(-1)[i])} bar {float(b.reshape(-1)[i]):.3g}")
    errs[name] = round(float((err / b.clamp_min(1e-300)).max()), 4)


# ------------------------------------------------------------------------------------ attention pool
def run_attnpool(ops, B, N, H, hd, dtype, kv, dout, q=None, latent=None, Wq=None, bq=None):
    """attnpool_q (unless q is given) -> _fwd -> _bwd -> _q_bwd against fp64; returns {output: error / bar}."""
    D, errs = H * hd, {}
    if q is None:
        qd = torch.full((D,), NAN, device=DEV)
        ops.attnpool_q(dev(latent), dev(Wq), dev(bq), qd)
        close(errs, "q", qd, Wq.double() @ latent.double() + bq.double())
    else:
        qd = dev(q)
    kvd, doutd = dev(kv, dtype), dev(dout, dtype)
    out = torch.full((B, D), NAN, device=DEV, dtype=dtype)
    prob = torch.full((B * H * N,), NAN, device=DEV)
    ops.attnpool_fwd(qd, kvd, out, prob, B, N, H, hd)
    dkv = torch.full_like(kvd, NAN)                   # sentinel: every element must be written
    dq_part = torch.full((B, D), NAN, device=DEV)
    ops.attnpool_bwd(qd, kvd, doutd, prob, dkv, dq_part, B, N, H, hd)
    q_k = qd.cpu()
    r_out, r_prob, r_dkv, r_dq, r_dq_mag = hr.attnpool_grads(q_k, kvd.cpu().reshape(B, N, 2, H, hd), doutd.cpu(), H)
    close(errs, "prob", prob.reshape(B, H, N), r_prob)
    close(errs, "out", out, r_out, dtype)
    assert not bool(torch.isnan(dkv).any()), "dkv: elements left unwritten"
    close(errs, "dkv", dkv.reshape(B, N, 2, H, hd), r_dkv, dtype)
    close(errs, "dq_part", dq_part, r_dq, mag=r_dq_mag)
    if latent is not None:
        dWq, dbq, dlat, ws = (torch.full(s, NAN, device=DEV) for s in ((D, D), (D,), (D,), (D,)))
        ops.attnpool_q_bwd(dq_part, dev(latent), dev(Wq), dWq, dbq, dlat, ws)
        dq = dq_part.cpu().double().sum(0)             # from the dq_part the kernel read
        close(errs, "dWq", dWq, torch.outer(dq, latent.double()))
        close(errs, "dbq", dbq, dq)
        close(errs, "dlatent", dlat, Wq.double().T @ dq)
    return errs


AP_SHAPES = [  # (B, N, H, hd): N over 64 -> lanes loop over tokens; hd over 64 -> over columns; B H % 4 != 0 -> idle waves
    (3, 1, 1, 4),
    (5, 18, 2, 36),
    (3, 64, 1, 64),
    (7, 65, 1, 384),
    (3, 66, 12, 64),      # SimMIM ViT-B: 64 patches + cls + RA/Dec
    (3, 66, 2, 512),      # downstream predictor at ViT-L: two heads of 512
    (3, 130, 2, 36),
    (3, 256, 1, 512),     # MAXN x MAXHD
    (1, 256, 2, 4),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT.get)
@pytest.mark.parametrize("shape", AP_SHAPES, ids=lambda s: "B%d_N%d_H%d_hd%d" % s)
def test_attnpool(ops, shape, dtype):
    B, N, H, hd = shape
    D = H * hd
    g = torch.Generator().manual_seed(B * 1000 + N * 10 + hd)
    latent = torch.randn(D, generator=g)
    Wq = torch.randn(D, D, generator=g) / D ** 0.5
    bq = 0.1 * torch.randn(D, generator=g)
    kv = torch.randn(B, N, 2, H, hd, generator=g)
    dout = torch.randn(B, D, generator=g)
    errs = run_attnpool(ops, B, N, H, hd, dtype, kv, dout, latent=latent, Wq=Wq, bq=bq)
    record_parity(f"head_attnpool[{DT[dtype]}-B{B}_N{N}_H{H}_hd{hd}]", errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT.get)
@pytest.mark.parametrize("case", ["large_pos", "large_neg", "one_hot"])
def test_attnpool_extreme_logits(ops, case, dtype):
    """Scores of |s| ~ 100 (exp overflows fp32 above 88.7 and underflows below -103 unless the max is subtracted) and an
    attention within e^-40 of one-hot.  Operands on a coarse dyadic grid (exact in every dtype) with hd = 64 (scale 1/8):
    the kernel's fp32 scores are exact, so the bar speaks to the softmax alone."""
    B, N, H, hd = 3, 66, 2, 64
    g = torch.Generator().manual_seed(17)
    r = torch.randint(0, 2, (H, hd), generator=g).float() * 2 - 1
    q = 4.0 * r                                                              # s_j = (1/8) 4 r . k_j = 32 a_j + (1/2) r . e_j
    if case == "one_hot":
        a = torch.full((B, N, H), 0.25)
        a[:, 7] = 1.5                                                        # one token 40 above the rest
    else:
        a = (3.0 + torch.randint(0, 8, (B, N, H), generator=g) / 32.0) * (1 if case == "large_pos" else -1)
    e = torch.randint(-1, 2, (B, N, H, hd), generator=g) / 8.0
    k = a[..., None] * r + e
    s = torch.einsum("hd,bnhd->bhn", q, k) / 8
    assert float(s.abs().min()) > (0 if case == "one_hot" else 90)
    kv = torch.stack([k, torch.randn(B, N, H, hd, generator=g)], 2)
    errs = run_attnpool(ops, B, N, H, hd, dtype, kv, torch.randn(B, H * hd, generator=g), q=q.reshape(-1))
    record_parity(f"head_attnpool_logits[{DT[dtype]}-{case}]", errs)


@pytest.mark.parametrize("B", [1, 300])
@pytest.mark.parametrize("D", [36, 1024])
def test_attnpool_q_bwd_batch_sum(ops, B, D):
    """The fixed-order reduction of dq over the batch (one 256-thread block per output: B > 256 loops) and the dlatent
    columns (D > 256: several blocks)."""
    g = torch.Generator().manual_seed(B + D)
    dq_part, latent, Wq = torch.randn(B, D, generator=g), torch.randn(D, generator=g), torch.randn(D, D, generator=g) / D ** 0.5
    dWq, dbq, dlat, ws = (torch.full(s, NAN, device=DEV) for s in ((D, D), (D,), (D,), (D,)))
    ops.attnpool_q_bwd(dev(dq_part), dev(latent), dev(Wq), dWq, dbq, dlat, ws)
    dq, errs = dq_part.double().sum(0), {}
    close(errs, "dWq", dWq, torch.outer(dq, latent.double()))
    close(errs, "dbq", dbq, dq)
    close(errs, "dlatent", dlat, Wq.double().T @ dq)
    record_parity(f"head_attnpool_q_bwd[B{B}_D{D}]", errs)


@pytest.mark.parametrize("N,hd", [(257, 64), (18, 516), (18, 6)])
def test_attnpool_rejects_shapes_beyond_its_lds(ops, N, hd):
    """N > MAXN = 256, hd > MAXHD = 512 and hd % 4 != 0 are refused by the argument check (nothing is launched; the
    buffers are full-sized all the same)."""
    B, H = 1, 1
    q = torch.zeros(hd, device=DEV)
    kv = torch.zeros(B, N, 2, H, hd, device=DEV)
    out, prob = torch.zeros(B, hd, device=DEV), torch.zeros(B * H * N, device=DEV)
    with pytest.raises(Exception, match="bad shape"):
        ops.attnpool_fwd(q, kv, out, prob, B, N, H, hd)
    with pytest.raises(Exception, match="bad shape"):
        ops.attnpool_bwd(q, kv, out, prob, torch.zeros_like(kv), torch.zeros(B, hd, device=DEV), B, N, H, hd)
    assert not bool(out.any()) and not bool(prob.any())


# ------------------------------------------------------------------------------------ SimMIM pixel loss
def loss_inputs(g, B, C, H, W, p, pixel_mean, pixel_std, norm_pix):
    """Images with a fully-NaN patch, a constant patch (variance 0), scattered NaN pixels, a per-channel 0/1 pixel mask,
    and a prediction at least 1/64 away from the fp64 target (an L1 sign never hangs on rounding)."""
    imgs = 1.5 * torch.randn(B, C, H, W, generator=g) + 0.3
    assert W // p >= 3
    imgs[0, :, 0:p, p:2 * p] = NAN                                     # patch 1 of sample 0: no valid pixel
    imgs[0, :, 0:p, 2 * p:3 * p] = pixel_mean                          # patch 2: constant, input-normalised to exactly 0
    imgs[B - 1, 0][torch.rand(H, W, generator=g) < 0.1] = NAN
    mask = (torch.rand(B, C, H, W, generator=g) < 0.6).float()
    t = hr.simmim_target(imgs, p, pixel_mean, pixel_std, norm_pix)
    off = (torch.rand(t.shape, generator=g) * 2 + 1 / 64) * (torch.randint(0, 2, t.shape, generator=g) * 2 - 1)
    pred_img = torch.where(torch.isnan(t), torch.randn(t.shape, generator=g, dtype=torch.float64), t + off).float()
    return imgs, mask, pred_img


def launch_loss(ops, imgs, pred, mask, dtype, p, extra, pixel_mean, pixel_std, norm_pix, l1, pooled, dscale=1.0):
    B, C, H, W = imgs.shape
    L = (H // p) * (W // p)
    loss = torch.full((1,), NAN, device=DEV)
    ws = torch.full((4 * B * L + 4,), NAN, device=DEV)
    dpred = torch.full(pred.shape, NAN, device=DEV, dtype=dtype)        # sentinel: cls / RA-Dec rows must become 0
    pred_img = torch.full((B, C, H, W), NAN, device=DEV)
    ops.simmim_pixel_loss(dev(imgs), dev(pred), dev(mask), loss, dpred, ops.dtype_code(dtype), pred_img, ws, p, extra,
                          pixel_mean, pixel_std, norm_pix, l1, pooled=pooled, dscale=dscale)
    return loss.cpu(), dpred.cpu(), pred_img.cpu()


PL_GEOMS = [  # (B, C, H, W, p, extra, pooled)
    (16, 1, 64, 64, 4, 1, False),    # B L = 4096 patches in the finalize reduction
    (3, 5, 32, 48, 8, 2, False),     # pv = 320 > 256 threads, non-square grid, cls + RA/Dec rows
    (2, 9, 48, 48, 16, 0, False),    # pv = 2304
    (4, 9, 32, 32, 4, 1, False),
    (2, 5, 32, 32, 8, 0, True),      # attention-pool head: the prediction is the image
    (3, 1, 48, 48, 16, 0, True),     # pv = 256
]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT.get)
@pytest.mark.parametrize("norm_pix,l1", [(True, True), (True, False), (False, True), (False, False)],
                         ids=["normpix-l1", "normpix-mse", "l1", "mse"])
@pytest.mark.parametrize("geom", PL_GEOMS, ids=lambda s: "B%d_C%d_%dx%d_p%d_extra%d_pooled%d" % s)
def test_simmim_pixel_loss(ops, geom, norm_pix, l1, dtype):
    B, C, H, W, p, extra, pooled = geom
    mean, std = 0.2, 1.7
    g = torch.Generator().manual_seed(B * 100 + C * 10 + p + 1000 * norm_pix + 2000 * l1)
    imgs, mask, pred_img = loss_inputs(g, B, C, H, W, p, mean, std, norm_pix)
    if pooled:
        pred = pred_img
    else:   # junk in the cls / RA-Dec rows: they take no part in the loss
        tok = hr.image_to_tokens(pred_img, p)
        pred = torch.cat([100 * torch.randn(B, extra, tok.shape[2], generator=g), tok], 1)
    r_loss, r_dpred, _ = hr.simmim_pixel_loss(imgs, pred, mask, p, mean, std, norm_pix, l1, extra=extra, pooled=pooled)
    loss, dpred, pimg = launch_loss(ops, imgs, pred, mask, dtype, p, extra, mean, std, norm_pix, l1, pooled)
    errs = {}
    close(errs, "loss", loss.reshape(()), r_loss)
    close(errs, "dpred", dpred, r_dpred, dtype)
    if not pooled:
        assert bool((dpred[:, :extra] == 0).all()), "cls / RA-Dec rows of dpred must be written as 0"
    # pred_img is the PixelShuffle of the token rows, bit for bit
    assert torch.equal(pimg, pred if pooled else hr.tokens_to_image(pred, C, H, W, p, extra))
    record_parity(f"head_simmim_loss[{DT[dtype]}-B{B}_C{C}_p{p}_x{extra}_pool{int(pooled)}-np{int(norm_pix)}-l1{int(l1)}]", errs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT.get)
def test_simmim_pixel_loss_edges(ops, dtype):
    """All-zero and all-one pixel masks, L1 where the prediction equals the target (gradient 0, as torch's sign(0)),
    and the static loss scale: dscale = 2^k scales dpred by exactly 2^k and leaves the loss alone."""
    B, C, H, W, p, extra = 3, 5, 32, 32, 8, 1
    mean, std = 0.25, 2.0             # dyadic, with pixels on a 2^-10 grid: the normalised target is exact in fp32
    g = torch.Generator().manual_seed(29)
    imgs, _, pred_img = loss_inputs(g, B, C, H, W, p, mean, std, False)
    imgs = torch.where(torch.isnan(imgs), imgs, torch.round(imgs * 1024) / 1024)
    t = hr.simmim_target(imgs, p, mean, std, False)
    ok = ~torch.isnan(t)
    assert torch.equal(t[ok].float().double(), t[ok])                  # the fp32 target the kernel forms is this one
    same = ~torch.isnan(t)
    same[:, :, :, : W // 2] = False
    pred_img = torch.where(same, t.float(), pred_img)                  # prediction == target on the right half
    tok = hr.image_to_tokens(pred_img, p)
    pred = torch.cat([torch.randn(B, extra, tok.shape[2], generator=g), tok], 1)
    errs = {}
    for kind in ("zero", "one", "random"):
        mask = {"zero": torch.zeros(B, C, H, W), "one": torch.ones(B, C, H, W),
                "random": (torch.rand(B, C, H, W, generator=g) < 0.5).float()}[kind]
        r_loss, r_dpred, _ = hr.simmim_pixel_loss(imgs, pred, mask, p, mean, std, False, True, extra=extra)
        loss, dpred, _ = launch_loss(ops, imgs, pred, mask, dtype, p, extra, mean, std, False, True, False)
        if kind == "zero":            # sum(w) = 0: the 1e-5 keeps the loss 0 / 1e-5 = 0 (no NaN)
            assert float(loss) == 0.0 and bool((dpred == 0).all()) and float(r_loss) == 0.0
            continue
        assert abs(float(loss) - float(r_loss)) <= ACC * float(r_loss), (kind, float(loss), float(r_loss))
        close(errs, f"dpred_{kind}", dpred, r_dpred, dtype)
        rows = hr.image_to_tokens(same.double(), p).bool()
        assert bool((dpred[:, extra:][rows] == 0).all()), "L1 gradient where pred == target must be 0"
        assert bool((dpred[:, :extra] == 0).all())
    # dscale = 2^k: the loss is unchanged and dpred is exactly 2^k times the unscaled one (fp16: where both are normal)
    base_loss, base, _ = launch_loss(ops, imgs, pred, mask, dtype, p, extra, mean, std, True, False, False)
    for k in ((4, 10) if dtype == torch.float16 else (-3, 4, 10)):     # fp16 gradients need scaling up, not down
        loss, d, _ = launch_loss(ops, imgs, pred, mask, dtype, p, extra, mean, std, True, False, False, dscale=2.0 ** k)
        assert torch.equal(loss, base_loss)
        want = base.float() * 2.0 ** k
        sel = torch.ones_like(want, dtype=torch.bool)
        if dtype == torch.float16:
            # (2^-13, not 2^-14: a stored 2^-14 may have been rounded up from a subnormal)
            sel = (base.float().abs() >= 2.0 ** -13) & (want.abs() >= 2.0 ** -13) & (want.abs() <= 65504)
            assert int(sel.sum()) > 1000
        assert torch.equal(d.float()[sel], want[sel]), k
    record_parity(f"head_simmim_loss_edges[{DT[dtype]}]", errs)


# ------------------------------------------------------------------------------------ blended patch gather
@pytest.mark.parametrize("dtype", DTYPES, ids=DT.get)
@pytest.mark.parametrize("geom", [(5, 64, 16), (9, 32, 8), (1, 32, 4)], ids=lambda s: "C%d_S%d_p%d" % s)
def test_patch_gather_blend(ops, geom, dtype):
    C, S, p = geom
    B, L, pv = 3, (S // p) ** 2, C * p * p
    mean, std = 0.2, 1.7
    g = torch.Generator().manual_seed(C * 7 + p)
    x = torch.randn(B, C, S, S, generator=g)
    x[0, 0, :5, :11] = NAN
    x[2, C - 1][torch.rand(S, S, generator=g) < 0.2] = NAN
    mask = (torch.rand(B, C, S, S, generator=g) < 0.5).float()
    mask[1, :, ::5] = torch.rand(C, (S + 4) // 5, S, generator=g)     # a few fractional weights besides the 0 / 1 mask
    nan = torch.isnan(x)
    assert bool((nan & (mask == 1)).any()) and bool((nan & (mask == 0)).any())
    pmv = torch.randn(C, p, p, generator=g)
    xd, pmvd, maskd = dev(x), dev(pmv), dev(mask)
    out = torch.full((B * L, pv), NAN, device=DEV, dtype=dtype)
    ops.patch_gather_blend(xd, pmvd, None, maskd, out, p, L, mean, std)
    errs = {}
    close(errs, "rows", out, hr.patch_rows_blend(x, pmv, mask, p, mean, std), dtype)
    # no pixel mask: the plain patch gather, bit for bit
    a = torch.full((B * L, pv), NAN, device=DEV, dtype=dtype)
    b = torch.full((B * L, pv), 7.0, device=DEV, dtype=dtype)
    ops.patch_gather_blend(xd, pmvd, None, None, a, p, L, mean, std)
    ops.patch_gather(xd, pmvd, None, b, p, L, mean, std)
    assert torch.equal(a.cpu().view(torch.int16 if dtype != torch.float32 else torch.int32),
                       b.cpu().view(torch.int16 if dtype != torch.float32 else torch.int32))
    close(errs, "rows_unblended", a, hr.patch_rows_blend(x, pmv, None, p, mean, std), dtype)
    # d patch_mask_values = sum of w drows, w = 1 at NaN pixels, else the pixel mask
    drows = torch.randn(B * L, pv, generator=g)
    part, dpmv = torch.full((B, pv), NAN, device=DEV), torch.full((C, p, p), NAN, device=DEV)
    ops.patch_gather_bwd_pmv_blend(xd, None, maskd, dev(drows), part, dpmv, p, L)
    close(errs, "dpmv", dpmv, hr.patch_mask_values_grad(x, mask, drows, p))
    record_parity(f"head_patch_gather_blend[{DT[dtype]}-C{C}_S{S}_p{p}]", errs)


# ------------------------------------------------------------------------------------ RA/Dec token
RD_EDGES = [(359.999, 90.0), (0.0, -90.0), (360.0, 0.0), (0.0, 0.0), (123.4, 90.0), (360.0, -90.0), (359.999, -45.5)]


@pytest.mark.parametrize("with_pos", [True, False], ids=["pos", "nopos"])
@pytest.mark.parametrize("D", [32, 768, 1000, 1024])
@pytest.mark.parametrize("B", [1, 3, 300])
def test_radec_token(ops, B, D, with_pos):
    """Forward into the second of three token rows per sample (row_stride 3 D; the other rows hold a sentinel that must
    survive), then the backward from gradient rows whose neighbours are NaN (read, they would poison the result).
    Each stage against fp64 from the operands the kernel read: sh from the coordinates, z from the kernel's sh, the token
    from its z; the gradients by fp64 autograd through the kernel's z and sh."""
    g = torch.Generator().manual_seed(B * 7 + D + with_pos)
    ra_dec = torch.stack([torch.rand(B, generator=g) * 360, torch.rand(B, generator=g) * 180 - 90], 1)
    n = min(B, len(RD_EDGES))
    ra_dec[:n] = torch.tensor(RD_EDGES[:n])
    W0 = (torch.rand(8, 25, generator=g) * 2 - 1) * 0.2
    b0 = (torch.rand(8, generator=g) * 2 - 1) * 0.5
    W1 = torch.randn(D, 8, generator=g) / 8 ** 0.5
    b1 = 0.1 * torch.randn(D, generator=g)
    pos = 0.02 * torch.randn(D, generator=g) if with_pos else None
    NT, SENT = 3, -1234.5
    x = torch.full((B, NT, D), SENT, device=DEV)
    sh, z = torch.full((B, 25), NAN, device=DEV), torch.full((B, 8), NAN, device=DEV)
    W1d = dev(W1)
    ops.radec_token_fwd(dev(ra_dec), dev(W0), dev(b0), W1d, dev(b1), dev(pos) if with_pos else None, x.view(-1)[D:], NT * D,
                        B, D, sh, z)
    x, sh_k, z_k, errs = x.cpu(), sh.cpu(), z.cpu(), {}
    r_sh = hr.spherical_harmonics(ra_dec)
    cond = torch.maximum((hr.spherical_harmonics(ra_dec, 2.0 ** -23) - r_sh).abs(), (hr.spherical_harmonics(ra_dec, -2.0 ** -23) - r_sh).abs())
    close(errs, "sh", sh_k, r_sh, extra=cond)
    pole = ra_dec[:, 1].abs() == 90                  # every m != 0 harmonic vanishes there: held to the plain fp32 bar
    mnz = [l * l + l + m for l in range(5) for m in range(-l, l + 1) if m != 0]
    assert float(sh_k[pole][:, mnz].abs().max()) <= ACC * float(r_sh.abs().max())
    _, r_z = hr.radec_token(sh_k, W0, b0, W1, b1)
    close(errs, "z", z_k, r_z)
    tok = torch.sin(30.0 * z_k.double()) @ W1.double().T + b1.double() + (pos.double() if with_pos else 0.0)
    close(errs, "token", x[:, 1], tok)
    assert bool((x[:, 0] == SENT).all()) and bool((x[:, 2] == SENT).all()), "rows beside the RA/Dec row were written"
    # backward
    gr = torch.full((B, NT, D), NAN)
    gr[:, 1] = torch.randn(B, D, generator=g)
    outs = [torch.full(s, NAN, device=DEV) for s in ((B, 8), (8, 25), (8,), (D, 8), (D,))]
    ops.radec_token_bwd(dev(gr).view(-1)[D:], NT * D, W1d, dev(sh_k), dev(z_k), *outs, B, D)
    _, dW0, db0, dW1, db1 = (o.cpu() for o in outs)
    W0l, b0l, W1l, b1l = (t.double().clone().requires_grad_(True) for t in (W0, b0, W1, b1))
    zl = sh_k.double() @ W0l.T + b0l
    zl = zl + (z_k.double() - zl).detach()           # the kernel's z as the value, the linear layer's gradient
    y = torch.sin(30.0 * zl) @ W1l.T + b1l
    (y * gr[:, 1].double()).sum().backward()
    close(errs, "dW0", dW0, W0l.grad)
    close(errs, "db0", db0, b0l.grad)
    close(errs, "dW1", dW1, W1l.grad)
    close(errs, "db1", db1, b1l.grad)
    record_parity(f"head_radec[B{B}_D{D}_{'pos' if with_pos else 'nopos'}]", errs)
