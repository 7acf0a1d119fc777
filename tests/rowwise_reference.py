"""Float64 statements of the row-wise kernels around the GEMMs -- LayerNorm forward / backward / reduce (layernorm.hip,
ln_bwd_body.h), the flat-buffer AdamW (adamw.hip, adamw_math.h), the masked per-patch loss of the MAE path (loss.hip) and the
reductions and copies of frontend.hip -- with their elementwise error bars, fp32 emulations and the case tables of
tests/test_rowwise_elementwise_gpu.py.  Pinned on the CPU by tests/test_rowwise_reference_cpu.py.

Every statement (`*_reference`) is computed in fp64 from the inputs exactly as the kernel reads them (16-bit values and fp32
scalars widened) and follows the semantics of the .hip headers, not their summation order.  Every function here is plain torch
and runs on the device of its inputs (the 12.6 M element AdamW case is compared on the GPU in fp64).

Notation.  u = 2^-24 (fp32 unit roundoff); h = the stored format's (2^-8 bf16, 2^-11 fp16, u fp32).  A sum of n terms accumulated
in fp32 in ANY order errs by at most n u sum|terms| (the gamma_n bound; n = the additions the kernel makes, the roundings of the
terms themselves counted separately).  Transcendentals and divisions get explicit allowances, relative to their result:
    E_DIV = 5 u   a / b: 2.5 ulp, the loosest fp32 division the compiler may emit (correctly rounded by default: 0.5 ulp)
    E_SQRT = 4 u  sqrtf: 2 ulp (v_sqrt_f32 is specified at 1 ulp)          E_RSQ = 4 u  rsqrtf: 2 ulp (v_rsq_f32: 1 ulp)
A value whose fp32 form errs by e and that is rounded once to the stored format obeys (attention_reference, item 3)
    |y - r| <= h |r| + (1 + h) e + floor,   floor = 2^-126 (a flushed subnormal) + 2^-25 in fp16 (its subnormal rounding);
an fp32 output: e + 2^-126 (its own rounding is part of e).  Bounds are first order in u unless said otherwise.

LayerNorm forward (x [M, D], gamma, beta, eps -> mean, rstd = 1 / sqrt(var_biased + eps), y; y32 and y are two roundings of the
same value).  A = sum|x| / D.
    mean:  D - 1 additions and the division by D:               e_mean = D u A
    c_i = x_i - mean:  the kernel subtracts ITS mean; the difference is rounded relative to |x_i - mean32|, but the mean it
           subtracts is off by e_mean, and e_mean scales with |x|, not with |x - mean|:
                                                                e_c,i = e_mean + u (|x_i| + |mean|)
           THIS is the cancellation term: a row of mean 300 and unit spread has e_c ~ 300 (D + 2) u against a centred row's
           ~ (D + 2) u -- about 300 times wider, carried into y by rstd |gamma| below.
    var:   sum of squares of c (d_i = x_i - mean exact), D additions, square and division:
                                                                e_var = sum(2 |d_i| e_c,i + e_c,i^2) / D + (D + 2) u var
    rstd:  w = var + eps (one rounding), rsqrtf:                e_w = e_var + u w;  e_rstd = rstd (e_w / (2 (w - e_w)) + E_RSQ)
           ((1 - t)^-1/2 - 1 <= t / (2 (1 - t)): valid to all orders, the offset rows have e_w / w of a few per cent)
    y32:   ((c rstd) gamma) + beta, three roundings of t = |xhat gamma| and one of the sum:
                                                                e_y = |gamma| (rstd e_c + |d| e_rstd) + 3 u t + u |beta|
LayerNorm backward (dy, x, gamma and the STORED fp32 mean / rstd as inputs, so the backward is judged on its own and no
cancellation term appears: fl(x - mean32) errs by u |x - mean32| only).  xhat = (x - mean) rstd, a = dy gamma, m1 = sum a / D,
m2 = sum a xhat / D, g_out = g_in + rstd (a - m1 - xhat m2); block blk of nblk = skyemb_layernorm_bwd_blocks(M) owns the rows
blk 4 + w + k nblk 4 (w = 0..3, k = 0, 1, ...), part[0 / 1][blk] = sum over them of dy xhat / dy, dgamma / dbeta = sum_blk part.
    xhat: 2 u |xhat|;   a: u |a|
    m1:   products rounded once, D - 1 additions, division:     e_m1 = (D + 1) u sum|a| / D
    m2:   a xhat carries 1 + 2 + 1 roundings:                   e_m2 = (D + 4) u sum|a xhat| / D
    g:    T = |a| + |m1| + |xhat m2|; the operands' own errors (4 u |a|, 3 u |m1|, 5 u |xhat m2| with the two subtractions and
          the rstd multiply) are bounded by 5 u T:              e_g = rstd (e_m1 + |xhat| e_m2 + 5 u T) + u (rstd T + |g_in|)
          (the last term: the add of g_in; absent without it)
    part: R = rows of the block; a term passes through at most R additions in its wave and 3 across the four waves, and the
          product dy xhat carries 3 roundings:                  e_part0 = (R + 6) u sum|dy xhat|,  e_part1 = (R + 3) u sum|dy|
    dgamma / dbeta (and skyemb_layernorm_bwd_reduce_batch on any table): nblk more additions of the parts:
                                                                e = sum_blk e_part + nblk u sum_blk |part terms|

AdamW (adamw_math.h; lr, bc1, bc2, beta1, beta2, eps, wd, grad_scale as the fp32 values the kernel receives): gj = g grad_scale,
pd = p (1 - lr wd) where index < n_decay else p, m' = beta1 m + (1 - beta1) gj, v' = beta2 v + (1 - beta2) gj^2,
denom = sqrt(v') / sqrt(bc2) + eps, p' = pd - (lr / bc1) m' / denom, p_lp = round(p'), g zeroed when asked.
    pd:    lr wd, 1 - lr wd, the product:                       e_pd = 3 u |p| (0 where not decayed)
    m':    gj, 1 - beta1, their product, the fma:               e_m = 4 u (|beta1 m| + |(1 - beta1) gj|)
    v':    gj^2 (3 u), 1 - beta2, product, fma; all terms >= 0:  e_v = 6 u v' + 2^-126 (gj^2 of a 1e-20 gradient is subnormal)
    sqrt:  |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b):      e_s = e_v / (sqrt v' + sqrt max(v' - e_v, 0)) + E_SQRT sqrt v'
    denom: q = sqrt v' / sqrt bc2: E_SQRT for sqrt bc2, E_DIV; then + eps: e_den = (e_s / sqrt bc2) + (E_SQRT + E_DIV) q + u denom
           (v' = 0: denom = eps exactly and the update m' / eps is as large as it gets: the sensitive elements of the cases)
    r = m' / denom:                                             e_r = e_m / denom + |r| (e_den / denom + E_DIV)
    p':    lr / bc1 (E_DIV), the fma:                           e_p = e_pd + step (e_r + E_DIV |r|) + u |p'|
The masked patch loss (loss.hip; t = (img - pixel_mean) / pixel_std in patchify order, finite elements only, n of them per patch):
mu = sum t / n, var = sum (t - mu)^2 / n, istd = 1 / sqrt(var + 1e-6), tn = (t - mu) istd, diff = tn - pred, per patch S = sum diff^2
| sum |diff| and cnt over the non-NaN elements; over the masked patches S, N; scale = N / numel numel, loss = S / (scale + 1e-5),
inv = dscale / (scale + 1e-5), dpred = mask valid (2 (pred - tn) | sign(pred - tn)) inv, zero rows for the `extra` tokens and the
unmasked patches; ws[patch] = (S, cnt, mu, istd), zeros for an unmasked patch.
    t:     subtraction, division:                               e_t = (u + E_DIV) |t|
    mu:    n additions, division:                               e_mu = sum e_t / n + (n + 5) u sum|t| / n
    d:     as LayerNorm's c:                                    e_d = e_t + e_mu + u (|t| + |mu|)
    var:                                                        e_var = sum(2 |d| e_d + e_d^2) / n + (n + 1 + 5) u var
    istd:  w = var + 1e-6, sqrtf, 1 / .:                        e_istd = istd (e_w / (2 (w - e_w)) + E_SQRT + E_DIV), e_w = e_var + u w
    diff:  (d istd) - pred:                                     e_diff = istd e_d + |d| e_istd + u |tn| + u |diff|
    elem:  mse 2 |diff| e_diff + e_diff^2 + u diff^2; L1 e_diff;  S_patch: sum e_elem + pv u S_patch;  S: + B L u S
    loss:  N is exact (integers below 2^24); N / numel numel: E_DIV + u; + 1e-5: u; S / den: E_DIV:
                                                                e_loss = e_S / den + |loss| (2 E_DIV + 2 u)
    dpred: inv: 2 E_DIV + 3 u relative (the reciprocal, dscale); mse: 2 e_diff inv + |g| (2 E_DIV + 4 u); L1: |g| (2 E_DIV + 3 u)
           where the sign is determined, i.e. |diff| > e_diff.  Elements with 0 < |diff| <= e_diff are ill-conditioned and are not
           compared (`ill`; the cases are chosen so that there are none, test_l1_cases_have_no_ill_conditioned_sign).  A diff of
           exactly 0 is compared: it arises only where t = mu and pred = 0 exactly (the patch of two EQUAL finite pixels), which
           every arithmetic reproduces (t + t, / 2, t - t and 0 istd are exact), and there the gradient must be exactly 0.
colsum (X [M, ldx] -> out[n] = sum_m X[m, n]): M u sum|X| + 2^-126.  rowsum_select (partial[blk] = the selected rows i = blk mod
256, out = colsum of the 256 partials): partial ceil(n_rows / 256) u sum|x|, out (ceil(n_rows / 256) + 256) u sum|x|.
gather_rows, fill_mask_tokens (one fp32 addition: correctly rounded) and cast are exact: torch.equal against the rounded value.

The fp32 terms are worst-case bounds (every rounding in one direction, n u where real sums err like sqrt(n) u).  Worst err/bar of
the fp32 emulation (`*_emulate`) over the cases, measured on the CPU and pinned per family by the floors of
tests/test_rowwise_reference_cpu.py (FLOORS, one tenth of the smallest figure):
%(MEASURED)s
What the kernels achieve on the GPU is recorded by tests/test_rowwise_elementwise_gpu.py (record_parity "rowwise_elementwise"), not
assumed here.
"""
import math
from collections import namedtuple

import torch

from tests.attention_reference import F16_SUB, TINY, U32, UNIT, round_to, worst  # noqa: F401  (re-exported)

MEASURED = """\
    ln_fwd     mean 0.0001-0.041, rstd 0.00001-0.047, y32 0.002-0.64 (highest at D = 4), 16-bit y 0.75-0.98
    ln_bwd     g_out 0.005-0.20, 16-bit g_lp 0.57-0.995, fp32 g_lp as g_out, part 0.11-0.37, dgamma 0.0006-0.26, dbeta 0.0002-0.24
               (dbeta of a few 16-bit rows: often exact); the D = 192 table of 289 blocks: dgamma / dbeta 0.0002-0.0008
    ln_reduce  0.0096
    adamw      p 0.49-0.98 (the final rounding u |p'| IS the bar where the update is small, and half an ulp reaches u |p'| just
               above a power of two), m 0.42-0.48, v 0.29-0.42, 16-bit p_lp 0.97-0.996
    loss       loss 0.000001-0.003, ws 0.07-0.09, dpred32 0.009-0.06, 16-bit dpred 0.19-0.95
    colsum     0.00008-0.002 (M >= 301);   rowsum_select  partial 0.37-0.60 (two to five terms), out 0.0007-0.004"""
__doc__ = __doc__ % {"MEASURED": MEASURED}

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {F32: "f32", BF: "bf16", F16: "f16", None: "none"}
E_DIV = 5 * U32
E_SQRT = 4 * U32
E_RSQ = 4 * U32
LN_BWD_CAP = 576              # common.h SKY_LN_BWD_CAP
LN_EPS = 1e-6


def f32(x):
    """The python float x as the fp32 value a kernel receives."""
    return float(torch.tensor(x, dtype=F32))


def stored(r, e, dtype):
    """Bar of an output stored in `dtype` whose fp32 form errs by at most e from the statement r (module docstring)."""
    if dtype == F32:
        return e + TINY
    h = UNIT[dtype]
    return h * r.abs() + (1 + h) * e + TINY + (F16_SUB if dtype == F16 else 0.0)


def ratio(got, ref, bar, skip=None):
    """max |got - ref| / bar (inf for a NaN that the statement does not have); `skip`: elements left out."""
    got, ref = got.double(), ref.double()
    nan = torch.isnan(ref)
    if not torch.equal(torch.isnan(got), nan):
        return math.inf
    keep = ~nan if skip is None else ~nan & ~skip
    return worst((got[keep] - ref[keep]).abs(), bar[keep]) if bool(keep.any()) else 0.0


# ------------------------------------------------------------------------------------------------------------- LayerNorm
# kind: std (x = 2 randn + 0.3) | offset (x = 300 + randn) | narrow (x = 0.3 + 0.05 randn: var = 2.5e-3, where eps = 1e-6 is
# 4e-4 of the variance and its place in the formula shows) | bwd (backward only)
LN = namedtuple("LN", "M D dtype kind what", defaults=("std", ""))
LN_SHAPES = ((5, 4, "one live lane"), (9, 64, "quarter slot, M % 4"), (6, 260, "NV2 ragged"), (7, 1284, "NV6 one lane in last slot"),
             (5, 1536, "NV6 full"), (5, 1792, "NV7"), (6, 2048, "NV8 limit"))
LN_CASES = [LN(M, D, dt, "std", what) for M, D, what in LN_SHAPES for dt in (F32, BF, F16)]
LN_CASES.append(LN(37, 768, F32, "offset", "offset 300"))
LN_CASES.append(LN(8, 64, F32, "narrow", "eps visible"))
LN_CASES.append(LN(2309, 192, BF, "bwd", "rounds 2, nblk 289, waves of 2 and 3 rows"))
LN_FWD_VARIANTS = ("y+y32", "y32only")
LN_BWD_VARIANTS = ("gin-glp", "nogin-glp", "gin-noglp", "nogin-noglp", "dy32-gin-glp")
LN_REDUCE_SHAPE = (70, 100)   # nblk > 32 with two row groups of 3 rows, D % 32 != 0
LN_REFUSED_D = (2052, 6)


def ln_id(c):
    return f"ln-{c.M}x{c.D}-{DT[c.dtype]}-{c.kind}"


def ln_fwd_cases():
    return [(c, v) for c in LN_CASES if c.kind != "bwd" for v in LN_FWD_VARIANTS]


def ln_bwd_cases():
    return [(c, v) for c in LN_CASES for v in LN_BWD_VARIANTS if not (v.startswith("dy32") and c.dtype == F32)]


def ln_bwd_blocks(M):
    """layernorm.hip skyemb_layernorm_bwd_blocks."""
    nb = max((M + 3) // 4, 1)
    rounds = (nb + LN_BWD_CAP - 1) // LN_BWD_CAP
    return (nb + rounds - 1) // rounds


def ln_inputs(c):
    """fp32 CPU operands of case c: x, gamma, beta (signed), dy32, dy (rounded to c.dtype), g_in, and the fp32 mean / rstd the
    backward reads (the forward emulation's)."""
    g = torch.Generator().manual_seed(1000 * c.M + c.D)
    z = torch.randn(c.M, c.D, generator=g)
    x = 300.0 + z if c.kind == "offset" else (0.3 + 0.05 * z if c.kind == "narrow" else z * 2 + 0.3)
    t = {"x": x, "gamma": torch.randn(c.D, generator=g), "beta": torch.randn(c.D, generator=g)}
    t["dy32"] = torch.randn(c.M, c.D, generator=g)
    t["dy"] = t["dy32"].to(c.dtype).float()
    t["g_in"] = torch.randn(c.M, c.D, generator=g)
    e = ln_fwd_emulate(t, c.dtype)
    t["mean"], t["rstd"] = e["mean"].float(), e["rstd"].float()
    return t


def ln_fwd_reference(t, eps=LN_EPS):
    """-> ({mean, rstd, y} fp64, {mean, rstd, y} fp32-arithmetic error terms)."""
    x, gam, bet = t["x"].double(), t["gamma"].double(), t["beta"].double()
    D = x.shape[1]
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    w = var + f32(eps)
    rstd = w.rsqrt()
    y = d * rstd * gam + bet
    e_mean = D * U32 * x.abs().mean(1, keepdim=True)
    e_c = e_mean + U32 * (x.abs() + mean.abs())
    e_var = (2 * d.abs() * e_c + e_c * e_c).mean(1, keepdim=True) + (D + 2) * U32 * var
    e_w = e_var + U32 * w
    e_rstd = rstd * (e_w / (2 * (w - e_w).clamp_min(1e-300)) + E_RSQ)
    tt = (d * rstd * gam).abs()
    e_y = gam.abs() * (rstd * e_c + d.abs() * e_rstd) + 3 * U32 * tt + U32 * bet.abs()
    return {"mean": mean[:, 0], "rstd": rstd[:, 0], "y": y}, {"mean": e_mean[:, 0], "rstd": e_rstd[:, 0], "y": e_y}


def ln_fwd_bars(ref, err, dtype):
    return {"mean": stored(ref["mean"], err["mean"], F32), "rstd": stored(ref["rstd"], err["rstd"], F32),
            "y32": stored(ref["y"], err["y"], F32), "y": stored(ref["y"], err["y"], dtype)}


LN_FWD_MUTANTS = ("unbiased", "eps_outside", "ragged")


def ln_fwd_emulate(t, dtype, eps=LN_EPS, mutant=None):
    """layernorm.hip ln_fwd_kernel in torch fp32 (per-row sums in torch's order).  mutant: unbiased variance | eps outside the
    square root | the last float4 of a row left out of the statistics."""
    x, gam, bet = t["x"], t["gamma"], t["beta"]
    D = x.shape[1]
    xs = x[:, :D - 4] if mutant == "ragged" else x
    mean = xs.sum(1, keepdim=True) / D
    c = x - mean
    cs = c[:, :D - 4] if mutant == "ragged" else c
    var = (cs * cs).sum(1, keepdim=True) / (D - 1 if mutant == "unbiased" else D)
    e = torch.tensor(eps, dtype=F32)
    rstd = 1.0 / (var.sqrt() + e) if mutant == "eps_outside" else (var + e).rsqrt()
    y32 = c * rstd * gam + bet
    return {"mean": mean[:, 0].double(), "rstd": rstd[:, 0].double(), "y32": y32.double(), "y": round_to(y32, dtype).double()}


def ln_block_of_row(M, nblk, contiguous=False):
    r = torch.arange(M)
    if contiguous:
        rounds = ((M + 3) // 4 + nblk - 1) // nblk
        return (r // 4) // rounds
    return (r // 4) % nblk


def ln_bwd_reference(t, variant, nblk):
    """-> ({g_out, part [2, nblk, D], dgamma, dbeta} fp64, error terms of the same names) for a backward variant (dy fp32 for
    "dy32", g_in absent for "nogin")."""
    x, gam = t["x"].double(), t["gamma"].double()
    dy = (t["dy32"] if variant.startswith("dy32") else t["dy"]).double()
    mu, rs = t["mean"].double()[:, None], t["rstd"].double()[:, None]
    gin = None if "nogin" in variant else t["g_in"].double()
    M, D = x.shape
    xh = (x - mu) * rs
    a = dy * gam
    m1 = a.mean(1, keepdim=True)
    m2 = (a * xh).mean(1, keepdim=True)
    g = rs * (a - m1 - xh * m2)
    T = a.abs() + m1.abs() + (xh * m2).abs()
    e_m1 = (D + 1) * U32 * a.abs().mean(1, keepdim=True)
    e_m2 = (D + 4) * U32 * (a * xh).abs().mean(1, keepdim=True)
    e_g = rs * (e_m1 + xh.abs() * e_m2 + 5 * U32 * T)
    if gin is not None:
        g = g + gin
        e_g = e_g + U32 * (rs * T + gin.abs())
    blk = ln_block_of_row(M, nblk)
    R = torch.zeros(nblk, dtype=torch.float64).index_add_(0, blk, torch.ones(M, dtype=torch.float64))[:, None]
    acc = lambda v: torch.zeros(nblk, D, dtype=torch.float64).index_add_(0, blk, v)
    part = torch.stack([acc(dy * xh), acc(dy)])
    mag = torch.stack([acc((dy * xh).abs()), acc(dy.abs())])
    e_part = torch.stack([(R + 6) * U32 * mag[0], (R + 3) * U32 * mag[1]])
    e_red = e_part.sum(1) + nblk * U32 * mag.sum(1)
    return ({"g_out": g, "part": part, "dgamma": part[0].sum(0), "dbeta": part[1].sum(0)},
            {"g_out": e_g, "part": e_part, "dgamma": e_red[0], "dbeta": e_red[1]})


def ln_bwd_bars(ref, err, dtype):
    return {"g_out": stored(ref["g_out"], err["g_out"], F32), "g_lp": stored(ref["g_out"], err["g_out"], dtype),
            "part": stored(ref["part"], err["part"], F32), "dgamma": stored(ref["dgamma"], err["dgamma"], F32),
            "dbeta": stored(ref["dbeta"], err["dbeta"], F32)}


LN_BWD_MUTANTS = ("m2_nogamma", "contiguous")


def ln_bwd_emulate(t, variant, nblk, dtype, mutant=None):
    """ln_bwd_body.h in torch fp32.  mutant: m2 without gamma | the rows of a block contiguous instead of strided."""
    x, gam = t["x"], t["gamma"]
    dy = t["dy32"] if variant.startswith("dy32") else t["dy"]
    mu, rs = t["mean"][:, None], t["rstd"][:, None]
    M, D = x.shape
    xh = (x - mu) * rs
    a = dy * gam
    m1 = a.sum(1, keepdim=True) / D
    m2 = ((dy if mutant == "m2_nogamma" else a) * xh).sum(1, keepdim=True) / D
    g = rs * (a - m1 - xh * m2)
    if "nogin" not in variant:
        g = g + t["g_in"]
    blk = ln_block_of_row(M, nblk, contiguous=mutant == "contiguous")
    acc = lambda v: torch.zeros(nblk, D).index_add_(0, blk, v)
    part = torch.stack([acc(dy * xh), acc(dy)])
    return {"g_out": g.double(), "g_lp": round_to(g, dtype).double(), "part": part.double(), "dgamma": part[0].sum(0).double(),
            "dbeta": part[1].sum(0).double()}


def ln_reduce_inputs():
    nblk, D = LN_REDUCE_SHAPE
    return torch.randn(nblk, D, generator=torch.Generator().manual_seed(70100)) * torch.logspace(-2, 2, D)[None, :]


def colsum_reference(X):
    """fp64 column sums of X [M, N] and the bar M u sum|X| + 2^-126."""
    Xd = X.double()
    return Xd.sum(0), Xd.shape[0] * U32 * Xd.abs().sum(0) + TINY


# ------------------------------------------------------------------------------------------------------------- AdamW
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.05, step=3)
AW = namedtuple("AW", "n n_decay lp gdt hyper grad_scale zero_grad what", defaults=(False, 1.0, False, ""))
_S = 4096 * 256               # float4 groups one pass of the capped grid covers
AW_CASES = [AW(8, 0, None, F32, what="no shadow, nothing decayed"),
            AW(4104, 1001, BF, F32, hyper=True, what="boundary inside a float4, device scalars"),
            AW(4104, 4104, F16, F16, grad_scale=2.0 ** -16, zero_grad=True, what="all decayed, fp16 grads zeroed"),
            AW(4104, 1003, F32, BF, zero_grad=True, what="fp32 shadow, bf16 grads zeroed"),
            AW(4 * (3 * _S + 37), 4 * (2 * _S) + 4 * _S + 2, BF, F32, what="capped grid: u = 1, two trips")]


def aw_id(c):
    return f"adamw-n{c.n}-d{c.n_decay}-lp{DT[c.lp]}-g{DT[c.gdt]}" + ("-hyper" if c.hyper else "") + ("-zero" if c.zero_grad else "")


def aw_scalars():
    a = ADAM
    return dict(lr=a["lr"], bc1=1 - a["beta1"] ** a["step"], bc2=1 - a["beta2"] ** a["step"], beta1=a["beta1"], beta2=a["beta2"],
                eps=a["eps"], wd=a["wd"])


def aw_inputs(c):
    """fp32 CPU buffers p, g (representable in c.gdt), m, v as in test_adamw, with exact zeros and a few 1e-20 among the gradients
    and exact zeros in v -- some of them where the gradient is zero or tiny too, so that denom = eps."""
    gen = torch.Generator().manual_seed(5 + c.n % 1000)
    n = c.n
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1
    m, v = torch.randn(n, generator=gen) * 0.01, torch.rand(n, generator=gen) * 0.01
    g[::7] = 0.0
    g[3::50] = 1e-20
    v[::21] = 0.0             # (every third of them under a zero gradient: v' = 0)
    v[5::33] = 0.0
    v[3::100] = 0.0           # (under a 1e-20 gradient)
    g = (g / c.grad_scale).to(c.gdt).float()
    return {"p": p, "g": g, "m": m, "v": v}


def aw_reference(t, c):
    """-> ({p, m, v} fp64, error terms) on the device of t."""
    s = {k: f32(x) for k, x in aw_scalars().items()}
    gs = f32(c.grad_scale)
    p, g, m, v = (t[k].double() for k in ("p", "g", "m", "v"))
    dec = torch.arange(p.numel(), device=p.device) < c.n_decay
    gj = g * gs
    pd = torch.where(dec, p * (1.0 - s["lr"] * s["wd"]), p)
    mn = s["beta1"] * m + (1.0 - s["beta1"]) * gj
    vn = s["beta2"] * v + (1.0 - s["beta2"]) * gj * gj
    sb = math.sqrt(s["bc2"])
    sq = vn.sqrt()
    denom = sq / sb + s["eps"]
    r = mn / denom
    step = s["lr"] / s["bc1"]
    pn = pd - step * r
    e_pd = torch.where(dec, 3 * U32 * p.abs(), torch.zeros_like(p))
    e_m = 4 * U32 * ((s["beta1"] * m).abs() + ((1.0 - s["beta1"]) * gj).abs())
    e_v = 6 * U32 * vn + TINY
    e_s = e_v / (sq + (vn - e_v).clamp_min(0).sqrt()) + E_SQRT * sq
    e_den = e_s / sb + (E_SQRT + E_DIV) * sq / sb + U32 * denom
    e_r = e_m / denom + r.abs() * (e_den / denom + E_DIV)
    e_p = e_pd + step * (e_r + E_DIV * r.abs()) + U32 * pn.abs()
    return {"p": pn, "m": mn, "v": vn}, {"p": e_p, "m": e_m, "v": e_v}


def aw_bars(ref, err, c):
    b = {k: stored(ref[k], err[k], F32) for k in ("p", "m", "v")}
    if c.lp is not None:
        b["p_lp"] = stored(ref["p"], err["p"], c.lp)
    return b


AW_MUTANTS = ("decay_quad", "bc2_nosqrt", "decay_after")


def aw_emulate(t, c, mutant=None):
    """adamw_math.h in torch fp32 (multiplies and adds unfused).  mutant: the decay boundary rounded down to a multiple of 4 |
    bc2 not square-rooted | weight decay applied after the moment update."""
    s = {k: torch.tensor(x, dtype=F32) for k, x in aw_scalars().items()}
    gs = torch.tensor(c.grad_scale, dtype=F32)
    p, g, m, v = t["p"], t["g"], t["m"], t["v"]
    nd = c.n_decay // 4 * 4 if mutant == "decay_quad" else c.n_decay
    dec = torch.arange(p.numel()) < nd
    one = torch.tensor(1.0, dtype=F32)
    decay = one - s["lr"] * s["wd"]
    step = s["lr"] / s["bc1"]
    gj = g * gs
    mn = m * s["beta1"] + gj * (one - s["beta1"])
    vn = v * s["beta2"] + (gj * gj) * (one - s["beta2"])
    denom = vn.sqrt() / (s["bc2"] if mutant == "bc2_nosqrt" else s["bc2"].sqrt()) + s["eps"]
    if mutant == "decay_after":
        pn = p - step * (mn / denom)
        pn = torch.where(dec, pn * decay, pn)
    else:
        pn = torch.where(dec, p * decay, p) - step * (mn / denom)
    out = {"p": pn.double(), "m": mn.double(), "v": vn.double()}
    if c.lp is not None:
        out["p_lp"] = round_to(pn, c.lp).double()
    return out


# ------------------------------------------------------------------------------------------------------------- masked patch loss
PIXEL_MEAN, PIXEL_STD = 0.1, 1.3
# lp: the dtype of dpred (None: `dtype` F32 and dpred32 = NULL, the fp32 gradient goes to dpred); mask: rand (70 % masked) | one
# (only the patch of two unequal finite pixels: N = 2, where the 1e-5 of the denominator is not lost in the bar)
LS = namedtuple("LS", "B C H p extra lp l1 dscale mask what", defaults=(1.0, "rand", ""))
LS_GEOM = ((2, 12, 32, 16, 1, BF, 1.0, "pv 3072: last cached size"), (2, 13, 32, 16, 2, F16, 1.0, "pv 3328: uncached in both passes"),
           (5, 2, 32, 4, 0, None, 2.0 ** 10, "B L 320 > 256 in finalize, dscale 2^10"))
LS_CASES = [LS(B, C, H, p, ex, lp, l1, ds, "rand", what) for B, C, H, p, ex, lp, ds, what in LS_GEOM for l1 in (False, True)]
LS_CASES += [LS(5, 2, 32, 4, 0, None, l1, 1.0, "one", "a single masked patch of two finite pixels") for l1 in (False, True)]


def ls_id(c):
    return (f"loss-B{c.B}C{c.C}H{c.H}p{c.p}-x{c.extra}-{DT[c.lp] if c.lp else 'f32only'}-{'l1' if c.l1 else 'mse'}"
            + (f"-ds{int(c.dscale)}" if c.dscale != 1 else "") + ("" if c.mask == "rand" else "-" + c.mask))


def patchify(imgs, p):
    """[B, C, H, W] -> [B, L, p p C], element (py p + px) C + c (loss.hip target_elem)."""
    B, C, H, W = imgs.shape
    x = imgs.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1)
    return x.reshape(B, (H // p) * (W // p), p * p * C)


def unpatchify(x, C, H, p):
    B = x.shape[0]
    g = H // p
    return x.reshape(B, g, g, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, H)


def ls_inputs(c, seed=0):
    """imgs with a NaN plane and a NaN rectangle (as test_masked_patch_loss), the last patch of image 0 NaN but for two unequal
    pixels, the last patch of image 1 NaN but for two EQUAL pixels under a zero prediction; mask; pred [B, L + extra, pv]."""
    B, C, H, p = c.B, c.C, c.H, c.p
    L, pv = (H // p) ** 2, C * p * p
    g = torch.Generator().manual_seed(100 * H + C + 7 * seed)
    x = torch.randn(B, C, H, H, generator=g)
    x[1, C - 1] = float("nan")
    x[0, 0, 3:9, 5:20] = float("nan")
    tp = patchify(x, p).clone()
    two = tp[0, L - 1, [5, pv - 3]].clone()
    tp[0, L - 1] = float("nan")
    tp[0, L - 1, [5, pv - 3]] = torch.tensor([0.75, -1.5]) if bool(torch.isnan(two).any()) else two
    tp[1, L - 1] = float("nan")
    tp[1, L - 1, [2, pv - 6]] = 0.625
    x = unpatchify(tp, C, H, p).contiguous()
    mask = (torch.rand(B, L, generator=g) < 0.7).float()
    if c.mask == "one":
        mask.zero_()
    else:
        mask[0, 0], mask[1, L - 1] = 0.0, 1.0
    mask[0, L - 1] = 1.0
    pred = torch.randn(B, L + c.extra, pv, generator=g)
    if c.l1:
        # the sign of pred - tn is ill-conditioned within the error bound of 0 (up to ~3e-4 at pv = 3072, where two or three of 30 000
        # random elements fall): predictions closer than L1_MARGIN to the fp64 target are moved out to that distance
        tn = ls_targets(x.double(), p)
        near = (pred[:, c.extra:].double() - tn).abs() < L1_MARGIN          # (False where the target is NaN)
        side = torch.where(pred[:, c.extra:].double() >= tn, 1.0, -1.0)
        pred[:, c.extra:] = torch.where(near, (tn + L1_MARGIN * side).float(), pred[:, c.extra:])
    pred[1, c.extra + L - 1, [2, pv - 6]] = 0.0
    return {"imgs": x, "mask": mask, "pred": pred}


L1_MARGIN = 0.01


def ls_targets(imgs64, p):
    """fp64 normalised targets tn [B, L, pv] of the statement (NaN where the pixel is)."""
    tt = (patchify(imgs64, p) - f32(PIXEL_MEAN)) / f32(PIXEL_STD)
    ok = ~torch.isnan(tt)
    n = ok.sum(-1, keepdim=True).double()
    mu = torch.where(ok, tt, torch.zeros_like(tt)).sum(-1, keepdim=True) / n
    var = (torch.where(ok, tt - mu, torch.zeros_like(tt)) ** 2).sum(-1, keepdim=True) / n
    return (tt - mu) / (var + f32(1e-6)).sqrt()


def ls_reference(t, c):
    """-> ({loss [1], ws [B L, 4], dpred [B, L + extra, pv]} fp64, error terms, ill [B, L + extra, pv]: elements whose L1 sign is
    ill-conditioned)."""
    B, C, H, p, ex = c.B, c.C, c.H, c.p, c.extra
    L, pv = (H // p) ** 2, C * p * p
    tt = (patchify(t["imgs"].double(), p) - f32(PIXEL_MEAN)) / f32(PIXEL_STD)
    pred = t["pred"].double()[:, ex:]
    m = t["mask"].double()
    ok = ~torch.isnan(tt)
    z = lambda v: torch.where(ok, v, torch.zeros_like(v))
    n = ok.sum(-1, keepdim=True).double()
    mu = z(tt).sum(-1, keepdim=True) / n
    d = z(tt - mu)
    var = (d * d).sum(-1, keepdim=True) / n
    w = var + f32(1e-6)
    istd = 1.0 / w.sqrt()
    tn = d * istd
    diff = z(tn - pred)
    elem = diff.abs() if c.l1 else diff * diff
    Sp = elem.sum(-1)
    S, N = (m * Sp).sum(), (m * n[..., 0]).sum()
    numel = f32(float(B * L * pv))
    scale = N / numel * numel
    den = scale + f32(1e-5)
    loss = S / den
    inv = f32(c.dscale) / den
    g = m[..., None] * ok * (-torch.sign(diff) if c.l1 else -2.0 * diff) * inv
    dpred = torch.cat([torch.zeros(B, ex, pv, dtype=torch.float64), g], 1)
    ws = torch.stack([Sp, n[..., 0], mu[..., 0], istd[..., 0]], -1) * m[..., None]
    ws = torch.where(m[..., None] == 0, torch.zeros_like(ws), ws).reshape(B * L, 4)
    # error terms
    ta = z(tt).abs()
    e_t = (U32 + E_DIV) * ta
    e_mu = e_t.sum(-1, keepdim=True) / n + (n + 5) * U32 * ta.sum(-1, keepdim=True) / n
    e_d = z(e_t + e_mu + U32 * (ta + mu.abs()))
    e_var = (2 * d.abs() * e_d + e_d * e_d).sum(-1, keepdim=True) / n + (n + 6) * U32 * var
    e_w = e_var + U32 * w
    e_istd = istd * (e_w / (2 * (w - e_w).clamp_min(1e-300)) + E_SQRT + E_DIV)
    e_diff = z(istd * e_d + d.abs() * e_istd + U32 * tn.abs() + U32 * diff.abs())
    e_elem = e_diff if c.l1 else 2 * diff.abs() * e_diff + e_diff * e_diff + U32 * diff * diff
    e_Sp = e_elem.sum(-1) + pv * U32 * Sp
    e_S = (m * e_Sp).sum() + B * L * U32 * S
    e_loss = e_S / den + loss.abs() * (2 * E_DIV + 2 * U32)
    if c.l1:
        e_g = g.abs() * (2 * E_DIV + 3 * U32)
    else:
        e_g = m[..., None] * ok * 2 * e_diff * inv + g.abs() * (2 * E_DIV + 4 * U32)
    zero = torch.zeros(B * L, dtype=torch.float64)
    mm = m.reshape(-1)
    e_ws = torch.stack([e_Sp.reshape(-1), zero, e_mu.reshape(-1), e_istd.reshape(-1)], -1) * mm[:, None]
    e_ws = torch.where(mm[:, None] == 0, torch.zeros_like(e_ws), e_ws)
    ill_p = (m[..., None] * ok).bool() & (diff != 0) & (diff.abs() <= e_diff) if c.l1 else torch.zeros_like(ok)
    pad = torch.zeros(B, ex, pv, dtype=torch.bool)
    return ({"loss": loss.reshape(1), "ws": ws, "dpred": dpred},
            {"loss": e_loss.reshape(1), "ws": e_ws, "dpred": torch.cat([torch.zeros(B, ex, pv, dtype=torch.float64), e_g], 1)},
            torch.cat([pad, ill_p], 1))


def ls_bars(ref, err, c):
    b = {"loss": stored(ref["loss"], err["loss"], F32), "ws": stored(ref["ws"], err["ws"], F32) - TINY * (ref["ws"] == 0),
         "dpred32": stored(ref["dpred"], err["dpred"], F32) - TINY * (ref["dpred"] == 0)}
    if c.lp is not None:
        lp = stored(ref["dpred"], err["dpred"], c.lp)
        b["dpred"] = torch.where(ref["dpred"] == 0, torch.zeros_like(lp), lp)      # (a zero the kernel must write as a zero)
    return b


LS_MUTANTS = ("var_all", "den_cnt", "sign0")


def ls_emulate(t, c, mutant=None):
    """loss.hip in torch fp32 (per-patch sums in torch's order).  mutant: the variance over all pv elements | the denominator cnt
    | sign(0) = 1 in the L1 gradient."""
    B, C, H, p, ex = c.B, c.C, c.H, c.p, c.extra
    L, pv = (H // p) ** 2, C * p * p
    c32 = lambda v: torch.tensor(v, dtype=F32)
    tt = (patchify(t["imgs"], p) - c32(PIXEL_MEAN)) / c32(PIXEL_STD)
    pred, m = t["pred"][:, ex:], t["mask"]
    ok = ~torch.isnan(tt)
    z = lambda v: torch.where(ok, v, torch.zeros_like(v))
    n = ok.sum(-1, keepdim=True).float()
    mu = z(tt).sum(-1, keepdim=True) / n
    d = z(tt - mu)
    var = (d * d).sum(-1, keepdim=True) / (float(pv) if mutant == "var_all" else n)
    istd = 1.0 / (var + c32(1e-6)).sqrt()
    tn = d * istd
    diff = z(tn - pred)
    Sp = (diff.abs() if c.l1 else diff * diff).sum(-1)
    S, N = (m * Sp).sum(), (m * n[..., 0]).sum()
    numel = c32(float(B * L * pv))
    den = N if mutant == "den_cnt" else N / numel * numel + c32(1e-5)
    loss = S / den
    inv = (1.0 / den) * c32(c.dscale)
    dd = z(pred - tn)
    if c.l1:
        sg = torch.where(dd >= 0, torch.ones_like(dd), -torch.ones_like(dd)) if mutant == "sign0" else torch.sign(dd)
    else:
        sg = 2.0 * dd
    g = torch.cat([torch.zeros(B, ex, pv), m[..., None] * ok * sg * inv], 1)
    ws = torch.stack([Sp, n[..., 0], mu[..., 0], istd[..., 0]], -1)
    ws = torch.where(m[..., None] == 0, torch.zeros_like(ws), ws).reshape(B * L, 4)
    out = {"loss": loss.reshape(1).double(), "ws": ws.double(), "dpred32": g.double()}
    if c.lp is not None:
        out["dpred"] = round_to(g, c.lp).double()
    return out


# ------------------------------------------------------------------------------------------------------------- reductions, copies
CS = namedtuple("CS", "M N ldx dtype")
CS_CASES = [CS(M, N, ldx, dt) for M, N, ldx in ((3, 70, 70), (301, 200, 208), (1030, 64, 64)) for dt in (F32, BF, F16)]
RS = namedtuple("RS", "B L D sel")      # n_rows = B L of [B, L + 1, D] (row0 = 1, inner = L, outer_stride = L + 1): the decoder use
RS_CASES = [RS(B, L, D, sel) for B, L in ((4, 50), (7, 100), (11, 100)) for D in (32, 300) for sel in ("none", "rand", "zero")]
GATHER_CASES = [("f32+bf16", BF, True), ("f32+f16", F16, True), ("bf16only", BF, False), ("f32only", None, True)]
GATHER_D, FILL_D = 1028, 1028
CAST_N = (4 * (4096 * 256 + 5), 4)


def cs_id(c):
    return f"colsum-{c.M}x{c.N}-ld{c.ldx}-{DT[c.dtype]}"


def rs_id(c):
    return f"rowsum-n{c.B * c.L}-D{c.D}-sel{c.sel}"


def cs_inputs(c):
    g = torch.Generator().manual_seed(c.M + c.N)
    return (torch.randn(c.M, c.N, generator=g) * torch.logspace(-1, 1, c.N)[None, :]).to(c.dtype).float()


def rs_inputs(c):
    g = torch.Generator().manual_seed(c.B * c.L + c.D)
    x = torch.randn(c.B, c.L + 1, c.D, generator=g)
    sel = {"none": None, "rand": (torch.rand(c.B * c.L, generator=g) < 0.6).float(), "zero": torch.zeros(c.B * c.L)}[c.sel]
    return x, sel


def rs_reference(x, sel, nblk=256):
    """-> ({partial [256, D], out [D]} fp64, bars)."""
    B, L1, D = x.shape
    rows = x[:, 1:].reshape(-1, D).double()
    if sel is not None:
        rows = rows * (sel != 0).double()[:, None]
    n = rows.shape[0]
    blk = torch.arange(n) % nblk
    part = torch.zeros(nblk, D, dtype=torch.float64).index_add_(0, blk, rows)
    mag = torch.zeros(nblk, D, dtype=torch.float64).index_add_(0, blk, rows.abs())
    per = (n + nblk - 1) // nblk
    return ({"partial": part, "out": part.sum(0)},
            {"partial": per * U32 * mag + TINY * (mag != 0), "out": (per + nblk) * U32 * mag.sum(0) + TINY * (mag.sum(0) != 0)})


def rs_emulate(x, sel, nblk=256):
    B, L1, D = x.shape
    rows = x[:, 1:].reshape(-1, D)
    if sel is not None:
        rows = rows * (sel != 0).float()[:, None]
    part = torch.zeros(nblk, D).index_add_(0, torch.arange(rows.shape[0]) % nblk, rows)
    return {"partial": part.double(), "out": part.sum(0).double()}


def cast_inputs(n):
    """fp32 values to cast: a spread of magnitudes, values that round to the 16-bit formats' infinity (fp16 above 65520, bf16
    above 3.39e38), fp16 subnormals and values below half the smallest one, signed zeros."""
    g = torch.Generator().manual_seed(n % 1000)
    x = torch.randn(n, generator=g) * torch.logspace(-9, 5, 29)[torch.arange(n) % 29]
    edge = torch.tensor([65519.9, 65520.0, -65520.0, 70000.0, 3.3895e38, 3.4e38, -3.4e38, 3.0e-5, 5.96e-8, 2.98e-8, 2.99e-8, 1e-9,
                         -0.0, 0.0, 6.1e-5, 1e-39])
    k = min(n, edge.numel())
    x[:k] = edge[:k]
    x[n - k:] = edge[:k]
    return x
