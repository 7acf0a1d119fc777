"""Float64 statement of the attention core (skyemb_mha_fwd / skyemb_mha_bwd), its elementwise error bar, a CPU emulation of the
kernels' arithmetic, and the dispatch rules that pick a kernel family.  Used by tests/test_attention_core_gpu.py and pinned on
the CPU by tests/test_attention_reference_cpu.py.

Layout: qkv [B, N, 3 H hd] (timm: qkv(x).reshape(B, N, 3, H, hd)), dout / out [B, N, H hd], dqkv like qkv.  With s = hd^-0.5,
S = s Q K^T, P = softmax_j(S), O = P V, dP = dO V^T, D_i = sum_j P_ij dP_ij, dS = P o (dP - D), dQ = s dS K, dK = s dS^T Q,
dV = P^T dO.  Every statement is computed in fp64 from the operands exactly as the kernel read them (16-bit values rounded).

The bar (`bar`).  u = 2^-24 is the fp32 unit roundoff; h is the unit roundoff of the stored format: 2^-8 for bf16 (8 significant
bits), 2^-11 for fp16, u for fp32.

1. Rounding of the operands the 16-bit kernels feed to the PV / dS.K MFMAs.  The MFMA kernels (packed, single-tile, strip, long)
   round every probability P_ij and every dS_ij to 16 bits exactly once (`pack_regs`, the `(lp_t)` casts) and accumulate the
   exact products of 16-bit operands in fp32.  Rounding to nearest moves an element by at most h of itself, so the PV sum moves
   by at most h sum_j P_ij |V_jd| = h M_o, and likewise h M_dv, h M_dq, h M_dk with
       M_o = P |V|,  M_dv = P^T |dO|,  M_dq = s |dS| |K|,  M_dk = s |dS|^T |Q|,  |dS| = P o (|dP| + |D|).
   dS is a difference that cancels, so its rounding is relative to those parts, not to |dS| itself.  c = 1: one rounding per
   element, and P and dS are never rounded twice.  (The fp32 LDS and streaming kernels keep P and dS in fp32 at every dtype,
   so for them this term is slack; the bar is the same for every family of a dtype.)  fp16 has subnormals below 2^-14: a
   rounded P or dS element can be off by 2^-25 in absolute terms, which adds 2^-25 sum_j |V_jd| (and 2^-25 sum_i |dO_id|,
   s 2^-25 sum_j |K_jd|, s 2^-25 sum_i |Q_id|).  In every format a P below fp32's normal range (2^-126, a logit gap past 87)
   may be flushed to zero: 2^-126 per P element, and 2^-126 (|dP_ij| + |D_i|) per dS element, through the same sums.

2. fp32 arithmetic before that rounding (this is what carries the fp32 bar).  A dot product of length n accumulated in fp32
   errs by at most n u times the sum of the magnitudes of its terms (the standard gamma_n bound, products exact or rounded
   once).  So each score errs by
       dS_ij <= hd u s sum_d |Q_id||K_jd|  +  3 u (|S_ij| + |m_i|)
   (the second term: the scale multiply and the argument S_ij - m_i of the exponential, m_i the row max).  P_ij =
   exp(S_ij - m_i) / sum_k exp(S_ik - m_i) inherits the score errors as RELATIVE error: its own, minus the P-weighted mean of
   the row's (the normaliser), plus (N + 4) u for the sum, the exponential and the division:
       rho_ij = dS_ij + sum_k P_ik dS_ik + (N + 4) u.
   This is the fp32 bar's main term for large logits: the spiked input of test_attention_long_gpu.py has |S| ~ 60, a score
   rounding of ~60 u = 3.6e-6 that P and dS carry as relative error -- the 2e-5 relative-L2 allowance it needed -- while
   the worst-case bound here is hd u s |q||k| ~ hd 60 u.  The sum over the N tokens that follows adds (N + 4) u of the
   magnitude once more.  dS_ij = P_ij (dP_ij - D_i) with dP_ij off by hd u sum_d |dO_id||V_jd| and D_i off by
       eD_i = sum_j P_ij ((rho_ij + (N + 4) u) |dP_ij| + hd u sum_d |dO_id||V_jd|),
   so  e_dS_ij = (rho_ij + 2u) |dS|_ij + P_ij (hd u sum_d |dO_id||V_jd| + eD_i).  Pushed through the last contraction these
   give R_o = (P o (rho + g)) |V|, R_dv = (P o (rho + g))^T |dO|, R_dq = s (e_dS + g |dS|) |K|, R_dk = s (e_dS + g |dS|)^T |Q|,
   g = (N + 4) u.

3. The output is rounded once to the stored format: at most h of the fp32 value y32, so with r the fp64 statement
       |y - r| <= h |y32| + |y32 - r| <= h |r| + (1 + h) |y32 - r|,
       bar = h |r| + (1 + h) (h_op M + (1 + h_op) R + floor),
   h_op = h for 16-bit (item 1), 0 for fp32; floor = the subnormal and flush terms of item 1 plus, for the output itself,
   2^-25 in fp16 (its subnormal rounding) or 2^-126 (a flushed fp32 / bf16 subnormal).

The fp32 terms are worst-case bounds (every rounding in one direction); real fp32 sums err like sqrt(n) u, so in fp32 the
emulation's worst err/bar stays near 0.01.  In 16 bit items 1 and 3 dominate and the emulation's worst err/bar lies in
[0.2, 1] (both pinned by tests/test_attention_reference_cpu.py).  What the kernels achieve on the GPU is recorded by
tests/test_attention_core_gpu.py (record_parity "attention_core"), not assumed here.
"""
import math

import torch

U32 = 2.0 ** -24
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: U32}
F16_SUB = 2.0 ** -25          # half the smallest fp16 subnormal: the absolute rounding error below 2^-14
TINY = 2.0 ** -126            # fp32 / bf16 values below the normal range may be flushed to zero
NAMES = ("out", "dq", "dk", "dv")


def heads(qkv, dout, H, hd):
    """qkv [B, N, 3 H hd], dout [B, N, H hd] -> q, k, v, do as fp64 [B, H, N, hd]."""
    B, N, _ = qkv.shape
    t = qkv.double().reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2], dout.double().reshape(B, N, H, hd).transpose(1, 2)


def flat(x):
    """[B, H, N, hd] -> [B, N, H hd]."""
    B, H, N, hd = x.shape
    return x.transpose(1, 2).reshape(B, N, H * hd)


def core(qkv, dout, H, hd):
    """fp64 out, dq, dk, dv ([B, N, H hd] each) and, per output, the terms of the module docstring's bar: the magnitude M,
    the fp32 term R, and the sums the per-element floors of item 1 multiply ("sub": sum |V|, ...; "flush": the extra
    (|dP| + |D|) factor of a flushed P in dS): {"ref": {name: t}, "mag": ..., "r32": ..., "sub": ..., "flush": ...}."""
    q, k, v, do = heads(qkv, dout, H, hd)
    N = q.shape[2]
    s = hd ** -0.5
    S = s * q @ k.transpose(-2, -1)
    m = S.amax(-1, keepdim=True)
    P = torch.softmax(S, -1)
    dP = do @ v.transpose(-2, -1)
    D = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - D)
    ref = {"out": P @ v, "dq": s * dS @ k, "dk": s * dS.transpose(-2, -1) @ q, "dv": P.transpose(-2, -1) @ do}
    aq, ak, av, ado = q.abs(), k.abs(), v.abs(), do.abs()
    mag_ds = P * (dP.abs() + D.abs())
    mag = {"out": P @ av, "dq": s * mag_ds @ ak, "dk": s * mag_ds.transpose(-2, -1) @ aq, "dv": P.transpose(-2, -1) @ ado}
    g = (N + 4) * U32
    e_s = hd * U32 * s * (aq @ ak.transpose(-2, -1)) + 3 * U32 * (S.abs() + m.abs())
    rho = e_s + (P * e_s).sum(-1, keepdim=True) + g
    e_dp = hd * U32 * (ado @ av.transpose(-2, -1))
    e_d = (P * ((rho + g) * dP.abs() + e_dp)).sum(-1, keepdim=True)
    e_ds = (rho + 2 * U32) * mag_ds + P * (e_dp + e_d) + g * mag_ds
    pr = P * (rho + g)
    r32 = {"out": pr @ av, "dq": s * e_ds @ ak, "dk": s * e_ds.transpose(-2, -1) @ aq, "dv": pr.transpose(-2, -1) @ ado}
    ones = torch.ones_like(q)
    sub = {"out": ones * av.sum(2, keepdim=True), "dq": s * ones * ak.sum(2, keepdim=True),
           "dk": s * ones * aq.sum(2, keepdim=True), "dv": ones * ado.sum(2, keepdim=True)}
    ddp = dP.abs() + D.abs()
    flush = {"out": torch.zeros_like(q), "dq": s * ddp @ ak, "dk": s * ddp.transpose(-2, -1) @ aq, "dv": torch.zeros_like(q)}
    return {key: {n: flat(d[n]) for n in NAMES}
            for key, d in (("ref", ref), ("mag", mag), ("r32", r32), ("sub", sub), ("flush", flush))}


def bar(ref, mag, r32, sub, flush, dtype):
    """Elementwise bound on |kernel - ref| for an output stored in `dtype` (module docstring, item 3)."""
    h = UNIT[dtype]
    h_op = 0.0 if dtype == torch.float32 else h
    tiny = F16_SUB if dtype == torch.float16 else TINY
    floor = (tiny + TINY) * sub + TINY * flush + tiny
    return h * ref.abs() + (1 + h) * (h_op * mag + (1 + h_op) * r32 + floor)


def bars(c, dtype):
    """{name: bar} for a core() result."""
    return {n: bar(c["ref"][n], c["mag"][n], c["r32"][n], c["sub"][n], c["flush"][n], dtype) for n in NAMES}


def round_to(x, dtype, rounding="rne"):
    """fp32 x rounded to `dtype` (returned as fp32): to nearest even, or toward zero ("trunc")."""
    if dtype == torch.float32:
        return x
    y = x.to(dtype)
    if rounding == "trunc":
        over = y.float().abs() > x.abs()
        bits = y.view(torch.int16)
        bits[over] -= 1               # sign-magnitude: one step down in the magnitude field, either sign
        y = bits.view(dtype)
    return y.float()


def emulate(qkv, dout, H, hd, dtype, rounding="rne"):
    """The 16-bit MFMA kernels' arithmetic on the CPU: fp32 scores and softmax, P and dS rounded to `dtype` by `rounding`, fp32
    accumulation, each output rounded to nearest once.  For fp32 nothing is rounded but the fp32 arithmetic itself.  Its only
    purpose is to test the bar without a GPU.  Returns {name: fp64 tensor [B, N, H hd]}."""
    B, N, _ = qkv.shape
    t = qkv.float().reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    do = dout.float().reshape(B, N, H, hd).transpose(1, 2)
    s = float(torch.tensor(hd, dtype=torch.float32).rsqrt())
    P = torch.softmax(s * (q @ k.transpose(-2, -1)), -1)
    dP = do @ v.transpose(-2, -1)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    p16, ds16 = round_to(P, dtype, rounding), round_to(dS, dtype, rounding)
    res = {"out": p16 @ v, "dq": s * (ds16 @ k), "dk": s * (ds16.transpose(-2, -1) @ q), "dv": p16.transpose(-2, -1) @ do}
    return {n: flat(round_to(x, dtype).double()) for n, x in res.items()}


# ----------------------------------------------------------------------------------------------------- dispatch rules
# An independent restatement of csrc/attention_plan.h (sky_mha_plan); tests/test_attention_reference_cpu.py sweeps it against the
# library's own answer (skyemb_mha_plan), so a threshold changed on one side only fails there.
LDS_LIMIT = 160 * 1024        # MHA_LDS_LIMIT: a whole-head LDS plan past it goes to the streaming kernel
MFMA_MAX_NT = 4               # MHA_MAX_NT: strips up to 128 tokens
STREAM_MAX_HD = 512           # MHA_STREAM_MAX_HD: the streaming kernels' widest head; wider is refused


def lds_plan(N, hd, bwd):
    """sky_mha_plan, lds family: (waves per block, dynamic LDS bytes) of the whole-head LDS kernel."""
    pitch, NP = hd + 4, N + 1
    per_wave = ((4 if bwd else 3) * N * pitch + (2 if bwd else 1) * N * NP + 3) & ~3
    per = per_wave * 4
    w = min(4, max(1, 65536 // per))
    return w, per * w


def family(B, N, H, hd, dtype, bwd, mfma=True):
    """The kernel skyemb_mha_fwd (bwd=False) / skyemb_mha_bwd (bwd=True) launches for this shape.  Restates the planner,
    csrc/attention_plan.h sky_mha_plan: 16-bit at hd 32 / 64 runs on MFMA (N > 32 MAX_NT: long kernels; N > 32: strips,
    nt = ceil(N / 32); else P = 32 / N samples per tile when N <= 16, nheads = ceil(B / P) H, and one tile per workgroup while
    (nheads + 3) / 4 < 512, else WPB = 4); everything else takes the whole-head LDS plan, or the streaming kernels where
    that plan passes 160 KB.  mfma=False: SKYEMB_MHA_MFMA=0."""
    if dtype != torch.float32 and hd in (32, 64) and mfma:
        if N > 32 * MFMA_MAX_NT:
            return "mfma_long"
        if N > 32:
            return f"mfma_strip{(N + 31) // 32}"
        P = 32 // N if N <= 16 else 1
        nheads = (B + P - 1) // P * H
        one = (nheads + 3) // 4 < 512
        return f"mfma_{'packed' if P > 1 else 'single'}_wpb{1 if one else 4}"
    w, smem = lds_plan(N, hd, bwd)
    return "stream" if smem > LDS_LIMIT else f"lds_w{w}"


def switch_points(hd, bwd, n_max=400):
    """First N at which the fp32 LDS kernel runs with 3, 2, 1 waves, and the first N that streams."""
    firsts, prev = [], None
    for N in range(1, n_max):
        f = family(1, N, 1, hd, torch.float32, bwd)
        if f != prev:
            firsts.append((f, N))
            prev = f
    return dict(firsts)


def scale_pattern(B, H, exps):
    """Per (sample, head) power-of-two factors cycling through 2^e for e in exps ([B, 1, H, 1]): exact in every format."""
    idx = (torch.arange(B)[:, None] * 7 + torch.arange(H)[None, :] * 3) % len(exps)
    return torch.tensor([2.0 ** e for e in exps])[idx].reshape(B, 1, H, 1)


def worst(err, b):
    """max err / bar (inf if any error is NaN; an exact zero over a zero bar counts 0)."""
    if bool(torch.isnan(err).any()):
        return math.inf
    r = torch.where(err == 0, torch.zeros_like(err), err / b)
    return float(r.max())
