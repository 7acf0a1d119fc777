"""GPU parity of the attention core, every kernel family and dtype, ELEMENT BY ELEMENT: each case calls ops.mha_fwd and
ops.mha_bwd and holds out, dq, dk and dv to the fp64 statement and the derived bar of tests/attention_reference.py (pinned on
the CPU by tests/test_attention_reference_cpu.py, which also checks that CASES reaches every family of `ar.family`).

What a case checks besides the bar (a NaN, e.g. an element never written, fails it):
- guards: qkv and dout are views into buffers with NaN rows before and after them (a read outside the operand poisons the
  result); out and dqkv are views into buffers whose outside is a sentinel and whose inside starts as NaN (every element must
  be written, nothing outside may change);
- contrast between tiles: V and dO are scaled per (sample, head) by different powers of two (exact in every format), so a
  leak between packed samples or heads is orders of magnitude over the bar of the tile it lands in;
- repeatability: a second backward gives the same bits;
- signed bias (the "pos" cases, one per family and 16-bit dtype): V and dO drawn positive, so O and dV are sums of positive
  terms.  Rounding to nearest even is unbiased: the mean signed error of n elements is sampling noise, a few bar / sqrt(n).
  Truncating P (or dO-side P in dV) pulls every element down by ~0.7 h M on average (the mean truncation error of a 16-bit
  value is half an ulp, 0.7 h relative), about a third of the mean bar h |r| + h M = 2 h M.  BIAS = 0.1 sits between.

Range: bf16 gradients scale bit for bit with dout by 2^k (every step is linear in dout, and bf16 shares fp32's exponent
range); fp16 with dout scaled the way fp16 mode scales the loss (engine.plan_loss_scale) and a chain factor that brings the
fp16-rounded dS within a factor of two to four of 65504 may not overflow while every fp64 gradient fits in fp16.
"""
import math
import os
import subprocess
import sys
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_reference as ar
from tests.helpers import record_parity

DEV = "cuda"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {F32: "f32", BF: "bf16", F16: "f16"}
SENT = 12.5
BIAS = 0.1
# per-tile exponents of V and dO: wide in bf16, narrower in fp16 (dS ~ dO V stays far from 65504)
CONTRAST = {BF: ([-6, -3, 0, 3, 6], [4, -4, 0, 2, -2]), F16: ([-2, 0, 2, 4], [2, -2, 0, -4]), F32: ([-6, -3, 0, 3, 6], [4, -4, 0, 2, -2])}

Case = namedtuple("Case", "B N H hd dtype kind mfma", defaults=("randn", True))


def cid(c):
    return f"{DT[c.dtype]}-B{c.B}_N{c.N}_H{c.H}_hd{c.hd}" + ("" if c.kind == "randn" else "-" + c.kind) + ("" if c.mfma else "-nomfma")


def _cases():
    cs = []
    for dt in (BF, F16):
        # the shapes training runs (tools/mha_probe.py, configs/)
        for B, N, H, hd in ((256, 5, 12, 64), (64, 5, 12, 64), (256, 17, 16, 32), (256, 17, 12, 64), (128, 65, 16, 64),
                            (128, 66, 16, 64), (4, 257, 4, 64), (4, 258, 4, 64), (8, 65, 1, 512)):
            cs.append(Case(B, N, H, hd, dt))
        # packing edges: B not a multiple of 32 / N; last packs of 16 and 17 rows (NS); single tiles at 17 and 32
        for B, N, H, hd in ((33, 1, 3, 64), (49, 1, 2, 32), (17, 2, 3, 32), (11, 3, 2, 64), (7, 5, 3, 32), (6, 8, 3, 64),
                            (5, 11, 2, 32), (3, 15, 3, 64), (3, 16, 3, 32), (5, 17, 3, 64), (3, 32, 5, 32)):
            cs.append(Case(B, N, H, hd, dt))
        # four tiles per workgroup with idle waves in the last one: 2045, 2049, 2051 tiles, single-tile and packed
        for B, N, H, hd in ((409, 17, 5, 32), (683, 17, 3, 64), (293, 17, 7, 32), (2449, 5, 5, 64), (4093, 5, 3, 32),
                            (1753, 5, 7, 64)):
            cs.append(Case(B, N, H, hd, dt))
        # strips
        for N in (33, 63, 64, 65, 96, 97, 127, 128):
            for hd in (32, 64):
                cs.append(Case(3, N, 3, hd, dt))
        # streaming MFMA
        for B, N, H, hd in ((3, 129, 3, 64), (3, 192, 2, 32), (2, 193, 3, 64), (2, 320, 2, 32), (1, 4098, 1, 64)):
            cs.append(Case(B, N, H, hd, dt))
        cs.append(Case(3, 257, 3, 64, dt, "spiked"))
        # 16-bit head dims without an MFMA kernel: the LDS kernel on both sides of the 160 KB switch (fwd / bwd), streaming past it
        for hd, ns in ((8, (52, 53, 131, 132, 184, 185)), (16, (124, 125, 175)), (24, (117, 118, 164, 165)),
                       (80, (21, 22, 81, 82, 112, 113)), (128, (7, 9, 11, 14, 19, 62, 63, 84, 85))):
            for N in ns:
                cs.append(Case(3, N, 3, hd, dt))
        # B H = 10: a last LDS block with idle waves at three waves per block (forward at N 12, backward at N 9, hd 128)
        for N in (9, 12):
            cs.append(Case(5, N, 2, 128, dt))
    # fp32: the LDS kernel at every waves-per-block value (B H not a multiple of it) and both sides of the switch
    for B, N, H, hd in ((3, 7, 3, 64), (5, 16, 2, 64), (3, 20, 3, 64), (5, 20, 2, 64), (3, 30, 3, 64), (3, 40, 3, 64), (3, 90, 3, 64),
                        (3, 91, 3, 64), (3, 124, 3, 64), (3, 125, 3, 64), (3, 111, 3, 32), (3, 112, 3, 32), (3, 155, 3, 32),
                        (3, 156, 3, 32), (5, 25, 2, 32), (3, 45, 3, 32), (3, 62, 3, 128), (3, 63, 3, 128), (3, 84, 3, 128),
                        (3, 85, 3, 128), (3, 9, 3, 128), (3, 12, 3, 128), (16, 65, 12, 64), (32, 17, 16, 32), (8, 65, 1, 512),
                        (3, 257, 3, 64), (2, 129, 3, 32)):
        cs.append(Case(B, N, H, hd, F32))
    cs.append(Case(3, 257, 3, 80, F32, "spiked"))
    # signed bias: one case per 16-bit family and dtype, V and dO positive
    seen = set()
    for c in list(cs):
        key = (c.dtype, ar.family(c.B, c.N, c.H, c.hd, c.dtype, False), ar.family(c.B, c.N, c.H, c.hd, c.dtype, True))
        if c.dtype != F32 and c.kind == "randn" and key not in seen and c.B * c.N * c.H * c.hd >= 4096:
            seen.add(key)
            cs.append(c._replace(kind="pos"))
    return cs


CASES = _cases()
# SKYEMB_MHA_MFMA=0: 16-bit hd 32 / 64 on the LDS and streaming kernels (packed-size, strip and long N)
NOMFMA_CASES = [Case(B, N, H, hd, dt, "randn", False) for dt in (BF, F16)
                for B, N, H, hd in ((7, 5, 3, 64), (5, 17, 3, 32), (3, 65, 3, 64), (3, 97, 2, 32), (2, 257, 2, 64), (2, 160, 2, 32))]


def inputs(c, seed):
    """qkv [B, N, 3 H hd] and dout [B, N, H hd] in fp32, exactly representable in c.dtype."""
    B, N, H, hd = c.B, c.N, c.H, c.hd
    g = torch.Generator().manual_seed(seed)
    if c.kind == "spiked":
        from tests.test_attention_long_gpu import spiked
        qkv, dout = spiked(B, N, H, hd, 11)
    else:
        qkv, dout = torch.randn(B, N, 3 * H * hd, generator=g), torch.randn(B, N, H * hd, generator=g)
    x = qkv.reshape(B, N, 3, H, hd)
    dout = dout.reshape(B, N, H, hd)
    if c.kind == "pos":
        x[:, :, 2] = x[:, :, 2].abs() + 0.25
        dout = dout.abs() + 0.25
    ev, eo = CONTRAST[c.dtype]
    x[:, :, 2] *= ar.scale_pattern(B, H, ev)
    dout = dout * ar.scale_pattern(B, H, eo).flip(0)
    return x.reshape(B, N, -1).to(c.dtype).float(), dout.reshape(B, N, -1).to(c.dtype).float()


def _pad(row):
    return (2 * row + 63) // 64 * 64


def guarded_in(x, dtype, row):
    """x as a view into a NaN-filled buffer with `_pad(row)` NaN elements before and after it."""
    p = _pad(row)
    buf = torch.full((x.numel() + 2 * p,), float("nan"), device=DEV, dtype=dtype)
    v = buf[p:p + x.numel()].view(x.shape)
    v.copy_(x.to(DEV, dtype))
    return v


def guarded_out(shape, dtype, row):
    """(buffer, view): the view NaN, the rest of the buffer the sentinel."""
    n = 1
    for s in shape:
        n *= s
    p = _pad(row)
    buf = torch.full((n + 2 * p,), SENT, device=DEV, dtype=dtype)
    v = buf[p:p + n].view(shape)
    v.fill_(float("nan"))
    return buf, v, p


def guards_intact(buf, p, n):
    return bool((buf[:p] == SENT).all()) and bool((buf[p + n:] == SENT).all())


def run(ops, c, qkv, dout):
    """One forward and two backward launches on guarded buffers: {out, dq, dk, dv} (fp64 CPU), and the checks' verdicts."""
    B, N, H, hd, dt = c.B, c.N, c.H, c.hd, c.dtype
    D = H * hd
    qd, dd = guarded_in(qkv, dt, 3 * D), guarded_in(dout, dt, D)
    ob, out, po = guarded_out((B, N, D), dt, D)
    gb, dqkv, pg = guarded_out((B, N, 3 * D), dt, 3 * D)
    gb2, dqkv2, _ = guarded_out((B, N, 3 * D), dt, 3 * D)
    ops.mha_fwd(qd, out, B, N, H, hd)
    ops.mha_bwd(qd, dd, dqkv, B, N, H, hd)
    ops.mha_bwd(qd, dd, dqkv2, B, N, H, hd)
    torch.cuda.synchronize()
    g = dqkv.reshape(B, N, 3, D)
    res = {"out": out, "dq": g[:, :, 0], "dk": g[:, :, 1], "dv": g[:, :, 2]}
    res = {k: v.double().cpu() for k, v in res.items()}
    ok = {"out_guard": guards_intact(ob, po, out.numel()), "dqkv_guard": guards_intact(gb, pg, dqkv.numel()),
          "repeat": bool(torch.equal(dqkv.view(torch.int16 if dt != F32 else torch.int32),
                                     dqkv2.view(torch.int16 if dt != F32 else torch.int32))),
          "in_intact": bool(torch.equal(qd.cpu().float(), qkv)) and bool(torch.equal(dd.cpu().float(), dout))}
    return res, ok


def check_case(ops, c, worst=None, seed=None):
    """Runs case c and asserts everything the module docstring lists; returns {name: err / bar}."""
    qkv, dout = inputs(c, seed if seed is not None else c.B * 131 + c.N * 17 + c.hd + c.H)
    res, ok = run(ops, c, qkv, dout)
    name = cid(c)
    assert all(ok.values()), (name, ok)
    ref = ar.core(qkv, dout, c.H, c.hd)
    bars = ar.bars(ref, c.dtype)
    ratios = {}
    for n in ar.NAMES:
        err = (res[n] - ref["ref"][n]).abs()
        ratios[n] = ar.worst(err, bars[n])
        if c.kind == "pos" and n in ("out", "dv"):
            bias = float((res[n] - ref["ref"][n]).mean() / bars[n].mean())
            assert abs(bias) < BIAS, (name, n, "signed bias", bias)
    fams = {"out": ar.family(c.B, c.N, c.H, c.hd, c.dtype, False, c.mfma)}
    fb = ar.family(c.B, c.N, c.H, c.hd, c.dtype, True, c.mfma)
    if worst is not None:
        for n, r in ratios.items():
            key = f"{DT[c.dtype]}/{'fwd' if n == 'out' else 'bwd'}/{fams.get(n, fb)}" + ("" if c.mfma else "/nomfma")
            worst[key] = max(worst.get(key, 0.0), r)
    bad = {n: r for n, r in ratios.items() if not r <= 1.0}
    assert not bad, (name, fams["out"], fb, ratios)
    return ratios


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    record_parity("attention_core", {k: round(v, 4) for k, v in sorted(w.items())})


@pytest.mark.parametrize("c", CASES, ids=cid)
def test_attention_core(ops, worst, c):
    check_case(ops, c, worst)


def test_mfma_switched_off():
    """SKYEMB_MHA_MFMA=0 sends 16-bit hd 32 / 64 to the LDS and streaming kernels; the switch is read once
    per process, hence the child process.  Same cases, same bars."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
from tests import test_attention_core_gpu as t
from sky_embeddings_amd import ops
w = {}
for c in t.NOMFMA_CASES:
    t.check_case(ops, c, w)
print("nomfma ok", sorted(w.items()))
'''
    env = dict(os.environ, SKYEMB_MHA_MFMA="0", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "nomfma ok" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
    print(out.stdout.strip().splitlines()[-1])


RANGE_SHAPES = [(7, 5, 3, 64), (5, 17, 3, 32), (3, 65, 3, 64), (2, 257, 2, 32), (3, 40, 3, 80)]


@pytest.mark.parametrize("k", [-8, 12])
@pytest.mark.parametrize("shape", RANGE_SHAPES, ids=lambda s: "B%d_N%d_H%d_hd%d" % s)
def test_bf16_gradients_scale_exactly(ops, shape, k):
    B, N, H, hd = shape
    c = Case(B, N, H, hd, BF)
    qkv, dout = inputs(c, 5)
    g1, _ = run(ops, c, qkv, dout)
    g2, ok = run(ops, c, qkv, dout * 2.0 ** k)
    assert all(ok.values()), ok
    for n in ("dq", "dk", "dv"):
        assert torch.equal(g2[n], g1[n] * 2.0 ** k), (n, k)


def loss_scale(masked_elements):
    from types import SimpleNamespace
    from sky_embeddings_amd.engine import MAEEngine
    return MAEEngine.plan_loss_scale(SimpleNamespace(_loss_scale_auto=True), masked_elements)


def f16_range_inputs(shape, masked):
    """qkv and dout for test_f16_loss_scaled_gradients_near_the_fp16_range, and max |dS| in fp64."""
    B, N, H, hd = shape
    S = loss_scale(masked)
    g = torch.Generator().manual_seed(masked % 1000 + N)
    qkv = torch.randn(B, N, 3, H, hd, generator=g)
    qkv[:, :, 1] = 2.0 * torch.randn(B, 1, H, hd, generator=g) + qkv[:, :, 1]
    qkv[:, :, 2] *= 4.0
    qkv = qkv.reshape(B, N, -1).half().float()
    raw = torch.randn(B, N, H * hd, generator=g) / masked                 # d mean / d element, before the chain factor

    def max_ds(dout):
        q, k, v, do = ar.heads(qkv, dout, H, hd)
        P = torch.softmax(hd ** -0.5 * q @ k.transpose(-2, -1), -1)
        dP = do @ v.transpose(-2, -1)
        return float((P * (dP - (P * dP).sum(-1, keepdim=True))).abs().max())

    chain = 2.0 ** math.floor(math.log2(2.0 ** 15 / max_ds(raw * S)))
    dout = (raw * S * chain).half().float()
    return qkv, dout, max_ds(dout)


@pytest.mark.parametrize("masked", [64 * 2 ** 6, 64 * 2 ** 12, 64 * 2 ** 20])
@pytest.mark.parametrize("shape", RANGE_SHAPES, ids=lambda s: "B%d_N%d_H%d_hd%d" % s)
def test_f16_loss_scaled_gradients_near_the_fp16_range(ops, shape, masked):
    """dout = loss_scale x (the gradient of a mean over `masked` elements, 1 / masked per element, times the power-of-two chain
    factor from the layers above that puts max |dS| in [2^14, 2^15)): dS, rounded to fp16 as an MFMA operand, comes within a
    factor of two to four of 65504.  Keys share a large common offset, so dq = s sum_j dS_ij K_j cancels (sum_j dS_ij = 0) and
    stays well inside fp16 while dS does not.  Every fp64 gradient fits fp16, so the kernel's must be finite and within the
    bar."""
    B, N, H, hd = shape
    assert loss_scale(masked) == min(2.0 ** 16, masked / 64)
    qkv, dout, ds_max = f16_range_inputs(shape, masked)
    assert 2.0 ** 14 <= ds_max < 65504 / 2, ds_max                                  # the regime this test is for
    res, ok = run(ops, Case(B, N, H, hd, F16), qkv, dout)
    assert all(ok.values()), ok
    ref = ar.core(qkv, dout, H, hd)
    bars = ar.bars(ref, F16)
    for n in ar.NAMES:
        assert float(ref["ref"][n].abs().max()) < 65504 / 2, n                       # ... with every gradient inside fp16
        assert bool(torch.isfinite(res[n]).all()), (n, "inf / NaN although the fp64 value fits fp16")
        assert ar.worst((res[n] - ref["ref"][n]).abs(), bars[n]) <= 1.0, n
