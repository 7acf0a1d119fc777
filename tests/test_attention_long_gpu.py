"""GPU parity of the long-sequence attention paths (N > 128 tokens, and heads that outgrow the LDS plan) through the C ABI,
full tensors against a float64 statement of softmax(q k^T hd^-0.5) v and its gradient computed from the very operands the
kernel read (the 16-bit operands rounded first):
- bf16 / fp16 at hd 32 / 64: the streaming MFMA kernels of csrc/attention_mfma.hip (online softmax forward; three-phase
  backward without atomics or workspace);
- fp32, and every other head dim: the streaming fp32 kernels of csrc/attention.hip;
- the attention pool past 256 tokens (csrc/attnpool.hip, token loop in chunks).
Bars are those of tests/test_kernels_gpu.py::test_attention: relative L2 error 6e-3 for 16-bit, 3e-6 for fp32; on top of them
every element of out, dq, dk and dv must meet the derived elementwise bar of tests/attention_reference.py, and the operands
sit in the guarded buffers of tests/test_attention_core_gpu.py (NaN around the inputs, a sentinel around the outputs).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_reference as ar
from tests.helpers import record_parity
from tests.test_attention_core_gpu import guarded_in, guarded_out, guards_intact

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
MAX_N = 4098


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()
    return _ops


def tol(dtype):
    return 3e-6 if dtype == torch.float32 else 6e-3


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def reference(qkv, dout, H, hd):
    """fp64 output and dqkv of the attention core, qkv [B, N, 3 H hd] and dout [B, N, H hd] as given (already rounded)."""
    B, N, _ = qkv.shape
    x = qkv.double().requires_grad_(True)
    t = x.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    att = ((t[0] * hd ** -0.5) @ t[1].transpose(-2, -1)).softmax(-1)
    o = (att @ t[2]).transpose(1, 2).reshape(B, N, H * hd)
    o.backward(dout.double())
    return o.detach(), x.grad


def run(ops, qkv, dout, H, hd, dtype, guards=None):
    """Inputs inside NaN, outputs NaN inside a sentinel (guards[...] = whether the sentinel survived)."""
    B, N, _ = qkv.shape
    D = H * hd
    qd, dd = guarded_in(qkv, dtype, 3 * D), guarded_in(dout, dtype, D)
    ob, out, po = guarded_out((B, N, D), dtype, D)
    gb, dqkv, pg = guarded_out((B, N, 3 * D), dtype, 3 * D)
    ops.mha_fwd(qd, out, B, N, H, hd)
    ops.mha_bwd(qd, dd, dqkv, B, N, H, hd)
    torch.cuda.synchronize()
    if guards is not None:
        guards.update(out=guards_intact(ob, po, out.numel()), dqkv=guards_intact(gb, pg, dqkv.numel()))
    return qd, dd, out, dqkv


def check(ops, name, qkv, dout, H, hd, dtype, f32_tol=None):
    guards = {}
    qd, dd, out, dqkv = run(ops, qkv, dout, H, hd, dtype, guards)
    assert all(guards.values()), (name, "write outside out / dqkv", guards)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all()), f"{name}: inf / NaN or unwritten elements"
    o_r, g_r = reference(qd.cpu(), dd.cpu(), H, hd)
    e_o, e_g = relerr(out, o_r), relerr(dqkv, g_r)
    c = ar.core(qd.cpu().float(), dd.cpu().float(), H, hd)
    bars = ar.bars(c, dtype)
    B, N, D = out.shape
    g = dqkv.double().cpu().reshape(B, N, 3, D)
    got = {"out": out.double().cpu(), "dq": g[:, :, 0], "dk": g[:, :, 1], "dv": g[:, :, 2]}
    ratios = {n: ar.worst((got[n] - c["ref"][n]).abs(), bars[n]) for n in ar.NAMES}
    record_parity(f"attention_long[{name}]", {"out": e_o, "dqkv": e_g, "err/bar": max(ratios.values())})
    bar = f32_tol if (f32_tol is not None and dtype == torch.float32) else tol(dtype)
    assert e_o < bar, (name, "out", e_o)
    assert e_g < bar, (name, "dqkv", e_g)
    assert all(r <= 1.0 for r in ratios.values()), (name, "elementwise bar", ratios)


def inputs(B, N, H, hd, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, 3 * H * hd, generator=g), torch.randn(B, N, H * hd, generator=g)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT.get)
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("N", [129, 130, 160, 257, 258, 513, 1025])
def test_long_attention(ops, N, hd, dtype):
    """Key blocks of 64 with a partial tail (129, 130, 257, 258: one to two tokens past a block), whole blocks (160 = 2.5
    blocks, 513, 1025), odd B and H."""
    B, H = 3, 3
    qkv, dout = inputs(B, N, H, hd, N * 7 + hd)
    check(ops, f"{DT[dtype]}-N{N}-hd{hd}", qkv, dout, H, hd, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=DT.get)
def test_longest_sequence(ops, dtype):
    """N = SKYEMB_MHA_MAX_N: 4096 patches + cls + RA/Dec; the backward keeps 2 x 4098 statistics in LDS."""
    qkv, dout = inputs(1, MAX_N, 1, 64, 5)
    check(ops, f"{DT[dtype]}-N{MAX_N}-hd64", qkv, dout, 1, 64, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=DT.get)
@pytest.mark.parametrize("N", [65, 257])
@pytest.mark.parametrize("hd", [8, 80, 128, 512])
def test_fallback_head_dims(ops, hd, N, dtype):
    """Head dims without an MFMA kernel; hd 512 at N = 65 is maesimple's single decoder head.  hd 8 and 80 at N = 65 still
    fit the whole-head LDS kernel (controls); the others stream."""
    B, H = 3, (1 if hd == 512 else 3)
    qkv, dout = inputs(B, N, H, hd, N + hd)
    check(ops, f"{DT[dtype]}-N{N}-hd{hd}", qkv, dout, H, hd, dtype)


def spiked(B, N, H, hd, seed):
    """Scores that force the online rescale: key N - 1 (alone in the last 64-key block at N = 257: blocks 0-63, ..., 192-255,
    256) is a large multiple of a unit vector u and key 3 (first block) of -u, so queries along +u meet their max in the last
    block and queries along -u in the first; their logits reach ~60.  Query 10 is zero: a row of identical scores (uniform
    attention)."""
    qkv, dout = inputs(B, N, H, hd, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = qkv.reshape(B, N, 3, H, hd)
    u = torch.randn(hd, generator=g)
    u = u / u.norm()
    x[:, N - 1, 1] = 8.0 * u
    x[:, 3, 1] = -8.0 * u
    sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
    x[:, :, 0] += 7.5 * hd ** 0.5 * sign[None, :, None, None] * u     # q . k_{N-1} hd^-0.5 ~ +-60
    x[:, 10, 0] = 0.0
    return x.reshape(B, N, -1), dout


@pytest.mark.parametrize("case", [(torch.bfloat16, 64), (torch.float16, 64), (torch.float32, 64), (torch.bfloat16, 32),
                                  (torch.float32, 80)], ids=lambda c: f"{DT[c[0]]}-hd{c[1]}")
def test_online_rescale_and_large_logits(ops, case):
    dtype, hd = case
    B, N, H = 3, 257, 3
    qkv, dout = spiked(B, N, H, hd, 11)
    # fp32: scores of magnitude 60 carry a rounding of 60 x 2^-24 = 3.6e-6, which P and dS inherit as relative error: 2e-5
    # (measured 5.9e-6 on the gradient at hd 80)
    check(ops, f"spiked-{DT[dtype]}-hd{hd}", qkv, dout, H, hd, dtype, f32_tol=2e-5)
    # the uniform row: its output is the plain mean of v
    qd, _, out, _ = run(ops, qkv, dout, H, hd, dtype)
    v = qd.cpu().double().reshape(B, N, 3, H, hd)[:, :, 2].mean(1).reshape(B, H * hd)
    assert relerr(out[:, 10], v) < tol(dtype)


@pytest.mark.parametrize("case", [(torch.bfloat16, 64, 257), (torch.float16, 32, 513), (torch.float32, 64, 257),
                                  (torch.bfloat16, 80, 257)], ids=lambda c: f"{DT[c[0]]}-hd{c[1]}-N{c[2]}")
def test_backward_is_deterministic(ops, case):
    dtype, hd, N = case
    B, H = 5, 3
    qkv, dout = inputs(B, N, H, hd, 3)
    _, _, o1, g1 = run(ops, qkv, dout, H, hd, dtype)
    _, _, o2, g2 = run(ops, qkv, dout, H, hd, dtype)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=DT.get)
def test_graph_replay_matches_eager(ops, dtype):
    B, N, H, hd = 3, 257, 3, 64
    D = H * hd
    qkv, dout = inputs(B, N, H, hd, 21)
    qd, dd, o_e, g_e = run(ops, qkv, dout, H, hd, dtype)
    out = torch.zeros(B, N, D, device=DEV, dtype=dtype)
    dqkv = torch.zeros(B, N, 3 * D, device=DEV, dtype=dtype)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                      # warm-up on the capture stream
        ops.mha_fwd(qd, out, B, N, H, hd)
        ops.mha_bwd(qd, dd, dqkv, B, N, H, hd)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.mha_fwd(qd, out, B, N, H, hd)
        ops.mha_bwd(qd, dd, dqkv, B, N, H, hd)
    out.zero_()
    dqkv.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, o_e) and torch.equal(dqkv, g_e)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT.get)
def test_too_long_is_an_error_and_launches_nothing(ops, dtype):
    from sky_embeddings_amd._lib import SkyembError
    B, N, H, hd = 1, MAX_N + 1, 1, 64
    qd = torch.zeros(B, N, 3 * H * hd, device=DEV, dtype=dtype)
    out = torch.full((B, N, H * hd), 7.0, device=DEV, dtype=dtype)
    with pytest.raises(SkyembError, match="4099 tokens"):
        ops.mha_fwd(qd, out, B, N, H, hd)
    with pytest.raises(SkyembError, match="4099 tokens"):
        ops.mha_bwd(qd, out, qd, B, N, H, hd)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((qd == 0).all())


# ------------------------------------------------------------------------------------ attention pool
@pytest.mark.parametrize("dtype", DTYPES, ids=DT.get)
@pytest.mark.parametrize("shape", [(3, 66, 12, 64), (3, 257, 3, 64), (3, 257, 2, 512), (2, 1025, 3, 36), (1, MAX_N, 1, 64)],
                         ids=lambda s: "B%d_N%d_H%d_hd%d" % s)
def test_attnpool_long(ops, shape, dtype):
    """Past the 256 tokens the pool keeps in LDS: the token loop in chunks of 256 (skyemb_attnpool_fwd_long / _bwd_long, what
    the engines call), bars of tests/test_head_kernels_gpu.py."""
    from types import SimpleNamespace
    from tests.test_head_kernels_gpu import run_attnpool
    long_ops = SimpleNamespace(attnpool_q=ops.attnpool_q, attnpool_fwd=ops.attnpool_fwd_long, attnpool_bwd=ops.attnpool_bwd_long,
                               attnpool_q_bwd=ops.attnpool_q_bwd)
    B, N, H, hd = shape
    D = H * hd
    g = torch.Generator().manual_seed(B * 1000 + N * 10 + hd)
    latent = torch.randn(D, generator=g)
    Wq = torch.randn(D, D, generator=g) / D ** 0.5
    bq = 0.1 * torch.randn(D, generator=g)
    kv = torch.randn(B, N, 2, H, hd, generator=g)
    dout = torch.randn(B, D, generator=g)
    errs = run_attnpool(long_ops, B, N, H, hd, dtype, kv, dout, latent=latent, Wq=Wq, bq=bq)
    record_parity(f"attnpool_long[{DT[dtype]}-B{B}_N{N}_H{H}_hd{hd}]", errs)
