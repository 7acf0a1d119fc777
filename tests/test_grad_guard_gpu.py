"""GPU: the overflow guard of a dynamically scaled optimiser step, kernel by kernel -- ``skyemb_grad_probe`` (flag for +-inf / NaN
and the largest finite |g|, accumulated over launches) against torch on the same tensor, and ``skyemb_adamw_guarded`` (flag 0: the
bytes of ``skyemb_adamw``; flag 1: nothing written) for every dtype combination the AdamW entry point dispatches."""
import functools
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
SWEEP = 4 * 256 * (256 * 16)        # elements one pass of the capped grid covers with one four-element group per lane
# 4: one group; 1024: one full block; 2048 + 4: a tail behind one full sweep of a block; SWEEP + 8 + 4: past one pass of the capped
# grid (the second group a lane keeps in flight); 2 * SWEEP + 8 + 4: past both groups, so the grid-stride loop itself runs again
SIZES = [4, 1024, 2048 + 4, SWEEP + 8 + 4, 2 * SWEEP + 8 + 4]
PLANTS = [float("inf"), float("-inf"), float("nan")]
_INT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def bits(t):
    return t.view(_INT.get(t.dtype, t.dtype))


def f32_bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


@functools.lru_cache(maxsize=None)
def base_gradients(dtype, n):
    """Finite gradients over ten decades, shared (never written) by the cases of one (dtype, n)."""
    gen = torch.Generator(device="cuda").manual_seed(1000 + n % 977)
    g = torch.randn(n, device="cuda", generator=gen) * torch.exp(torch.randn(n, device="cuda", generator=gen) * 4.0)
    return g.clamp_(-6e4, 6e4).to(dtype)


def reference(g):
    """(any non-finite, fp32 bits of the largest finite |g|) by torch, in fp64 / fp32."""
    fin = torch.isfinite(g)
    absmax = torch.where(fin, g.double().abs(), torch.zeros((), device=g.device, dtype=torch.float64)).max().float()
    return (not bool(fin.all())), int(absmax.view(torch.int32))


def run_probe(g, state=None):
    from sky_embeddings_amd import ops
    if state is None:
        state = torch.zeros(2, device="cuda", dtype=torch.int32)
    ops.grad_probe(g, g.numel(), state)
    return state


def interior_index(n):
    """An element a lane reaches in its second group (n > SWEEP) or its second trip of the loop (n > 2 * SWEEP); mid-range below."""
    return 2 * SWEEP + 5 if n > 2 * SWEEP else SWEEP + 5 if n > SWEEP else n // 2


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_probe_flag_and_absmax(dtype, n):
    base = base_gradients(dtype, n)
    want_flag, want_bits = reference(base)
    assert not want_flag
    got = run_probe(base).tolist()
    assert got[0] == 0 and got[1] == want_bits, ("no plant", got, want_bits)
    for plant in PLANTS:
        for at in (0, n - 1, interior_index(n)):
            g = base.clone()
            g[at] = plant
            want_flag, want_bits = reference(g)
            assert want_flag
            got = run_probe(g).tolist()
            assert got[0] != 0 and got[1] == want_bits, (plant, at, got, want_bits)


@pytest.mark.parametrize("dtype", DTYPES)
def test_probe_absmax_is_the_largest_element_wherever_it_sits(dtype):
    n = 2048 + 4
    for at in (0, 3, 1023, 1024, 2047, 2048, n - 1):
        g = base_gradients(dtype, n).clone()
        g[at] = -61440.0                                     # 15 * 2^12: exact in all three formats, above every other element
        assert run_probe(g).tolist() == [0, f32_bits(61440.0)], at


@pytest.mark.parametrize("dtype", DTYPES)
def test_probe_zeros_subnormals_and_the_largest_finite_value_are_finite(dtype):
    fi = torch.finfo(dtype)
    idt = _INT[dtype]
    sign = -2 ** 15 if idt == torch.int16 else -2 ** 31
    mant = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}[dtype]
    # bit patterns: +0, -0, smallest and largest subnormal of either sign
    sub = torch.tensor([0, sign, 1, sign + 1, 2 ** mant - 1, sign + 2 ** mant - 1, 0, 0], dtype=idt).view(dtype)
    assert bool((sub.double().abs() < fi.tiny).all())
    want, least = float(sub[4].double()), float(sub[2].double())   # (2^mant - 1) and 1 times 2^(emin - mant): exact in fp32
    assert 0.0 < least < want
    sub = sub.cuda()
    assert run_probe(sub).tolist() == [0, f32_bits(want)]
    assert run_probe(sub[:4].clone()).tolist() == [0, f32_bits(least)]
    assert run_probe(torch.zeros(8, device="cuda", dtype=dtype).neg_()).tolist() == [0, 0]
    big = torch.tensor([0.0, fi.tiny, -fi.max, 1.0, fi.max, -1.0, 0.0, 0.0], dtype=torch.float64).to(dtype).cuda()
    assert run_probe(big).tolist() == [0, f32_bits(fi.max)]
    # one step further is not finite: the flag rises, and the maximum keeps to the finite elements
    beyond = big.clone()
    beyond[2] = float("-inf")
    beyond[4] = float("nan")
    assert run_probe(beyond).tolist() == [1, f32_bits(1.0)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_probe_accumulates_over_launches(dtype):
    n = 2048 + 4
    lo, hi = base_gradients(dtype, n).clone().clamp_(-1.0, 1.0), base_gradients(dtype, n).clone()
    hi[7] = 5e4
    _, lo_bits = reference(lo)
    _, hi_bits = reference(hi)
    assert lo_bits < hi_bits
    for first, second in ((lo, hi), (hi, lo)):
        state = run_probe(first)
        assert run_probe(second, state).tolist() == [0, hi_bits]
    bad = lo.clone()
    bad[n - 2] = float("nan")
    for first, second in ((bad, hi), (hi, bad)):                 # the flag survives a clean range probed after it
        state = run_probe(first)
        got = run_probe(second, state).tolist()
        assert got[0] != 0 and got[1] == hi_bits
    # ranges of different formats share one state (the head's and the engine's buffers of one step)
    state = run_probe(lo)
    other = torch.full((4,), 3.0, device="cuda", dtype=torch.float32 if dtype != torch.float32 else torch.float16)
    assert run_probe(other, state).tolist() == [0, max(lo_bits, f32_bits(3.0))]


def test_probe_rejects_what_the_kernel_cannot_read():
    from sky_embeddings_amd import _lib, ops
    state = torch.zeros(2, device="cuda", dtype=torch.int32)
    g = torch.zeros(16, device="cuda")
    with pytest.raises(_lib.SkyembError):
        ops.grad_probe(g, 6, state)
    with pytest.raises(_lib.SkyembError):
        ops.grad_probe(g[1:], 4, state)
    with pytest.raises(_lib.SkyembError):
        ops.grad_probe(g, 0, state)


# (shadow dtype or None, gradient dtype): the instantiations skyemb_adamw dispatches
ADAMW_COMBOS = [(None, torch.float32), (None, torch.bfloat16), (None, torch.float16),
                (torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16),
                (torch.float16, torch.float32), (torch.float16, torch.float16),
                (torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.float32, torch.float16)]


def adamw_inputs(n, lp, gdt):
    gen = torch.Generator(device="cuda").manual_seed(7 + n)
    p = torch.randn(n, device="cuda", generator=gen)
    g = (torch.randn(n, device="cuda", generator=gen) * 64.0).to(gdt)
    m = torch.randn(n, device="cuda", generator=gen) * 0.1
    v = torch.rand(n, device="cuda", generator=gen) * 0.01
    p_lp = None if lp is None else torch.full((n,), 0.5, device="cuda").to(lp)
    return [p, g, m, v, p_lp]


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("n,n_decay", [(4, 2), (2048 + 4, 1001)])
@pytest.mark.parametrize("lp,gdt", ADAMW_COMBOS)
def test_guarded_adamw_is_adamw_or_nothing(lp, gdt, n, n_decay, zero_grad):
    from sky_embeddings_amd import ops
    hyp = dict(grad_scale=1.0 / 64.0, zero_grad=bool(zero_grad), lr=3e-3, bc1=1.0 - 0.9 ** 3, bc2=1.0 - 0.999 ** 3)
    start = adamw_inputs(n, lp, gdt)
    plain = [None if t is None else t.clone() for t in start]
    ops.adamw(*plain, n, n_decay, None, 0.9, 0.999, 1e-8, 0.05, **hyp)
    assert not torch.equal(plain[0], start[0])
    names = ("p", "g", "m", "v", "p_lp")
    for flag in (0, 1):
        skip = torch.tensor([flag, 0x7f000000], device="cuda", dtype=torch.int32)      # (only word 0 decides)
        bufs = [None if t is None else t.clone() for t in start]
        ops.adamw_guarded(*bufs, n, n_decay, None, 0.9, 0.999, 1e-8, 0.05, skip, **hyp)
        want = start if flag else plain
        for name, got, ref in zip(names, bufs, want):
            if ref is not None:
                assert torch.equal(bits(got), bits(ref)), (flag, name)
        assert skip.tolist() == [flag, 0x7f000000]
    if zero_grad:
        assert not bool(plain[1].any())
