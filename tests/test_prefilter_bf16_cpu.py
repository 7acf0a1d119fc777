"""CPU: the error bound of the two-stage search's first stage over a RESIDENT bf16 bank (csrc/topk_prefilter.hip, file header,
"Resident bf16 bank"), and what that search refuses before any launch.

The library's own host function supplies eps_a; a numpy restatement of stage 1 on exact bf16 rows (tests/
prefilter_bf16_reference.py) must stay inside
    |dot^ - chain(tw, x) 2^-f| <= eps_a ||q'|| ||x||
for every (query, row) pair whose row is inside the window the row constants ask for -- every other row is unboundable (its
bound is infinite: a candidate of every query) -- with tiny numbers kept and with them flushed to zero: bf16-subnormal operands
on either side, and every product below 2^-126.  Hi only and hi + lo."""
import ctypes
import math

import numpy as np
import pytest
import torch

from sky_embeddings_amd import _lib, ops
from tests import prefilter_bf16_reference as ref
from tests.prefilter_lp_reference import fma_chain
from tests.test_prefilter_lp_cpu import _queries

# rows of the bank below, by what they are
ORDINARY, TINY30, HUGE30, MIXED, IN_LO, IN_LO_ONE, OUT_LO, IN_HI, OUT_HI, ZERO = (slice(0, 12), slice(12, 16), slice(16, 20), 20, 21, 22, 23,
                                                                                 24, 25, 26)


def _bank(D, seed):
    """Seeded bf16 rows (as fp32): ordinary ones of mixed scale, rows at 1e-30 and at 1e+30, a row mixing 1e-35 and 1e+3 elements,
    rows just inside the unboundable window (every element in [2^-60, 2^-59); ONE element of 2^-60 beside zeros; elements up to the
    largest bf16 below 2^120) and just outside it (an element of 2^-61; an element of 2^120), a zero row."""
    rng = np.random.default_rng(seed)
    sign = lambda n: np.sign(rng.standard_normal((n, D)))
    one = np.zeros((1, D))
    one[0, D // 5] = 2.0 ** -60
    out_lo = rng.standard_normal((1, D))
    out_lo[0, 3] = 2.0 ** -61
    in_hi = rng.standard_normal((1, D)) * 2.0 ** 100
    in_hi[0, 5] = -(2.0 ** 119) * (2.0 - 2.0 ** -7)
    out_hi = rng.standard_normal((1, D))
    out_hi[0, 9] = 2.0 ** 120
    rows = [rng.standard_normal((12, D)) * rng.uniform(0.2, 5.0, size=(12, 1)),
            rng.standard_normal((4, D)) * 1e-30,
            rng.standard_normal((4, D)) * 1e+30,
            rng.standard_normal((1, D)) * np.where(rng.random((1, D)) < 0.5, 1e-35, 1e+3),
            sign(1) * rng.uniform(2.0 ** -60, 2.0 ** -59 * 0.99, size=(1, D)),
            one, out_lo, in_hi, out_hi,
            np.zeros((1, D))]
    x = ref.bf16(np.concatenate(rows).astype(np.float32))
    ub = ref.unboundable(x)
    assert not ub[ORDINARY].any() and ub[TINY30].all() and not ub[HUGE30].any() and ub[MIXED]
    assert not ub[IN_LO] and not ub[IN_LO_ONE] and ub[OUT_LO] and not ub[IN_HI] and ub[OUT_HI] and not ub[ZERO]
    assert np.abs(x[IN_LO]).min() >= 2.0 ** -60 and np.abs(x[IN_HI]).max() == 2.0 ** 119 * (2.0 - 2.0 ** -7)
    return x


@pytest.mark.parametrize("D", [128, 768])
@pytest.mark.parametrize("lo", [False, True])
def test_stage1_on_exact_bf16_rows_stays_inside_the_proven_bound(D, lo):
    eps_a = ops.topk_prefilter_eps_a_resident(D, torch.bfloat16, lo=lo)
    x = _bank(D, D)
    x64 = x.astype(np.float64)
    nx = np.sqrt((x64 * x64).sum(axis=1))
    ub = ref.unboundable(x)
    worst = 0.0
    for tw in _queries(D, D):
        qp, qh, ql, s = ref.scale_query(tw)
        assert 2.0 ** -21 <= np.abs(qp).max() < 2.0 ** -20 and ref.query_in_window(s)
        nq = math.sqrt((qp.astype(np.float64) ** 2).sum())
        want = fma_chain(tw, x).astype(np.float64) * s
        bound = np.where(ub, np.inf, eps_a * nq * nx)
        for flush_q in (False, True):
            for flush_x in (False, True):
                for flush_p in (False, True):
                    got = ref.stage1_dots(qh, ql, x, lo, flush_q, flush_x, flush_p)
                    err = np.abs(got - want)
                    assert (err <= bound).all(), (D, lo, flush_q, flush_x, flush_p, int(np.argmax(err - bound)), float((err - bound).max()))
                    with np.errstate(divide="ignore", invalid="ignore"):
                        worst = max(worst, float(np.nanmax(np.where((bound > 0) & ~ub, err / bound, 0.0))))
    print(f"D={D} lo={lo}: worst |error| / bound = {worst:.3f}")
    assert worst > 0.0                                       # the restatement is not vacuous: something was rounded


def test_the_bound_carries_no_additive_term_because_rows_below_the_window_are_unboundable():
    """The bf16 bound has no counterpart of the fp16 bound's additive subnormal term: what would need one is kept out by the window.
    A row of elements around 2^-110 against a core that flushes products below 2^-126: dot^ is 0, far outside eps_a ||q'|| ||x||
    -- and the row is one the row constants call unboundable.  The same row scaled into the window is inside the plain bound."""
    D = 128
    rng = np.random.default_rng(5)
    base = np.abs(rng.standard_normal((1, D))).astype(np.float32) + 0.5
    tw = np.abs(rng.standard_normal(D)).astype(np.float32)
    qp, qh, ql, s = ref.scale_query(tw)
    nq = math.sqrt((qp.astype(np.float64) ** 2).sum())
    eps_a = ops.topk_prefilter_eps_a_resident(D, torch.bfloat16, lo=False)
    for scale, inside in ((2.0 ** -110, False), (2.0 ** -59, True)):
        x = ref.bf16(base * np.float32(scale))
        nx = math.sqrt((x.astype(np.float64) ** 2).sum())
        want = float(fma_chain(tw, x)[0]) * s
        got = float(ref.stage1_dots(qh, ql, x, False, False, False, True)[0])
        if inside:
            assert not ref.unboundable(x)[0] and abs(got - want) <= eps_a * nq * nx
        else:
            assert got == 0.0 and abs(got - want) > 10 * eps_a * nq * nx and ref.unboundable(x)[0]


@pytest.mark.parametrize("D", [128, 160, 768, 1024, 4096])
def test_eps_a_values(D):
    """The bf16 bound against its written formula; the fp32-bank and resident-fp16 bounds are what they were, to the bit, through
    the old entry point and through the new one."""
    for lo in (False, True):
        bf = (2.0 ** -18 if lo else 2.0 ** -9) + 6.06 * D * 2.0 ** -24 + D * 2.0 ** -38
        assert ops.topk_prefilter_eps_a_resident(D, torch.bfloat16, lo=lo) == bf
        present = (2.0 ** -11 + 2.0 ** -21 if lo else 2.0 ** -10 + 2.0 ** -21) + 6.06 * D * 2.0 ** -24 + 2.0 * math.sqrt(D) * 2.0 ** -27
        assert ops.topk_prefilter_eps_a(D, lo=lo, resident=False) == present
        resident = (2.0 ** -21 if lo else 2.0 ** -11 + 2.0 ** -21) + 6.06 * D * 2.0 ** -24 + math.sqrt(D) * 2.0 ** -27
        assert ops.topk_prefilter_eps_a(D, lo=lo, resident=True) == resident
        assert ops.topk_prefilter_eps_a_resident(D, torch.float16, lo=lo) == resident
    hi, hilo = (ops.topk_prefilter_eps_a_resident(D, torch.bfloat16, lo=l) for l in (False, True))
    # hi + lo is tighter than the resident fp16 bank's hi only; hi only is the widest of all
    assert hilo < ops.topk_prefilter_eps_a(D, lo=False, resident=True) < hi
    with pytest.raises(ValueError, match="torch.float16 or torch.bfloat16"):
        ops.topk_prefilter_eps_a_resident(D, torch.float32)


def test_eps_a_at_768_is_what_the_design_quotes():
    assert abs(ops.topk_prefilter_eps_a_resident(768, torch.bfloat16, lo=False) - 2.23e-3) < 1e-5
    assert abs(ops.topk_prefilter_eps_a_resident(768, torch.bfloat16, lo=True) - 2.81e-4) < 1e-6


def test_resident_refuses_everything_but_a_16_bit_tensor_and_the_plain_constructor_names_it():
    from sky_embeddings_amd import search
    for bad in (torch.zeros(4, 32), torch.zeros(4, 32, dtype=torch.float64), torch.zeros(4, 32, dtype=torch.int16), [[0.0]]):
        with pytest.raises(ValueError, match="torch.float16 or torch.bfloat16"):
            search.PreparedBank.resident(bad)
    with pytest.raises(ValueError, match="bfloat16") as e:
        search.PreparedBank(torch.zeros(4, 32, dtype=torch.bfloat16))
    assert "PreparedBank.resident" in str(e.value)


def _odd(N, D, dtype):
    odd = torch.empty(N * D + 8, dtype=dtype)[4:4 + N * D].view(N, D)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 8
    return odd


def test_a_misaligned_bank_is_refused_before_any_launch():
    from sky_embeddings_amd import search
    N, D = 256, 64
    for dtype in (torch.bfloat16, torch.float16):
        odd = _odd(N, D, dtype)
        with pytest.raises(ValueError, match="16-byte aligned"):
            search.PreparedBank.resident(odd)
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.resident_rowp(odd, None)
    # the C entry points themselves (argument checks come before any device work: host pointers are never touched)
    L = _lib.lib()
    odd = _odd(N, D, torch.bfloat16)
    f = torch.zeros(4 * N)
    for dt in (_lib.BF16, _lib.F16):
        assert L.skyemb_resident_rowp(odd.data_ptr(), dt, f.data_ptr(), N, D, f.data_ptr(), None, None) != 0
        assert b"16-byte aligned" in L.skyemb_last_error()
        assert L.skyemb_cosine_topk_prefiltered_resident(f.data_ptr(), f.data_ptr(), 64, odd.data_ptr(), dt, f.data_ptr(), None, f.data_ptr(),
                                                         2048, 128, 10, 1e-6, 0, None, f.data_ptr(), 1 << 40, f.data_ptr(), f.data_ptr(),
                                                         f.data_ptr(), None) != 0
        assert b"16-byte aligned" in L.skyemb_last_error()
        assert L.skyemb_cosine_topk_prefiltered_resident_sel(f.data_ptr(), f.data_ptr(), 64, odd.data_ptr(), dt, f.data_ptr(), None,
                                                             f.data_ptr(), f.data_ptr(), 8, 0, 2048, 128, 10, 1e-6, 0, f.data_ptr(), 1 << 40,
                                                             f.data_ptr(), f.data_ptr(), f.data_ptr(), None) != 0
        assert b"16-byte aligned" in L.skyemb_last_error()
    # a whole number of tiles needs no tail tile; anything else does
    ok = torch.zeros(8, dtype=torch.bfloat16)
    assert L.skyemb_resident_rowp(ok.data_ptr(), _lib.BF16, f.data_ptr(), 300, D, f.data_ptr(), None, None) != 0
    assert b"tail tile" in L.skyemb_last_error()
    # the format code is SKYEMB_BF16 or SKYEMB_F16
    assert L.skyemb_resident_rowp(ok.data_ptr(), _lib.F32, f.data_ptr(), N, D, f.data_ptr(), None, None) != 0
    assert b"SKYEMB_BF16 (0) or SKYEMB_F16 (2)" in L.skyemb_last_error()


@pytest.mark.parametrize("lo,Q,tile", [("1", 2100, 128), ("0", 4096, 256)])
def test_the_work_item_refusal_uses_the_query_tile_of_the_variant(lo, Q, tile, monkeypatch):
    """ceil(N / 2048) * ceil(Q / tile) * (D / 32) >= 2^31 is refused before any launch, with the variant's own query tile: 128 under
    hi + lo, 256 under hi only."""
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", lo)
    L = _lib.lib()
    f = torch.zeros(64)
    N, D = (1 << 31) - 1, 4096
    assert -(-N // 2048) * -(-Q // tile) * (D // 32) >= 1 << 31
    rc = L.skyemb_cosine_topk_prefiltered_resident(f.data_ptr(), f.data_ptr(), Q, f.data_ptr(), _lib.BF16, f.data_ptr(), f.data_ptr(),
                                                   f.data_ptr(), N, D, 10, 1e-6, 0, None, f.data_ptr(), 1 << 40, f.data_ptr(), f.data_ptr(),
                                                   f.data_ptr(), None)
    assert rc != 0 and f"ceil(Q / {tile})".encode() in L.skyemb_last_error()
