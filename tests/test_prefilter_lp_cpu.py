"""CPU: the error bound of the two-stage search's first stage over a RESIDENT fp16 bank (csrc/topk_prefilter.hip, file header).

The library's own host function supplies eps_a; a numpy restatement of stage 1 on exact fp16 rows (tests/
prefilter_lp_reference.py) must stay inside
    |dot^ - chain(tw, x) 2^-f| <= eps_a ||q'|| ||x|| + ||q'|| sqrt(nsub) 2^-14
for every (query, row) pair, with fp16 subnormals kept and with them flushed to zero on either operand, hi only and hi + lo."""
import math

import numpy as np
import pytest

from sky_embeddings_amd import ops
from tests import prefilter_lp_reference as ref


def _bank(D, seed):
    """Seeded rows that stress the row side: ordinary ones, rows of scale 1e-4 (mostly fp16 subnormals), a row of nothing but
    subnormals, rows mixing large, small and subnormal elements, a zero row."""
    rng = np.random.default_rng(seed)
    rows = [rng.standard_normal((12, D)) * rng.uniform(0.2, 5.0, size=(12, 1)),
            rng.standard_normal((8, D)) * 1e-4,
            np.sign(rng.standard_normal((1, D))) * rng.uniform(2.0 ** -24, 2.0 ** -14 * 0.999, size=(1, D)),
            rng.standard_normal((8, D)) * np.where(rng.random((8, D)) < 0.5, 1e-5, 30.0),
            rng.standard_normal((4, D)) * np.where(rng.random((4, D)) < 0.9, 3e-6, 1.0),
            np.zeros((1, D))]
    x16 = np.concatenate(rows).astype(np.float32).astype(np.float16)
    assert ref.count_subnormals(x16)[20] == D and ref.count_subnormals(x16)[12:20].min() > D // 4
    return x16


def _queries(D, seed):
    """Weighted queries tw: ordinary ones, one with tiny components beside large ones (subnormal after the scaling), one small
    overall, one with a single large component."""
    rng = np.random.default_rng(seed + 1000)
    q = rng.standard_normal((6, D))
    q[1] *= np.where(rng.random(D) < 0.7, 1e-9, 1.0)        # scaled maximum ~2^13: components below 2^-14 after the scaling
    q[2] *= 1e-12
    q[3] = 1e-10 * rng.standard_normal(D)
    q[3, D // 3] = 40.0
    w = 1.0 / (rng.random(D) + 0.05) ** 2
    q[4:] *= w / w.sum()
    return q.astype(np.float32)


@pytest.mark.parametrize("D", [128, 768])
@pytest.mark.parametrize("lo", [False, True])
def test_stage1_on_exact_fp16_rows_stays_inside_the_proven_bound(D, lo):
    eps_a = ops.topk_prefilter_eps_a(D, lo=lo, resident=True)
    x16 = _bank(D, D)
    x = x16.astype(np.float64)
    nx = np.sqrt((x * x).sum(axis=1))
    nsub = ref.count_subnormals(x16)
    worst = 0.0
    for tw in _queries(D, D):
        qp, qh, ql, s = ref.scale_query(tw)
        assert 2.0 ** 13 <= np.abs(qp).max() < 2.0 ** 14
        nq = math.sqrt((qp.astype(np.float64) ** 2).sum())
        want = ref.fma_chain(tw, x16.astype(np.float32)).astype(np.float64) * s
        for flush_q in (False, True):
            for flush_x in (False, True):
                got = ref.stage1_dots(qh, ql, x16, lo, flush_q, flush_x)
                bound = eps_a * nq * nx + (nq * np.sqrt(nsub) * 2.0 ** -14 if flush_x else 0.0)
                err = np.abs(got - want)
                assert (err <= bound).all(), (D, lo, flush_q, flush_x, int(np.argmax(err - bound)), float((err - bound).max()))
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    print(f"D={D} lo={lo}: worst |error| / bound = {worst:.3f}")
    assert worst > 0.0                                       # the restatement is not vacuous: something was rounded


def test_the_flush_term_is_needed_and_carried_by_the_row():
    """A row of nothing but fp16 subnormals against a flushing matrix core: dot^ is 0, far outside eps_a ||q'|| ||x|| alone --
    the additive term ||q'|| sqrt(nsub) 2^-14 is what keeps the row's interval valid."""
    D = 128
    rng = np.random.default_rng(5)
    x16 = (np.abs(rng.standard_normal((1, D))) * 3e-6).astype(np.float16)
    tw = np.abs(rng.standard_normal(D)).astype(np.float32)
    qp, qh, ql, s = ref.scale_query(tw)
    nq = math.sqrt((qp.astype(np.float64) ** 2).sum())
    nx = math.sqrt((x16.astype(np.float64) ** 2).sum())
    want = float(ref.fma_chain(tw, x16.astype(np.float32))[0]) * s
    got = float(ref.stage1_dots(qh, ql, x16, False, False, True)[0])
    eps_a = ops.topk_prefilter_eps_a(D, lo=False, resident=True)
    assert got == 0.0 and abs(got - want) > 10 * eps_a * nq * nx
    assert abs(got - want) <= eps_a * nq * nx + nq * math.sqrt(ref.count_subnormals(x16)[0]) * 2.0 ** -14


@pytest.mark.parametrize("D", [128, 160, 768, 1024, 4096])
def test_eps_a_values(D):
    """The fp32-bank bound is the formula it has always been, to the bit; the resident one drops the bank's 2^-11 and the row
    side's half of the subnormal term, nothing else."""
    for lo in (False, True):
        present = (2.0 ** -11 + 2.0 ** -21 if lo else 2.0 ** -10 + 2.0 ** -21) + 6.06 * D * 2.0 ** -24 + 2.0 * math.sqrt(D) * 2.0 ** -27
        assert ops.topk_prefilter_eps_a(D, lo=lo, resident=False) == present
        resident = (2.0 ** -21 if lo else 2.0 ** -11 + 2.0 ** -21) + 6.06 * D * 2.0 ** -24 + math.sqrt(D) * 2.0 ** -27
        assert ops.topk_prefilter_eps_a(D, lo=lo, resident=True) == resident
        assert resident < present
