"""CPU: the two-stage weighted-MSE token search under combine 'mean' -- the route decision and every refusal text of its rule, the
answers without the opt-in (today's strings), eps and gamma against the library, the new symbols, the checkers of
tests/token_mse_mean_reference.py against planted defects, the soundness of the bound against the contract's mean, and, for every
case of tests/test_token_mse_mean_gpu.py, the conditions on its inputs (no flagged query, no candidate list that could overflow)."""
import os
import re

import numpy as np
import pytest
import torch

from sky_embeddings_amd import _lib, ops, search
from tests import token_mse_mean_reference as mr
from tests import token_mse_prefilter_reference as mpr

MIN, MEAN, MAX = (ops.COMBINE_CODES[c] for c in ("min", "mean", "max"))
NEW = ("skyemb_token_mse_mean_prefilter_applicable", "skyemb_token_mse_mean_prefilter_eps", "skyemb_token_mse_mean_prefilter_gamma",
       "skyemb_token_mse_mean_pool", "skyemb_token_mse_mean_rowp", "skyemb_distance_topk_tokens_mean_prefiltered")
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bank(prepared=True):
    tb = search.TokenBank.__new__(search.TokenBank)               # no device: the decision reads the flags only
    tb._resident, tb.dtype, tb._mse_mean = True, torch.float16, (None, None, None) if prepared else None
    return tb


def _request(**kw):
    base = dict(who="distance_topk_tokens", Q=2048, N=4096, P=16, D=128, k=10, combine=MEAN, metric=ops.METRIC_CODES["MSE"],
                metric_name="MSE", top_t=0, per_query=False, step=16, idx_offset=0, tokens=None, bank=_bank(), weights=None, select=None)
    base.update(kw)
    return search.TokenRequest(**base)


def test_new_symbols_are_declared_and_resolved():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "skyemb.h")).read()
    for name in NEW:
        assert getattr(L, name) is not None and getattr(L, name).argtypes is not None, name
        assert re.search(r"\b%s\(" % name, header), name


def test_route_decision_and_refusal_texts(monkeypatch):
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    refusal = search._token_prefilter_refusal
    pinned = "combine 'mean' under a distance metric"
    assert search.TOKEN_MSE_MEAN_PREFILTER_MIN_Q in (16, 32, 64, 128, 256, 512, 1024)     # a point of the tool's grid
    # not prepared: the pinned words; a bank built without the attribute too
    assert refusal(_request(bank=_bank(False))) == pinned
    bare = search.TokenBank.__new__(search.TokenBank)
    bare._resident, bare.dtype = True, torch.float16
    assert refusal(_request(bank=bare)) == pinned
    # prepared
    assert refusal(_request()) is None
    for P in (1, 2, 4, 8, 16, 32, 64):
        assert refusal(_request(P=P)) is None
    # prepared plus top_t, select or per-query weights: the pinned words stay
    assert refusal(_request(top_t=2)) == pinned
    assert refusal(_request(select=object())) == pinned
    assert refusal(_request(per_query=True)) == pinned
    # min / max over a bank prepared for mean only: the plain route's rule, as ever
    assert refusal(_request(combine=MIN)) is None and refusal(_request(combine=MAX)) is None
    assert "MAE" in refusal(_request(metric=ops.METRIC_CODES["MAE"], metric_name="MAE"))
    assert refusal(_request(P=48)) == "P = 48 does not divide 64"
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    assert refusal(_request()) == "SKYEMB_TOPK_PREFILTER=0"
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER")
    # the library's own text: N counts IMAGES here (2047 images of 16 tokens are 32752 rows, enough for min / max, not for mean)
    for kw in (dict(N=2047), dict(D=144), dict(D=96), dict(D=4128), dict(k=257), dict(k=4097, N=4096)):
        rq = _request(**kw)
        why = refusal(rq)
        assert why == ops.token_mse_mean_prefilter_refusal(rq.Q, rq.N, rq.P, rq.D, rq.k), kw
        assert why.startswith("many-query weighted-MSE patch-token search, combine mean: needs"), why
    assert "N >= 2048 images" in refusal(_request(N=2047)) and refusal(_request(N=2048)) is None
    assert refusal(_request(N=2047, combine=MIN)) is None
    # Q below the constant: on a bank of the measured size its own name, on a smaller one the shared small-bank constant
    big, small = dict(N=15625, P=64, D=768), search.TOKEN_MSE_PREFILTER_MIN_Q_SMALL
    monkeypatch.setattr(search, "TOKEN_MSE_MEAN_PREFILTER_MIN_Q", 128)
    assert refusal(_request(Q=127, **big)) == "Q = 127 < TOKEN_MSE_MEAN_PREFILTER_MIN_Q = 128"
    assert refusal(_request(Q=128, **big)) is None
    assert refusal(_request(Q=small - 1)).startswith(f"Q = {small - 1} < TOKEN_MSE_PREFILTER_MIN_Q_SMALL = {small}")
    assert refusal(_request(Q=small)) is None
    # a request that misses both: the shape rule speaks first, as the rule lists them
    assert refusal(_request(Q=16, N=2047)).startswith("many-query weighted-MSE patch-token search, combine mean: needs")
    # the same decision from plain facts
    plain = search.token_mse_route_refusal
    assert plain(small, 4096, 16, 128, 10, "MSE", "mean", mean_prepared=True) is None
    assert plain(small, 4096, 16, 128, 10, "MSE", "mean") == pinned
    assert plain(small, 4096, 16, 128, 10, "MSE", "mean", 2, mean_prepared=True, top_t_prepared=True) == pinned
    assert plain(small, 4096, 16, 128, 10, "MSE", "mean", None, True, mean_prepared=True, select_prepared=True) == pinned
    assert plain(small, 4096, 16, 128, 10, "MSE", "mean", None, False, True, mean_prepared=True, per_query_prepared=True) == pinned
    with pytest.raises(TypeError):
        plain(small, 4096, 16, 128, 10, "MSE", "mean", 0, False, False, True)          # keyword only


def test_without_the_opt_in_every_answer_is_what_it_was(monkeypatch):
    """``mean_prepared=False`` (the default): the tuples tests/test_token_mse_prefilter_cpu.py, test_token_mse_pq_cpu.py and
    test_token_mse_select_topt_cpu.py pin, answer for answer; and the opt-in changes nothing for a request that is not 'mean'."""
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    plain = search.token_mse_route_refusal
    small = search.TOKEN_MSE_PREFILTER_MIN_Q_SMALL
    kw = dict(top_t_prepared=True, select_prepared=True)
    pinned = "combine 'mean' under a distance metric"
    cases = [((2048, 4096, 16, 128, 10, "MSE", "mean"), {}, pinned),
             ((2048, 4096, 16, 128, 10, "MSE", MEAN), {}, pinned),
             ((small, 4096, 16, 128, 10, "MSE", "mean", 2), kw, pinned),
             ((small, 4096, 16, 128, 10, "MSE", "mean", None, True), kw, pinned),
             ((small, 4096, 16, 128, 10, "MSE", "mean", None, False, True), dict(per_query_prepared=True), pinned),
             ((2048, 4096, 16, 128, 10, "MAE", "mean"), {}, "metric MAE (a distance that is no dot product)"),
             ((2048, 4096, 16, 128, 10, "MSE", "max"), dict(top_t=2), "top_t under a distance metric"),
             ((2048, 4096, 16, 128, 10, "MSE", "max"), dict(select=True), "select under a distance metric"),
             ((2048, 4096, 16, 128, 10, "MSE", "max"), {}, None),
             ((small, 4096, 16, 128, 10, "MSE", "max", 2), kw, None),
             ((17, 4096, 16, 128, 10, "MSE", "min", None, False, True), {}, "per-query weights")]
    for args, kws, want in cases:
        assert plain(*args, **kws) == want == plain(*args, mean_prepared=False, **kws), (args, kws)
        if args[6] not in ("mean", MEAN):
            assert plain(*args, mean_prepared=True, **kws) == want, (args, kws)


def test_prepare_mse_mean_needs_a_resident_bank():
    tb = search.TokenBank.__new__(search.TokenBank)
    tb._resident, tb._mse_mean = False, None
    with pytest.raises(ValueError, match="TokenBank.resident"):
        tb.prepare_mse_mean()
    tb._resident = True
    with pytest.raises(ValueError, match="prepare_mse_mean"):
        tb.stage1_mse_mean(None)


@pytest.mark.parametrize("D", [128, 160, 768, 4096])
def test_exported_eps_and_gamma_match_the_restatement(D):
    for dt in ("f16", "bf16"):
        for lo in (False, True):
            assert ops.token_mse_mean_prefilter_eps(D, DT[dt], lo) == mr.eps(D, lo, dt)
            assert ops.token_mse_mean_prefilter_eps(D, DT[dt], lo) == ops.token_mean_prefilter_eps_m(D, DT[dt], lo) + 2.0 ** -22
    for P in (1, 2, 4, 8, 16, 32, 64):
        g = ops.token_mse_mean_prefilter_gamma(D, P)
        assert g == mr.gamma(D, P) == ops.token_mse_prefilter_gamma(D) + P * 2.0 ** -24
        assert mr.check_gamma(g, D, P)


def _bank_np(rng, N, P, D, dt):
    x = (rng.standard_normal((N, 1, D)) * rng.uniform(0.3, 2.0, (N, 1, 1)) + 0.7 * rng.standard_normal((N, P, D))).astype(np.float32)
    return mpr.to16(x, dt)


def test_checkers_reject_planted_defects():
    rng = np.random.default_rng(5)
    N, P, D = 40, 4, 128
    for dt in ("f16", "bf16"):
        x = _bank_np(rng, N, P, D, dt)
        c = (rng.random(D).astype(np.float32) + 0.1)
        c = (c / c.sum()).astype(np.float32)
        pr = mr.pooled_rows(x, dt)
        assert mr.check_pooled(pr["pooled"], x, dt)
        # (1) a pooled element one ulp (of the 16-bit format) off
        off = pr["pooled"].copy()
        v = off[7, 11]
        off[7, 11] = mpr.to16(np.array([v * (1 + (2.0 ** -10 if dt == "f16" else 2.0 ** -7))], np.float32), dt)[0]
        assert off[7, 11] != v and not mr.check_pooled(off, x, dt)
        # (2) Bbar_dn raised instead of lowered
        rc = mr.row_constants(c, x, dt)
        s = rc["s"].astype(np.float64)
        good = np.stack([rc["Bbar_dn"] * s, rc["R1_64"] * (1 + 2.0 ** -12), s, np.zeros(N)], axis=1)
        assert mr.check_rowp(good, c, x, dt)
        raised = good.copy()
        raised[:, 0] = rc["Bbar64"] * (1.0 + mr.bbar_slack(P, D)) * s
        assert not mr.check_rowp(raised, c, x, dt)
        low_norm = good.copy()
        low_norm[3, 1] = rc["R1_64"][3] * (1 - 2.0 ** -12)
        assert not mr.check_rowp(low_norm, c, x, dt)
    # (3) a gamma without the P term
    for D in (128, 768):
        assert mr.check_gamma(mr.gamma(D, 64), D, 64)
        assert not mr.check_gamma(mpr.gamma(D), D, 64) and not mr.check_gamma(mpr.gamma(D), D, 16)


@pytest.mark.parametrize("dt,lo,P", [("f16", True, 4), ("f16", False, 16), ("bf16", True, 64), ("bf16", False, 1)])
def test_lower_bound_holds_against_the_contract_mean(dt, lo, P):
    """L <= D mean (1 + gamma) + 2^-126 for every trusted pair, against the fp64 mean and against the contract's fp32 value, under
    three models of stage 1's dot products (the exact sum rounded to fp32, and that value moved by the accumulation term either way)."""
    rng = np.random.default_rng(P)
    N, D, Q = 96, 128, 12
    x = _bank_np(rng, N, P, D, dt)
    x[5] = np.stack([x[5, 0] if p % 2 == 0 else -x[5, 0] for p in range(P)]) if P > 1 else 0.0      # a pooled row of exact zero
    t = rng.standard_normal((Q, D)).astype(np.float32)
    t[1] = x[9].mean(axis=0)
    c = rng.random(D).astype(np.float32) + 0.05
    c = (c / c.sum()).astype(np.float32)
    dist32 = mr.contract_mean(c, t, x).astype(np.float64)
    d64 = (c.astype(np.float64) * (x.astype(np.float64)[None] - t.astype(np.float64)[:, None, None]) ** 2).sum(axis=3).mean(axis=2)
    L, trusted, dot = mr.lower_bounds(c, t, x, dt, lo)
    assert trusted.all()
    g = mr.gamma(D, P)
    qc = mr.query_constants(c, t, dt, lo)
    acc = 6.06 * D * 2.0 ** -24 * np.sqrt((qc["qh"].astype(np.float64) ** 2).sum(axis=1))[:, None] * \
        np.sqrt((mr.pooled_rows(x, dt)["pooled"].astype(np.float64) ** 2).sum(axis=1))[None, :]
    for moved in (dot, dot + acc, dot - acc):
        Lm, _, _ = mr.lower_bounds(c, t, x, dt, lo, dot=moved)
        assert (Lm <= d64 * (1.0 + g) + 2.0 ** -126).all()
        assert (Lm <= dist32 * D * (1.0 + g) + 2.0 ** -126).all()
    if P > 1:
        assert not mr.pooled_rows(x, dt)["pooled"][5].any() and not mr.pooled_rows(x, dt)["bad"][5]


def test_contract_mean_is_the_token_order_fold():
    rng = np.random.default_rng(2)
    N, P, D, Q = 20, 8, 128, 3
    x = _bank_np(rng, N, P, D, "f16")
    x[4, 3, 7] = np.nan
    t = rng.standard_normal((Q, D)).astype(np.float32)
    c = np.full(D, 1.0 / D, np.float32)
    m = mr.contract_mean(c, t, x)
    d = mpr.contract_distances(c, t, x.reshape(N * P, D)).reshape(Q, N, P)
    acc = np.zeros((Q, N), np.float32)
    for p in range(P):
        acc = acc + d[:, :, p]
    want = acc / np.float32(P)
    ok = np.arange(N) != 4
    assert np.array_equal(m[:, ok].view(np.uint32), want[:, ok].view(np.uint32)) and np.isposinf(m[:, 4]).all()
    dd, ii = mr.topk(m, N)
    assert (ii[:, -1] == -1).all() and np.isposinf(dd[:, -1]).all() and (np.diff(dd[:, :-1], axis=1) >= 0).all()


def test_bbar_slack_follows_from_the_summation_structure():
    """The lowering of Bbar^ against the roundings of the kernel's own layout, for every D and P the route takes; the count that reads
    P D / 64 fused multiply-adds per lane is rejected where it is wrong (D < 512 leaves lanes idle and the others with 8 P each)."""
    for D in range(128, 4097, 32):
        assert mr.bbar_chain(1, D) == 8 * ((D + 511) // 512) + 6
        for P in (1, 2, 4, 8, 16, 32, 64):
            assert mr.check_bbar_slack(mr.bbar_slack(P, D), P, D), (P, D)
    wrong = lambda P, D: (P * D // 64 + 8) * 2.0 ** -23
    assert not mr.check_bbar_slack(wrong(4, 128), 4, 128) and not mr.check_bbar_slack(wrong(64, 128), 64, 128)
    assert not mr.check_bbar_slack(wrong(4, 160), 4, 160) and not mr.check_bbar_slack(wrong(64, 224), 64, 224)
    assert mr.check_bbar_slack(wrong(64, 512), 64, 512)                               # (it is right where 512 divides D)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_bbar_worst_case_rounds_up_at_every_step_and_stays_bounded(dt):
    """The adversarial bank of the GPU file: the fp32 sum in the kernel's order exceeds the real Bbar by ~(8 P - 1) 2^-24 -- more than
    the P D / 64 count would have lowered it by --, and the stated lowering brings it back below."""
    from tests import test_token_mse_mean_gpu as g
    x, c = g.bbar_adversary(dt)
    N, P, D = x.shape
    assert np.array_equal(mpr.to16(x, dt), x)
    real = (c.astype(np.float64) * x.astype(np.float64) ** 2).sum(axis=(1, 2)) / P
    got = mr.bbar_kernel_order(c, x).astype(np.float64)
    assert (got > real * (1.0 + 400 * 2.0 ** -24)).all()
    assert (got * (1.0 - (P * D // 64 + 8) * 2.0 ** -23) > real).all()                # the wrong count: Bbar_dn > Bbar
    assert (got * (1.0 - mr.bbar_slack(P, D)) <= real).all()


def _conditions(x, q, c, dt, lo, k, Dn, skip=()):
    """No flagged query (but ``skip``), and a candidate list that holds every image of the bank: the slots of a query's list as the
    library lays its workspace out."""
    N, Q = x.shape[0], q.shape[0]
    assert N <= ops.topk_prefilter_ws_layout(Q, Dn, k)["cap"], (N, k)
    flagged = mr.query_constants(c, q, dt, bool(lo))["flagged"]
    assert sorted(np.nonzero(flagged)[0].tolist()) == sorted(skip), np.nonzero(flagged)[0]


def test_gpu_cases_meet_the_conditions_of_their_inputs():
    """For every case of tests/test_token_mse_mean_gpu.py -- the bit-equality cases, D = 160, the read-back, the hostile banks (whose
    zero query is the one flagged query), the opt-in test before and after set_weights: the restatement flags no query, and no query
    can have more stage-1 candidates in a slice than its list takes -- every image of the bank fits, whatever the thresholds.  (The
    negative-weight case is flagged whole, by design: ``redone == Q`` there.)"""
    from tests import test_token_mse_mean_gpu as g
    for case in g.CASES:
        N, P, dt, lo, Q, k, weighted, off = case
        x, q, w = g.inputs(case)
        _conditions(x, q, g.weights_c(w, g.D), dt, lo, k, g.D)
        assert search.token_mse_route_refusal(Q, N, P, g.D, k, "MSE", "mean", mean_prepared=True) in (
            None, f"Q = {Q} < TOKEN_MSE_PREFILTER_MIN_Q_SMALL = {search.TOKEN_MSE_PREFILTER_MIN_Q_SMALL} (a bank of fewer than "
                  f"TOKEN_MSE_PREFILTER_MIN_ELEMENTS = {search.TOKEN_MSE_PREFILTER_MIN_ELEMENTS} elements)")
    for dt, lo, k in g.D160_PARAMS:
        x, q, c = g.d160_inputs(dt, lo, k)
        _conditions(x, q, c, dt, lo, k, 160)
    for dt, lo in g.READBACK_PARAMS:
        x, q, c = g.readback_inputs(dt, lo)
        _conditions(x, q, c, dt, lo, 8, g.D)
    for dt, lo, k in g.HOSTILE_PARAMS:
        _, x, q = g.hostile_inputs(dt)
        _conditions(x, q, g.weights_c(None, g.D), dt, lo, k, g.D, skip=(g.HOSTILE_ZERO_QUERY,))
    x, q, w = g.optin_inputs()
    for ww in (None, w):
        _conditions(x, q, g.weights_c(ww, g.D), "f16", 1, 8, g.D)
    assert mr.query_constants(np.where(np.arange(g.D) == 5, -0.25, 1.0).astype(np.float32), q, "f16", True)["flagged"].all()
