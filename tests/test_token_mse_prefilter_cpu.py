"""CPU: the bound of the two-stage weighted-MSE token search (tests/token_mse_prefilter_reference.py restates its constants) holds
the contract's distance (tests/token_distance_reference.py) for every pair of a sweep; rows and queries the bound cannot serve are
classified as include/skyemb.h says; the route decision; the new symbols."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from sky_embeddings_amd import _lib, ops, search
from tests import token_distance_reference as tdr
from tests import token_mse_prefilter_reference as mpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sweep(D, dt, seed):
    """(c, t [Q, D], x [R, D] widened 16-bit rows): random standardised rows and queries; rows equal to a query (distance 0: the
    three terms cancel completely); rows of +-65504; fp16-subnormal rows; rows next to a query."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((12, D)).astype(np.float32)
    x = rng.standard_normal((40, D)).astype(np.float32)
    t[8] *= 1e-3
    t[9] *= 300.0
    x[30] = 65504.0
    x[31] = -65504.0
    x[32] = 65504.0 * np.sign(rng.standard_normal(D))
    x[33] = 2.0 ** -20 * rng.integers(-15, 16, D)                  # fp16 subnormals (and zeros)
    x[34] = 0.0
    x[35, ::2] = 2.0 ** -24
    x[36:40] = t[0:4] + 1e-3 * rng.standard_normal((4, D)).astype(np.float32)
    x = mpr.to16(x, dt)
    t[0:4] = x[20:24]                                              # queries that ARE bank rows
    t[10] = x[30]
    t[11] = x[33]
    return t, x


def _weights(D, kind, rng):
    w = rng.random(D).astype(np.float32) + 0.05
    if kind == "zeros":
        w[rng.random(D) < 0.5] = 0.0
    elif kind == "dominant":
        w[:] = 1e-6
        w[D // 3] = 1.0
    elif kind == "ones":
        w[:] = 1.0
    return tdr.prepare_c(w, D)


@pytest.mark.parametrize("D", [128, 160, 768])
@pytest.mark.parametrize("lo", [False, True], ids=["hi", "hilo"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_the_interval_contains_the_contract_distance(dt, lo, D):
    rng = np.random.default_rng(D + 7)
    for n, kind in enumerate(("ones", "random", "zeros", "dominant")):
        c = _weights(D, kind, rng)
        t, x = _sweep(D, dt, 100 * D + n)
        dist = mpr.contract_distances(c, t, x)
        if D % 64 == 0:                                            # the contract as tests/token_distance_reference.py states it
            ref = tdr.token_distances(c, t, x[:, None, :], "MSE")[:, :, 0]
            assert np.array_equal(dist.view(np.uint32), ref.view(np.uint32))
        L, U, trusted = mpr.interval(c, t, x, dt, lo)
        assert trusted.all(), (kind, np.argwhere(~trusted)[:4])
        ok = mpr.contains(L, U, dist, D)
        assert ok.all(), (kind, np.argwhere(~ok)[:4], L[~ok][:4], U[~ok][:4], (dist[~ok] * D)[:4])
        assert (dist[np.arange(4), 20 + np.arange(4)] == 0).all()   # the cancelling pairs were in the sweep
        # ... and the bound is worth something.  Unit weights, standardised rows and queries: D dist ~ 2 and the interval's half
        # width is 2 eps_mse ||tw|| ||x|| ~ 2 eps_mse, so L is within 2 eps_mse (bf16, hi only: 2^-8) of it -- asked within 4 x that
        if kind == "ones":
            rel = (dist[4:8, :20].astype(np.float64) * D - L[4:8, :20]) / (dist[4:8, :20].astype(np.float64) * D)
            assert rel.max() < 8 * mpr.eps_mse(D, lo, dt), rel.max()


def test_unboundable_rows_and_flagged_queries():
    D = 128
    rng = np.random.default_rng(3)
    c = tdr.prepare_c(None, D)
    x = rng.standard_normal((8, D)).astype(np.float32)
    x[1, 5] = np.inf
    x[2, 7] = np.nan
    x[3, 9] = 1e-30                                                # bf16: below the window; fp16: rounds to zero
    x[4, 11] = 3e37                                                # bf16: above the window; fp16: inf
    x[5] = 2.0 ** 50                                               # bf16: B_r = 2^100 >= 2^96
    for dt, want in (("f16", [0, 1, 1, 0, 1, 1, 0, 0]), ("bf16", [0, 1, 1, 1, 1, 1, 0, 0])):
        ub = mpr.row_constants(c, mpr.to16(x, dt), dt)[3]
        assert ub.tolist() == [bool(v) for v in want], (dt, ub)
    t = rng.standard_normal((6, D)).astype(np.float32)
    t[1] = 0.0                                                     # tw = 0
    t[2] *= 1e-30                                                  # fp16: scale 2^-f >= 2^90; bf16: >= 2^30
    t[3] *= 1e30                                                   # bf16: scale <= 2^-100 (clamped); A_q overflows fp32 in both
    t[4] *= 1e15                                                   # fine in both formats
    for dt in ("f16", "bf16"):
        assert mpr.query_constants(c, t, dt, False)["flagged"].tolist() == [False, True, True, True, False, False], dt
    for bad in (-1e-3, np.nan, 2048.0):
        cb = c.copy()
        cb[17] = bad
        assert mpr.weights_flagged(cb) and mpr.query_constants(cb, t, "f16", True)["flagged"].all()
    assert not mpr.weights_flagged(c)


def test_constants_follow_the_library():
    for D in (128, 160, 768, 4096):
        assert mpr.gamma(D) == ops.token_mse_prefilter_gamma(D)
        for lo in (False, True):
            assert mpr.eps_mse(D, lo, "f16") == ops.token_mse_prefilter_eps(D, torch.float16, lo)
            assert mpr.eps_mse(D, lo, "bf16") == ops.token_mse_prefilter_eps(D, torch.bfloat16, lo)
            assert mpr.eps_mse(D, lo, "f16") == ops.topk_prefilter_eps_a_resident(D, torch.float16, lo) + 2.0 ** -22
        # gamma covers the chain's roundings, counted on the chain itself: the fullest partial of contract_distances' loop holds
        # m terms, and a term carries four factors (1 + d) (the subtraction twice), then m additions, four folds, one division
        m = max(sum(1 for d in range(D) if (d >> 2) & 15 == j) for j in range(16))
        assert m == 4 * -(-D // 64) and (m == D // 16 if D % 64 == 0 else True)
        n = 4 + m + 4 + 1
        assert n == mpr.chain_roundings(D)
        assert (1.0 - 2.0 ** -24) ** -n <= 1.0 + mpr.gamma(D)


def _request(**kw):
    tb = search.TokenBank.__new__(search.TokenBank)               # no device: the decision reads the flag only
    tb._resident = True
    tb.dtype = torch.float16
    base = dict(who="distance_topk_tokens", Q=2048, N=4096, P=16, D=128, k=10, combine=ops.COMBINE_CODES["min"],
                metric=ops.METRIC_CODES["MSE"], metric_name="MSE", top_t=0, per_query=False, step=16, idx_offset=0, tokens=None, bank=tb,
                weights=None, select=None)
    base.update(kw)
    return search.TokenRequest(**base)


def test_route_decision(monkeypatch):
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    refusal = search._token_prefilter_refusal
    assert search.TOKEN_MSE_PREFILTER_MIN_Q in (32, 64, 128, 256, 512, 1024)      # a point of the measured grid
    assert refusal(_request()) is None
    assert refusal(_request(combine=ops.COMBINE_CODES["max"], P=1, N=2092, k=256)) is None
    for P in (1, 2, 4, 8, 16, 32, 64):
        assert refusal(_request(P=P, N=4096 * 16 // P)) is None
    plain = search.TokenBank.__new__(search.TokenBank)
    plain._resident, plain.dtype = False, torch.float16
    f32 = search.TokenBank.__new__(search.TokenBank)
    f32._resident, f32.dtype = False, torch.float32
    assert refusal(_request(bank=f32)) == "an fp32 token bank"
    assert refusal(_request(bank=plain)) == refusal(_request(bank=None)) == "the bank was not made by TokenBank.resident"
    assert "MAE" in refusal(_request(metric=ops.METRIC_CODES["MAE"], metric_name="MAE"))
    assert refusal(_request(combine=ops.COMBINE_CODES["mean"])) == "combine 'mean' under a distance metric"
    assert refusal(_request(top_t=2)) == "top_t under a distance metric"
    assert refusal(_request(select=object())) == "select under a distance metric"
    assert refusal(_request(per_query=True)) == "per-query weights"
    assert refusal(_request(P=48)) == "P = 48 does not divide 64"
    # the first reason wins: MAE with a selection and P = 48 names the metric
    assert "MAE" in refusal(_request(metric=ops.METRIC_CODES["MAE"], metric_name="MAE", select=object(), P=48))
    assert "N * P" in refusal(_request(N=127)) and "k <= N" in refusal(_request(k=257))          # the library's own text
    assert refusal(_request(D=144)) == ops.token_mse_prefilter_refusal(2048, 4096, 16, 144, 10) is not None
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    assert refusal(_request()) == "SKYEMB_TOPK_PREFILTER=0"
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER")
    # the measured constant holds from the measured bank size on; a smaller bank waits for the grid's largest Q
    Qmin, Qsmall, big = search.TOKEN_MSE_PREFILTER_MIN_Q, search.TOKEN_MSE_PREFILTER_MIN_Q_SMALL, dict(N=15625, P=64, D=768)
    assert search.TOKEN_MSE_PREFILTER_MIN_ELEMENTS == 15625 * 64 * 768 and Qmin <= Qsmall == 1024
    assert refusal(_request(Q=Qmin, **big)) is None
    assert refusal(_request(Q=Qmin - 1, **big)) == f"Q = {Qmin - 1} < TOKEN_MSE_PREFILTER_MIN_Q = {Qmin}"
    assert refusal(_request(Q=Qsmall)) is None
    assert refusal(_request(Q=Qsmall - 1)).startswith(f"Q = {Qsmall - 1} < TOKEN_MSE_PREFILTER_MIN_Q_SMALL = {Qsmall}")
    assert refusal(_request(Q=Qsmall - 1, N=15624, P=64, D=768)).startswith(f"Q = {Qsmall - 1} < TOKEN_MSE_PREFILTER_MIN_Q_SMALL")
    monkeypatch.setattr(search, "TOKEN_MSE_PREFILTER_MIN_Q_SMALL", 17)
    assert refusal(_request(Q=17)) is None and "TOKEN_MSE_PREFILTER_MIN_Q_SMALL" in refusal(_request(Q=16))
    # the same decision from plain facts, for a caller that has not wrapped its bank yet (similarity_search.py)
    plain_facts = search.token_mse_route_refusal
    assert plain_facts(17, 4096, 16, 128, 10, 'MSE', 'min') is None and plain_facts(17, 4096, 16, 128, 10, 'MSE', 'max', None) is None
    assert plain_facts(16, 4096, 16, 128, 10, 'MSE', 'min') == refusal(_request(Q=16))
    assert 'MAE' in plain_facts(17, 4096, 16, 128, 10, 'MAE', 'min') and 'mean' in plain_facts(17, 4096, 16, 128, 10, 'MSE', 'mean')
    assert plain_facts(17, 4096, 16, 128, 10, 'MSE', 'min', 2) == 'top_t under a distance metric'
    assert plain_facts(17, 4096, 16, 128, 10, 'MSE', 'min', None, True) == 'select under a distance metric'
    assert plain_facts(17, 4096, 16, 128, 10, 'MSE', 'min', None, False, True) == 'per-query weights'
    # the cosine decision is untouched
    cos = dataclasses.replace(_request(Q=4096), metric=None, metric_name=None, who="cosine_topk_tokens")
    assert refusal(cos) is None


def test_new_symbols_are_exported_and_the_version_stands():
    names = ("skyemb_token_mse_prefilter_applicable", "skyemb_token_mse_prefilter_eps", "skyemb_token_mse_prefilter_gamma",
             "skyemb_token_mse_rowp", "skyemb_distance_topk_tokens_prefiltered")
    header = open(os.path.join(ROOT, "include", "skyemb.h")).read()
    L = _lib.lib()
    for n in names:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.PROTOTYPES and hasattr(L, n), n
    assert L.skyemb_version() == 111 == _lib.ABI_VERSION
    assert ops.token_mse_prefilter_refusal(300, 523, 4, 160, 8) is None
    assert ops.token_mse_prefilter_refusal(300, 500, 4, 160, 8).startswith("many-query weighted-MSE patch-token search")
    assert callable(ops.token_mse_rowp) and callable(ops.distance_topk_tokens_prefiltered)
    assert hasattr(search.TokenBank, "stage1_mse")
