"""CPU: the bound of the two-stage token search under combine 'mean' (tests/token_mean_prefilter_reference.py) holds against the
contract mean of tests/token_search_reference.py, is as tight as stated, recognises what it cannot bound, and the route decision
and the C ABI carry the new entries."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from oracle import similarity_oracle as so
from sky_embeddings_amd import _lib, ops, search
from tests import prefilter_stage1_reference as sr
from tests import token_mean_prefilter_reference as mr
from tests import token_search_reference as tsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = ("fp16", "bf16")


def store(a, fmt):
    """float32 values a 16-bit bank of `fmt` holds after rounding `a` to it."""
    return mr.round16(np.asarray(a, np.float32), fmt)


def bank_of(kind, fmt, N, P, D, rng):
    x = rng.standard_normal((N, P, D)).astype(np.float32)
    if kind == "mixed":                       # token norms 2^-10 .. 2^10 inside one image
        x *= np.exp2(rng.integers(-10, 11, (N, P, 1))).astype(np.float32)
    elif kind == "cancel":                    # tokens come in pairs (t, -t): m = 0 exactly; odd images nearly so
        if P > 1:
            x[:, 1::2] = -x[:, 0::2]
            x[1::2, 1] *= np.float32(1 + 2.0 ** -9)
    elif kind == "aligned":                   # near-parallel tokens: the pooled row is as long as a unit token
        x = (rng.standard_normal((N, 1, D)) + 0.1 * rng.standard_normal((N, P, D))).astype(np.float32)
    elif kind == "subnormal":                 # a third of the elements below the format's normal range (bf16: far down its window)
        tiny = rng.random((N, P, D)) < 0.33
        x = np.where(tiny, x * np.float32(2.0 ** -18 if fmt == "fp16" else 2.0 ** -50), x)
    return store(x, fmt)


def case(kind, fmt, N, P, D, seed, Q=6, weights="random", anti=False):
    rng = np.random.default_rng(seed)
    x = bank_of(kind, fmt, N, P, D, rng)
    if weights == "unit":
        w = None
    elif weights == "signed":                 # a few negative weights: the norms stay real, Cauchy-Schwarz on them does not hold
        w = (rng.random(D) + 0.1).astype(np.float32)
        w[rng.choice(D, 4, replace=False)] = -0.05
    else:
        w = (rng.random(D) + 0.1).astype(np.float32)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    if anti:                                  # every token scores negative: the eps term has the other sign
        q = -x.reshape(N * P, D)[rng.integers(0, N * P, Q)] - 3 * x.mean(axis=(0, 1))
        x = store(np.abs(x), fmt)
        q = -np.abs(q)
    xn = so.wnorms_np(x.reshape(N * P, D), w)
    tw, qn = so.prep_queries_np(q, w)
    return x, xn, w, q, tw, qn


def bound_gap(x, xn, w, q, tw, qn, fmt, lo, eps):
    """(U - contract mean, eps_m in cosine units, refs) over the boundable images and accepted queries; asserts the kernel's test
    passes every pair at tau = its own contract mean."""
    N, P, D = x.shape
    pref = mr.pool(x, xn, fmt)
    qref = mr.query_side(tw, qn, fmt, D, lo, eps)
    rowp = mr.model_rowp(pref)
    dot = mr.dot_hat(qref, pref)
    U = mr.upper_bound(dot, qref, rowp)
    mean = tsr.combined_scores(q, x, "mean", w, eps).astype(np.float64)
    keep = ~qref["flagged"][:, None] & ~pref["unboundable"][None, :] & np.isfinite(mean)
    assert keep.any()
    gap = U - mean
    assert (gap[keep] >= 0).all(), f"U < contract mean: worst {gap[keep].min():.3e}"
    # the fp32 test at the tightest threshold each pair must pass: its own contract mean
    assert mr.passes(dot, qref, rowp, mean.astype(np.float32))[keep].all()
    mr.check_error_c(x, xn, pref)
    return gap, mr.eps_m_cosine(qref, fmt, D)[:, None] * np.ones_like(gap), keep, pref, qref


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("lo", (False, True))
@pytest.mark.parametrize("P,D", ((1, 128), (4, 160), (64, 128), (4, 768), (64, 160)))
def test_bound_holds_on_random_banks_and_is_tight(fmt, lo, P, D):
    x, xn, w, q, tw, qn = case("random", fmt, 24 if P == 64 else 64, P, D, seed=P + D, weights="unit")
    for eps in (1e-6, 1e-2):
        gap, em, keep, pref, _ = bound_gap(x, xn, w, q, tw, qn, fmt, lo, eps)
        assert not pref["unboundable"].any()
        if eps == 1e-6:
            ratio = np.median(gap[keep] / em[keep])
            print(f"{fmt} lo={lo} P={P} D={D}: median (U - mean) / eps_m = {ratio:.3f}")
            assert ratio <= 4.0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", ("mixed", "cancel", "aligned", "subnormal"))
@pytest.mark.parametrize("weights", ("random", "signed"))
def test_bound_holds_on_hard_banks(fmt, kind, weights):
    for P, D, lo in ((4, 128, False), (64, 160, True), (1, 160, True)):
        x, xn, w, q, tw, qn = case(kind, fmt, 32, P, D, seed=7 * P + D, weights=weights)
        for eps in (1e-6, 1e-2):
            bound_gap(x, xn, w, q, tw, qn, fmt, lo, eps)


@pytest.mark.parametrize("fmt", FMTS)
def test_bound_holds_for_anti_aligned_queries(fmt):
    for P, D in ((4, 128), (64, 160)):
        x, xn, w, q, tw, qn = case("aligned", fmt, 32, P, D, seed=3, anti=True)
        mean = tsr.combined_scores(q, x, "mean", w, 1e-2)
        assert (mean < 0).all()
        for eps in (1e-6, 1e-2):
            bound_gap(x, xn, w, q, tw, qn, fmt, True, eps)


@pytest.mark.parametrize("fmt", FMTS)
def test_aligned_images_are_bounded_within_a_few_eps_m(fmt):
    """The pooled row of near-parallel tokens is as long as a unit token: here the bound is at its loosest in cosine units."""
    x, xn, w, q, tw, qn = case("aligned", fmt, 32, 16, 128, seed=11, weights="unit")
    gap, em, keep, _, _ = bound_gap(x, xn, w, q, tw, qn, fmt, True, 1e-6)
    ratio = np.median(gap[keep] / em[keep])
    print(f"{fmt}: aligned tokens, median (U - mean) / eps_m = {ratio:.3f}")
    assert ratio <= 4.0


@pytest.mark.parametrize("fmt", FMTS)
def test_unboundable_images_are_recognised(fmt):
    rng = np.random.default_rng(5)
    N, P, D = 24, 4, 128
    x = bank_of("random", fmt, N, P, D, rng)
    x[1, 2, 5] = np.nan
    x[3, 0, 7] = np.inf
    x[5, 1] = 0                                                    # an all-zero token: norm 0
    if fmt == "bf16":
        x[7, 3, 9] = 2.0 ** -70
        x[9, 0, 1] = 2.0 ** 121
    with np.errstate(all="ignore"):
        xn = so.wnorms_np(x.reshape(N * P, D), None)
    xn[11 * P + 2] = 2.0 ** -41                                    # norms outside the window (as another weighting could give)
    xn[13 * P] = 2.0 ** 41
    xn[15 * P + 1] = np.inf
    ref = mr.pool(x, xn, fmt)
    want = {1, 3, 5, 11, 13, 15} | ({7, 9} if fmt == "bf16" else set())
    assert set(np.nonzero(ref["unboundable"])[0].tolist()) == want
    rowp = mr.model_rowp(ref, 256)
    assert (rowp[sorted(want)] == np.array([0, np.inf, 1, 0], np.float32)).all() and (ref["m16"][sorted(want)] == 0).all()
    assert np.isnan(rowp[N:, 1]).all()
    # a candidate of every query, whatever the threshold
    q = rng.standard_normal((3, D)).astype(np.float32)
    tw, qn = so.prep_queries_np(q, None)
    qref = mr.query_side(tw, qn, fmt, D, True, 1e-6)
    ok = mr.passes(mr.dot_hat(qref, ref), qref, rowp[:N], np.full(3, 1e30, np.float32))
    assert ok[:, sorted(want)].all() and ok.sum() == 3 * len(want)


@pytest.mark.parametrize("fmt", FMTS)
def test_queries_outside_the_windows_are_flagged(fmt):
    D = 128
    rng = np.random.default_rng(2)
    q = rng.standard_normal((6, D)).astype(np.float32)
    q[1] = 0
    q[2] *= np.float32(2.0 ** -30)
    q[3] *= np.float32(2.0 ** 30)
    tw, qn = so.prep_queries_np(q, None)
    ref = mr.query_side(tw, qn, fmt, D, True, 1e-6)
    assert ref["flagged"].tolist() == [False, True, True, True, False, False]
    assert mr.query_side(tw, qn, fmt, D, True, -1e-6)["flagged"].all()


def test_library_states_the_same_eps_m():
    for D in (128, 160, 768, 4096):
        for lo in (False, True):
            assert ops.token_mean_prefilter_eps_m(D, torch.float16, lo) == mr.eps_m("fp16", D, lo)
            assert ops.token_mean_prefilter_eps_m(D, torch.bfloat16, lo) == mr.eps_m("bf16", D, lo)
            assert ops.token_mean_prefilter_eps_m(D, torch.float16, lo) == ops.topk_prefilter_eps_a(D, lo, False)


def _request(**kw):
    tb = search.TokenBank.__new__(search.TokenBank)               # no device: the decision reads the flags only
    tb._resident, tb.dtype = True, torch.float16
    base = dict(who="cosine_topk_tokens", Q=300, N=4096, P=16, D=128, k=10, combine=ops.COMBINE_CODES["mean"], metric=None,
                metric_name=None, top_t=0, per_query=False, step=16, idx_offset=0, tokens=None, bank=tb, weights=None, select=None)
    base.update(kw)
    return search.TokenRequest(**base)


def test_route_decision_for_mean(monkeypatch):
    """'mean' over a resident bank takes the two-stage route under its own shape rule and its own smallest Q; everything the
    route leaves out keeps the grouped route, with a reason that names it."""
    monkeypatch.setattr(search, "TOKEN_MEAN_PREFILTER_MIN_Q", 17)
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 100000)   # the min / max constant does not decide for mean
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    refusal = search._token_prefilter_refusal
    assert refusal(_request()) is None
    for P in (1, 2, 4, 8, 16, 32, 64):
        assert refusal(_request(P=P, N=2048)) is None                      # rows = images: N >= 2048 whatever P
        assert "N >= 2048" in refusal(_request(P=P, N=2047))
    assert refusal(_request(Q=17, k=256, D=4096, idx_offset=5)) is None
    fp32 = search.TokenBank.__new__(search.TokenBank)
    fp32._resident, fp32.dtype = False, torch.float32
    sel = search.Selection.__new__(search.Selection)
    sel.count = 4096
    named = dict(select=(sel, "select"), top_t=(4, "top_t"), per_query=(True, "per-query weights"), bank=(fp32, "fp32"),
                 metric=(ops.METRIC_CODES["MSE"], "distance metric"), Q=(16, "TOKEN_MEAN_PREFILTER_MIN_Q"), P=(48, "divide 64"),
                 D=(144, "D % 32"), k=(257, "k <= 256"), N=(2 ** 27, "2^31"))
    for field, (v, word) in named.items():
        why = refusal(_request(**{field: v}))
        assert isinstance(why, str) and word in why, (field, why)
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    assert "SKYEMB_TOPK_PREFILTER" in refusal(_request())
    assert dataclasses.is_dataclass(search.TokenRequest)


def test_new_symbols_are_exported_with_the_declared_signatures():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skyemb.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.build())
    for name in ("skyemb_token_mean_pool", "skyemb_token_mean_prefilter_applicable", "skyemb_token_mean_prefilter_ws_bytes",
                 "skyemb_cosine_topk_tokens_mean_prefiltered"):
        m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/skyemb.h"
        assert hasattr(L, name), f"{name} is not exported"
        res, args = _lib.PROTOTYPES[name]
        assert res is (ctypes.c_int64 if m.group(1) == "int64_t" else ctypes.c_int32)
        assert len([p for p in m.group(2).split(",")]) == len(args), name
    ops_lib = _lib.lib()
    assert ops_lib.skyemb_token_mean_prefilter_applicable(300, 2048, 64, 768, 100) == 1
    assert ops_lib.skyemb_token_mean_prefilter_applicable(300, 2047, 64, 768, 100) == 0
    assert b"N >= 2048" in ops_lib.skyemb_last_error()
    assert ops_lib.skyemb_token_mean_prefilter_ws_bytes(300, 768, 100) == ops_lib.skyemb_token_prefilter_ws_bytes(300, 768, 100)
    # argument checks come before any device work
    assert ops_lib.skyemb_token_mean_pool(None, 2, None, 10, 4, 128, None, None, None, None) != 0
    assert b"null argument" in ops_lib.skyemb_last_error()
