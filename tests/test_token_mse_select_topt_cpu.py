"""CPU: the two-stage weighted-MSE token search under ``top_t`` and under a selection -- the opted-in route decision and every
refusal text, the unprepared answers (today's strings), the key-space mapping, the new C entries' host refusals, the plans of the
new requests, and the rules of tests/token_mse_select_topt_reference.py against tests/token_distance_reference.py."""
import ctypes
import os
import re
import weakref

import numpy as np
import pytest
import torch

from sky_embeddings_amd import _lib, ops, search
from tests import token_distance_reference as tdr
from tests import token_mse_select_topt_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN, MEAN, MAX = (ops.COMBINE_CODES[c] for c in ("min", "mean", "max"))
NEW = ("skyemb_token_mse_topt_prefilter_applicable", "skyemb_distance_topk_tokens_prefiltered_top",
       "skyemb_distance_topk_tokens_prefiltered_sel", "skyemb_distance_topk_tokens_prefiltered_top_sel")


def _bank(top_t=False):
    tb = search.TokenBank.__new__(search.TokenBank)               # no device: the decision reads the flags only
    tb._resident, tb.dtype = True, torch.float16
    if top_t:
        assert tb.prepare_mse_top_t() is tb
    return tb


def _selection(count, N=4096, asked=None):
    sel = search.Selection.__new__(search.Selection)              # no device either
    sel.N, sel.count, sel._mse = N, count, None
    if asked is not None:
        sel._mse = weakref.WeakKeyDictionary()
        sel._mse[asked] = None
    return sel


def _request(**kw):
    base = dict(who="distance_topk_tokens", Q=2048, N=4096, P=16, D=128, k=10, combine=MAX, metric=ops.METRIC_CODES["MSE"],
                metric_name="MSE", top_t=0, per_query=False, step=16, idx_offset=0, tokens=None, bank=_bank(), weights=None, select=None)
    base.update(kw)
    return search.TokenRequest(**base)


def test_unprepared_requests_answer_as_before(monkeypatch):
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    refusal = search._token_prefilter_refusal
    assert refusal(_request(top_t=2)) == "top_t under a distance metric"
    assert refusal(_request(top_t=2, combine=MIN)) == "top_t under a distance metric"
    assert refusal(_request(select=object())) == "select under a distance metric"
    # a prepared bank does not open the door for an unprepared selection, nor the other way round
    assert refusal(_request(bank=_bank(True), select=object())) == "select under a distance metric"
    tb = _bank()
    assert refusal(_request(bank=tb, top_t=2, select=_selection(2000, asked=tb))) == "top_t under a distance metric"
    # a real Selection never asked: the pinned words, then the way in
    why = refusal(_request(select=_selection(2000)))
    assert why.startswith("select under a distance metric") and "Selection.prepare_mse" in why
    other = _bank()
    why = refusal(_request(bank=tb, select=_selection(2000, asked=other)))          # asked for another bank
    assert why.startswith("select under a distance metric") and "Selection.prepare_mse" in why
    plain = search.token_mse_route_refusal
    assert plain(2048, 4096, 16, 128, 10, "MSE", "max", top_t=2) == "top_t under a distance metric"
    assert plain(2048, 4096, 16, 128, 10, "MSE", "max", select=True) == "select under a distance metric"
    assert plain(2048, 4096, 16, 128, 10, "MSE", "max", 2, True) == "top_t under a distance metric"
    assert plain(2048, 4096, 16, 128, 10, "MSE", "max") is None


def test_opted_in_route_decision(monkeypatch):
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    refusal = search._token_prefilter_refusal
    small = search.TOKEN_MSE_PREFILTER_MIN_Q_SMALL
    for name in ("TOKEN_MSE_TOPT_PREFILTER_MIN_Q", "TOKEN_MSE_SELECT_PREFILTER_MIN_Q", "TOKEN_MSE_SELECT_TOPT_PREFILTER_MIN_Q"):
        assert getattr(search, name) in (32, 64, 128, 256, 512, 1024), name              # a point of the measured grid
    tb = _bank(True)
    sel = _selection(2000, asked=tb)
    for top_t in (1, 2, 15, 16):
        for combine in (MIN, MAX):
            assert refusal(_request(bank=tb, top_t=top_t, combine=combine)) is None, (top_t, combine)
            assert refusal(_request(bank=tb, top_t=top_t, combine=combine, select=sel)) is None
    assert refusal(_request(bank=tb, select=sel)) is None
    assert refusal(_request(bank=_bank(), select=_selection(2000, asked=None))) is not None
    tb2 = _bank()
    assert refusal(_request(bank=tb2, select=_selection(2000, asked=tb2))) is None       # a selection alone needs no bank flag
    for P in (1, 2, 4, 8, 16, 32, 64):
        assert refusal(_request(bank=tb, P=P, N=4096 * 16 // P, top_t=min(P, 3))) is None
    # the reasons that come first stay first
    assert "MAE" in refusal(_request(bank=tb, top_t=2, metric=ops.METRIC_CODES["MAE"], metric_name="MAE"))
    assert refusal(_request(bank=tb, top_t=2, combine=MEAN)) == "combine 'mean' under a distance metric"
    assert refusal(_request(bank=tb, top_t=2, per_query=True)) == "per-query weights"
    assert refusal(_request(bank=tb, top_t=2, P=48)) == "P = 48 does not divide 64"
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    assert refusal(_request(bank=tb, top_t=2, select=sel)) == "SKYEMB_TOPK_PREFILTER=0"
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER")
    # the library's own texts
    assert "top_t must be 1 .. min(P, 16)" in refusal(_request(bank=tb, top_t=17))
    assert "top_t must be 1 .. min(P, 16)" in refusal(_request(bank=tb, top_t=9, P=8, N=8192))
    assert "N * P" in refusal(_request(bank=tb, top_t=2, N=127)) and "k <= N" in refusal(_request(bank=tb, top_t=2, k=257))
    # the selected images are themselves a bank the route takes: selected x P >= 2048 rows, k <= selected
    assert refusal(_request(bank=tb, select=_selection(127, asked=tb))).startswith("the selected images alone: many-query weighted-MSE")
    assert refusal(_request(bank=tb, k=200, select=_selection(199, asked=tb))).startswith("the selected images alone: ")
    assert refusal(_request(bank=tb, k=200, select=_selection(200, asked=tb))) is None
    assert refusal(_request(bank=tb, select=_selection(0, asked=tb))).startswith("the selected images alone: ")
    # the smallest Q: each route names its own constant on a bank of the measured size; a smaller bank waits for the grid's largest Q
    big = dict(N=15625, P=64, D=768)
    monkeypatch.setattr(search, "TOKEN_MSE_PREFILTER_MIN_Q", 64)
    monkeypatch.setattr(search, "TOKEN_MSE_TOPT_PREFILTER_MIN_Q", 128)
    monkeypatch.setattr(search, "TOKEN_MSE_SELECT_PREFILTER_MIN_Q", 256)
    monkeypatch.setattr(search, "TOKEN_MSE_SELECT_TOPT_PREFILTER_MIN_Q", 512)
    selb = _selection(2000, N=15625, asked=tb)
    assert refusal(_request(bank=tb, Q=127, top_t=4, **big)) == "Q = 127 < TOKEN_MSE_TOPT_PREFILTER_MIN_Q = 128"
    assert refusal(_request(bank=tb, Q=128, top_t=4, **big)) is None
    assert refusal(_request(bank=tb, Q=255, select=selb, **big)) == "Q = 255 < TOKEN_MSE_SELECT_PREFILTER_MIN_Q = 256"
    assert refusal(_request(bank=tb, Q=256, select=selb, **big)) is None
    assert refusal(_request(bank=tb, Q=511, top_t=4, select=selb, **big)) == "Q = 511 < TOKEN_MSE_SELECT_TOPT_PREFILTER_MIN_Q = 512"
    assert refusal(_request(bank=tb, Q=512, top_t=4, select=selb, **big)) is None
    # distance 'min' under top_t and 'max' under top_t == P ARE the plain search: its constant
    assert refusal(_request(bank=tb, Q=64, top_t=4, combine=MIN, **big)) is None
    assert refusal(_request(bank=tb, Q=63, top_t=4, combine=MIN, **big)) == "Q = 63 < TOKEN_MSE_PREFILTER_MIN_Q = 64"
    assert refusal(_request(bank=tb, Q=64, top_t=16, N=62500, P=16, D=768)) is None
    assert refusal(_request(bank=tb, Q=255, top_t=4, combine=MIN, select=selb, **big)) == "Q = 255 < TOKEN_MSE_SELECT_PREFILTER_MIN_Q = 256"
    assert refusal(_request(bank=tb, Q=small - 1, top_t=2)).startswith(f"Q = {small - 1} < TOKEN_MSE_PREFILTER_MIN_Q_SMALL = {small}")
    assert refusal(_request(bank=tb, Q=small, top_t=2)) is None
    # the same decision from plain facts (similarity_search.py)
    plain = search.token_mse_route_refusal
    kw = dict(top_t_prepared=True, select_prepared=True)
    assert plain(small, 4096, 16, 128, 10, "MSE", "max", 2, **kw) is None
    assert plain(small, 4096, 16, 128, 10, "MSE", "max", 2, True, selected=2000, **kw) is None
    assert plain(small, 4096, 16, 128, 10, "MSE", "max", None, True, selected=100, **kw).startswith("the selected images alone: ")
    assert plain(small, 4096, 16, 128, 10, "MSE", "max", 2, True, top_t_prepared=True) == "select under a distance metric"
    assert plain(small, 4096, 16, 128, 10, "MSE", "max", 2, True, select_prepared=True) == "top_t under a distance metric"
    assert plain(small, 4096, 16, 128, 10, "MSE", "mean", 2, **kw) == "combine 'mean' under a distance metric"


def test_the_way_in_checks_its_bank():
    tb = search.TokenBank.__new__(search.TokenBank)
    tb._resident = False
    with pytest.raises(ValueError, match="TokenBank.resident"):
        tb.prepare_mse_top_t()
    assert not getattr(tb, "_mse_top_t", False)
    sel = _selection(10)
    with pytest.raises(ValueError, match="TokenBank.resident"):
        sel.prepare_mse(tb)
    with pytest.raises(ValueError, match="TokenBank.resident"):
        sel.prepare_mse(torch.zeros(1))


def test_key_space_mapping():
    for P in (1, 2, 4, 8, 16, 32, 64):
        tp = min(P, 16)
        for top_t in range(0, tp + 1):
            assert ref.key_space_request("min", top_t, P) == ("max", 0)                 # 'min' + top_t is plain
            assert ref.stage_folds("min", top_t, P) == ("or", "max") == ops.token_mse_topt_folds(P, MIN, top_t)
            want = ("min", 0) if top_t in (0, P) else ("min", top_t)                     # top_t == 0 and 'max' + top_t == P are plain
            assert ref.key_space_request("max", top_t, P) == want
            assert ref.stage_folds("max", top_t, P) == ops.token_mse_topt_folds(P, MAX, top_t)
            assert ref.stage_folds("max", top_t, P) == ops.token_topt_folds(P, MIN, top_t)   # the cosine rule, in key space
    assert ref.stage_folds("max", 1, 16) == ("or", "top") and ref.stage_folds("max", 5, 16) == ("count", "top")
    assert ref.stage_folds("max", 16, 16) == ("and", "min") and ref.stage_folds("max", 16, 64) == ("count", "top")


def test_reference_rules_against_the_distance_reference():
    rng = np.random.default_rng(5)
    Q, N, P, k = 5, 60, 8, 9
    a = rng.random((Q, N, P)).astype(np.float32)
    a[:, 3, 2] = np.nan                                                # ranks as +inf
    a[:, 4, :6] = np.nan                                               # two finite distances
    a[:, 5] = np.inf
    a[:, 7] = a[:, 6]                                                  # a tie: the lower image first
    flags = rng.random(N) < 0.5
    flags[3:8] = True
    for combine in ("min", "max"):
        for top_t in (None, 1, 2, 3, 7, 8):
            for fl in (None, flags):
                s, i = ref.topk(a, k, combine, top_t, fl, 11)
                rs, ri = tdr.topk_of_token_distances(a, k, combine, top_t, fl, 11)
                assert np.array_equal(i, ri) and np.array_equal(s.view(np.uint32), rs.view(np.uint32)), (combine, top_t)
            d = ref.combine_under_top_t(a, combine, top_t)
            assert np.array_equal(d.view(np.uint32), tdr.combine_distances(a, combine, top_t).view(np.uint32))
            if combine == "max" and top_t in (3, 7, 8):                # fewer than top_t finite distances: +inf, never returned
                assert np.isinf(d[:, 4]).all() and 4 + 11 not in ref.topk(a, N, combine, top_t, None, 11)[1]
            if combine == "min":                                       # 'min' under any top_t is the plain min
                assert np.array_equal(d.view(np.uint32), ref.combine_under_top_t(a, "min").view(np.uint32))
    assert np.array_equal(ref.combine_under_top_t(a, "max", P).view(np.uint32), ref.combine_under_top_t(a, "max").view(np.uint32))
    # fewer than k selected images: a (+inf, -1) tail
    few = np.zeros(N, bool)
    few[[6, 9, 20]] = True
    s, i = ref.topk(a, k, "max", 2, few)
    assert i[:, :3].tolist() == [[6, 9, 20]] * Q or (np.sort(i[:, :3], axis=1) == [6, 9, 20]).all()
    assert (i[:, 3:] == -1).all() and np.isinf(s[:, 3:]).all()


def test_live_tiles_and_the_select_routes_limits():
    flags = np.zeros(1024, bool)
    flags[16:48] = True                                                # tiles 1 and 2 of a P = 16 bank (16 images per tile)
    flags[1023] = True
    tiles, cum, last_live, whole = ref.live_tiles(flags, 16)
    assert tiles.tolist() == [1, 2, 63] and cum.tolist() == [16, 32, 33] and last_live and whole == 3
    assert not ref.select_route_takes(flags, 16, 8)                    # fewer than 8 live whole tiles
    flags[:] = False
    flags[::8] = True                                                  # 128 images: 2048 rows, every tile live
    assert ref.live_tiles(flags, 16)[3] == 64 and ref.select_route_takes(flags, 16, 128) and not ref.select_route_takes(flags, 16, 129)
    flags[8] = False
    assert not ref.select_route_takes(flags, 16, 8)                    # 127 x 16 < 2048 rows
    # a ragged bank: 523 images of 4 tokens are 8 whole tiles and 44 rows; the tail tile is live but not whole
    flags = np.ones(523, bool)
    tiles, cum, last_live, whole = ref.live_tiles(flags, 4)
    assert len(tiles) == 9 and last_live and whole == 8 and cum[-1] == 523
    assert ref.direct_end(cum, 1) == 2 and ref.direct_end(cum, 256) == 9 and ref.direct_end(list(range(1, 301)), 1) == 96


def test_the_predicate_states_its_limits():
    lib = _lib.lib()
    ok = lib.skyemb_token_mse_topt_prefilter_applicable
    for P in (1, 2, 4, 8, 16, 32, 64):
        for t in range(1, min(P, 16) + 1):
            assert ok(300, 4096 * 16 // P, P, 128, 10, MIN, t) == 1 and ok(300, 4096 * 16 // P, P, 128, 10, MAX, t) == 1, (P, t)
    for P, t in ((16, 0), (16, 17), (8, 9), (64, 17), (1, 2), (16, -1)):
        assert ok(300, 65536 // P, P, 128, 10, MAX, t) == 0
        assert b"top_t must be 1 .. min(P, 16)" in lib.skyemb_last_error(), (P, t)
    assert ok(300, 4096, 16, 128, 10, MEAN, 4) == 0 and b"combine mean is not served" in lib.skyemb_last_error()
    assert ok(300, 4096, 16, 128, 10, 7, 4) == 0 and b"combine code 7" in lib.skyemb_last_error()
    assert ok(300, 127, 16, 128, 10, MAX, 4) == 0 and b"N * P" in lib.skyemb_last_error()
    assert lib.skyemb_last_error().startswith(b"many-query weighted-MSE patch-token search")
    assert ops.token_mse_topt_prefilter_refusal(300, 4096, 16, 128, 10, MAX, 4) is None
    assert "top_t must be" in ops.token_mse_topt_prefilter_refusal(300, 4096, 16, 128, 10, MAX, 17)


def test_bad_arguments_are_refused_before_any_device_work():
    """Every refusal returns before the first launch: the pointers are never dereferenced (no GPU is needed to run this)."""
    lib = _lib.lib()
    one = ctypes.c_void_p(256)                                         # non-null, 16-byte aligned, never read
    odd = ctypes.c_void_p(260)

    def top(combine=MAX, top_t=4, P=16, c=one, t=one, N=4096, rowp=one):
        return lib.skyemb_distance_topk_tokens_prefiltered_top(c, t, 300, one, _lib.F16, rowp, one, N, P, 128, 10, combine, top_t, 0, None, one, 0,
                                                               one, one, one, None)

    def top_sel(combine=MAX, top_t=4, tiles=one, n_live=16, last_live=1, direct_end=1, N=4096, P=16):
        return lib.skyemb_distance_topk_tokens_prefiltered_top_sel(one, one, 300, one, _lib.F16, one, one, tiles, n_live, last_live, direct_end, N,
                                                                   P, 128, 10, combine, top_t, 0, None, one, 0, one, one, one, None)

    def sel(combine=MAX, n_live=16, direct_end=1):
        return lib.skyemb_distance_topk_tokens_prefiltered_sel(one, one, 300, one, _lib.F16, one, one, one, n_live, 1, direct_end, 4096, 16, 128,
                                                               10, combine, 0, None, one, 0, one, one, one, None)

    err = lib.skyemb_last_error
    assert top(combine=MEAN) != 0 and b"combines by min or max" in err() and err().startswith(b"skyemb_distance_topk_tokens_prefiltered_top:")
    assert top_sel(combine=MEAN) != 0 and err().startswith(b"skyemb_distance_topk_tokens_prefiltered_top_sel:") and b"min or max" in err()
    assert sel(combine=MEAN) != 0 and err().startswith(b"skyemb_distance_topk_tokens_prefiltered_sel:") and b"min or max" in err()
    assert top(top_t=17) != 0 and b"top_t must be 0 (all tokens) or 1 .. min(P, 16)" in err()
    assert err().startswith(b"skyemb_distance_topk_tokens_prefiltered_top:")
    assert top(top_t=-1) != 0 and top(top_t=9, P=8, N=8192) != 0 and b"top_t must be" in err()
    assert top_sel(top_t=17) != 0 and b"top_t must be" in err()
    assert top(top_t=17, combine=MIN) != 0 and b"top_t must be" in err()        # refused under 'min' too, where it would not be used
    assert top(c=None) != 0 and b"c and t must be given" in err()
    assert top(t=odd) != 0 and b"16-byte aligned" in err()
    assert top(N=127) != 0 and b"N * P" in err() and err().startswith(b"skyemb_distance_topk_tokens_prefiltered_top:")
    assert top(rowp=None) != 0 and b"null argument" in err()
    assert top_sel(tiles=None) != 0 and b"null argument" in err()
    # the select entry's own limits: n_live, at least one live whole tile, direct_end
    assert top_sel(n_live=0) != 0 and b"n_live = 0" in err() and err().startswith(b"skyemb_distance_topk_tokens_prefiltered_top_sel:")
    assert sel(n_live=257) != 0 and b"n_live = 257" in err() and err().startswith(b"skyemb_distance_topk_tokens_prefiltered_sel:")
    assert top_sel(n_live=1, last_live=1, N=523, P=4) != 0 and b"only live tile is the bank's tail tile" in err()
    assert top_sel(direct_end=0) != 0 and b"first slice ends at position 0" in err()
    assert sel(direct_end=17) != 0 and b"first slice ends at position 17" in err()
    # past the argument checks every variant stops at the workspace size (0 bytes were offered)
    for kw in (dict(top_t=0), dict(top_t=1), dict(top_t=4), dict(top_t=16), dict(combine=MIN, top_t=3)):
        assert top(**kw) != 0 and b"workspace too small" in err(), kw
        assert top_sel(**kw) != 0 and b"workspace too small" in err(), kw
    assert sel() != 0 and b"workspace too small" in err()
    # top_t = 0 IS the plain call: it reports under the plain call's name
    assert top(top_t=0) != 0 and err().startswith(b"skyemb_distance_topk_tokens_prefiltered:")
    assert top_sel(top_t=0) != 0 and err().startswith(b"skyemb_distance_topk_tokens_prefiltered_sel:")
    assert top(top_t=4) != 0 and err().startswith(b"skyemb_distance_topk_tokens_prefiltered_top:")


@pytest.mark.parametrize("bank", [_lib.PF_BANK_F16, _lib.PF_BANK_BF16])
@pytest.mark.parametrize("lo", [0, 1, _lib.PF_LO_UNSET])
def test_the_new_requests_plan_as_the_cosine_ones(bank, lo):
    """An MSE entry hands skyemb_prefilter_plan the request {PF_TOKENS, key-space combine, top_t, sel}: the plan is the cosine
    _top / _sel entry's of the same shape, field for field (eps_mse, the LDS for c and gamma are launch values outside the plan)."""
    code = {"min": MIN, "max": MAX}
    for (N, P, Q, k) in ((523, 4, 130, 8), (40, 64, 300, 1), (2092, 1, 130, 256), (1024, 16, 300, 8)):
        for combine in ("min", "max"):
            for top_t in (0, 1, 2, min(P, 16) - 1, min(P, 16)):
                if top_t < 0 or top_t > min(P, 16):
                    continue
                key, t = ref.key_space_request(combine, top_t, P)
                tiles, cum, last_live, whole = ref.live_tiles(np.arange(N) % 3 != 1, P)
                for sel in (None, dict(n_live=len(tiles), last_live=int(last_live), direct_sel=ref.direct_end(cum, k))):
                    kw = dict(P=P, thr0=True, lo=lo, **(sel or {}))
                    mse = ops.prefilter_plan(_lib.PF_TOKENS, bank, Q, N, 128, k, combine=code[key], top_t=t, eps=0.0, **kw)
                    # the cosine entry's own request: the key-space combine with the caller's top_t, which the planner folds itself
                    cos = ops.prefilter_plan(_lib.PF_TOKENS, bank, Q, N, 128, k, combine=code[key], top_t=top_t if key == "min" else 0, **kw)
                    assert bytes(mse) == bytes(cos), (N, P, combine, top_t, sel)
                    assert mse.top_t == t and bool(mse.cnt) == (t > 1) and bool(mse.sel) == (sel is not None)
                    assert ref.stage_folds(combine, top_t, P)[0] == ("count" if mse.cnt else "or" if (mse.tok_word >> 8) & 1 else "and")


def test_new_symbols_are_exported_and_the_version_stands():
    header = open(os.path.join(ROOT, "include", "skyemb.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.PROTOTYPES and hasattr(L, n), n
    assert L.skyemb_version() == 111 == _lib.ABI_VERSION
    for f in ("token_mse_topt_prefilter_refusal", "token_mse_topt_folds", "distance_topk_tokens_prefiltered_top",
              "distance_topk_tokens_prefiltered_sel", "distance_topk_tokens_prefiltered_top_sel"):
        assert callable(getattr(ops, f)), f
    assert hasattr(search.TokenBank, "prepare_mse_top_t") and hasattr(search.Selection, "prepare_mse")
    assert hasattr(search.Selection, "mse_prefilter")
    # the header states what the selection's preparation does to the MSE constants
    assert "{0, NaN, 0, 0}" in header and "fails the MSE row test under both folds" in header
