"""CPU: combine 'mean' under a selection of images on the two-stage route (the compacted pooled image of Selection.prepare_mean) --
the route decision, the two new library entries and every refusal of theirs before a launch, the plan they run under, and the
NumPy restatement of the gather the GPU test holds the kernel to."""
import ctypes
import os
import re
import weakref

import numpy as np
import pytest
import torch

from sky_embeddings_amd import _lib, ops, search
from tests import token_mean_select_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, MIN = ops.COMBINE_CODES["mean"], ops.COMBINE_CODES["min"]
GATHER, ENTRY = "skyemb_token_mean_select_gather", "skyemb_cosine_topk_tokens_mean_prefiltered_sel"


def _bank():
    tb = search.TokenBank.__new__(search.TokenBank)               # no device: the decision reads the flags only
    tb._resident, tb.dtype = True, torch.float16
    return tb


def _selection(count, held_for=None):
    sel = search.Selection.__new__(search.Selection)
    sel.count = count
    if held_for is not None:                                       # a faked entry: the decision asks only whether one is held
        sel._mean = weakref.WeakKeyDictionary({held_for: None})
    return sel


def _request(tb, **kw):
    base = dict(who="cosine_topk_tokens", Q=300, N=4400, P=16, D=128, k=10, combine=MEAN, metric=None, metric_name=None, top_t=0,
                per_query=False, step=16, idx_offset=0, tokens=None, bank=tb, weights=None, select=None)
    base.update(kw)
    return search.TokenRequest(**base)


def test_route_decision(monkeypatch):
    monkeypatch.setattr(search, "TOKEN_MEAN_SELECT_PREFILTER_MIN_Q", 17)
    monkeypatch.setattr(search, "TOKEN_MEAN_PREFILTER_MIN_Q", 100000)      # the unselected constant does not decide here
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 100000)
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    refusal = search._token_prefilter_refusal
    tb, other = _bank(), _bank()
    # a bare Selection, and one that holds the compacted image of ANOTHER bank: the grouped route, with the way in named
    for sel in (_selection(2085), _selection(2085, held_for=other)):
        why = refusal(_request(tb, select=sel))
        assert "select under combine 'mean'" in why and "Selection.prepare_mean" in why
    held = _selection(2085, held_for=tb)
    assert refusal(_request(tb, select=held)) is None
    assert refusal(_request(tb, select=held, Q=17, k=256, N=2085)) is None
    # each thing the route leaves out names itself
    assert "TOKEN_MEAN_SELECT_PREFILTER_MIN_Q = 17" in refusal(_request(tb, select=held, Q=16))
    why = refusal(_request(tb, select=_selection(2047, held_for=tb)))
    assert why.startswith("the selected images alone: ") and "N >= 2048" in why and "N=2047" in why
    why = refusal(_request(tb, select=_selection(9, held_for=tb), k=10))
    assert why.startswith("the selected images alone: ") and "k <= N" in why and "k=10" in why
    assert "the selected images alone" not in refusal(_request(tb, select=held, N=2047))      # the bank's own shape comes first
    assert refusal(_request(tb, select=held, top_t=4)) == "top_t under combine 'mean'"
    assert "per-query weights" in refusal(_request(tb, select=held, per_query=True))
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    assert "SKYEMB_TOPK_PREFILTER=0" in refusal(_request(tb, select=held))
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER")
    # the unselected mean search and the min / max searches under a selection decide as they did
    monkeypatch.setattr(search, "TOKEN_MEAN_PREFILTER_MIN_Q", 17)
    assert refusal(_request(tb)) is None
    assert "TOKEN_PREFILTER_MIN_Q" in refusal(_request(tb, combine=MIN, select=held))


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skyemb.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.build())
    for name in (GATHER, ENTRY):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/skyemb.h"
        assert hasattr(L, name), f"{name} is not exported"
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int32
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == len(args), name
        for p, a in zip(params, args):                             # pointer / 64-bit / 32-bit / float, position by position
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_float if p.startswith("float") \
                else ctypes.c_int32
            assert a is want, (name, p)


# fake, never followed pointers: every refusal below is a host check that returns before the first launch
A16, ODD = 0x10000, 0x10008


def _entry(L, **kw):
    a = dict(tw=A16, qn=A16, Q=300, bank16=A16, dtype=_lib.F16, xn=A16, tail=A16, rowp=A16, N=4400, S=2085, map=A16, P=16, D=128, k=10,
             combine=MEAN, eps=1e-6, off=0, thr0=None, ws=A16, ws_bytes=1 << 40, out_s=A16, out_i=A16, redo=A16, pooled=A16, stream=None)
    a.update(kw)
    rc = L.skyemb_cosine_topk_tokens_mean_prefiltered_sel(a["tw"], a["qn"], a["Q"], a["bank16"], a["dtype"], a["xn"], a["tail"], a["rowp"],
                                                          a["N"], a["S"], a["map"], a["P"], a["D"], a["k"], a["combine"], a["eps"], a["off"],
                                                          a["thr0"], a["ws"], a["ws_bytes"], a["out_s"], a["out_i"], a["redo"], a["pooled"],
                                                          a["stream"])
    return rc, L.skyemb_last_error().decode()


@pytest.mark.parametrize("kw,words", (
    (dict(combine=MIN), "combines by mean"),
    (dict(S=2047), "S >= 2048"),
    (dict(k=3000, S=2085), "k = 3000 exceeds the S = 2085"),
    (dict(S=4401), "S = 4401 selected images of a bank of N = 4400"),
    (dict(N=1 << 27, P=16), "2^31"),
    (dict(map=None), "null argument (map)"),
    (dict(pooled=ODD), "16-byte aligned"),
    (dict(tail=ODD), "16-byte aligned"),
    (dict(tail=None), "tail tile of skyemb_token_mean_select_gather is needed"),
    (dict(pooled=None), "null argument"),
    (dict(dtype=_lib.F32), "dtype"),
    (dict(P=48), "P a divisor of 64"),
    (dict(k=257), "k <= 256"),
    (dict(ws_bytes=1024), "workspace too small"),
))
def test_every_refusal_of_the_search_entry_comes_before_a_launch(kw, words):
    rc, text = _entry(_lib.lib(), **kw)
    assert rc != 0 and text.startswith(ENTRY + ":") and words in text, text


def test_a_whole_number_of_tiles_needs_no_tail():
    """S % 256 == 0: a null tail passes the host checks -- the call gets as far as the workspace check, the last one before a launch."""
    rc, text = _entry(_lib.lib(), S=2048, tail=None, ws_bytes=1024)
    assert rc != 0 and "workspace too small" in text


def _gather(L, **kw):
    a = dict(pooled=A16, rowp=A16, idx=A16, N=4400, S=2085, D=128, dtype=_lib.BF16, pooled_sel=A16, rowp_sel=A16, tail=A16, map=A16)
    a.update(kw)
    rc = L.skyemb_token_mean_select_gather(a["pooled"], a["rowp"], a["idx"], a["N"], a["S"], a["D"], a["dtype"], a["pooled_sel"], a["rowp_sel"],
                                           a["tail"], a["map"], None)
    return rc, L.skyemb_last_error().decode()


@pytest.mark.parametrize("kw,words", (
    (dict(dtype=_lib.F32), "dtype"),
    (dict(idx=None), "null argument"),
    (dict(map=None), "null argument"),
    (dict(S=0), "1 <= S <= N"),
    (dict(S=4401), "1 <= S <= N"),
    (dict(D=144), "D % 32 == 0"),
    (dict(tail=None), "a tail tile [256, D] is needed"),
    (dict(pooled_sel=ODD), "16-byte aligned"),
    (dict(tail=ODD), "16-byte aligned"),
))
def test_every_refusal_of_the_gather_comes_before_a_launch(kw, words):
    rc, text = _gather(_lib.lib(), **kw)
    assert rc != 0 and text.startswith(GATHER + ":") and words in text, text


def test_the_entry_plans_as_the_unselected_mean_request_over_s_rows():
    """Nothing was added to the planner: the entry's plan IS skyemb_prefilter_plan's answer to {MEAN, N = S, sel = 0}, and a mean request
    with selection fields is refused as it ever was."""
    for bank in (_lib.PF_BANK_F16, _lib.PF_BANK_BF16):
        for S, k in ((2085, 10), (2048, 256), (25030, 100)):
            p = ops.prefilter_plan(_lib.PF_TOKENS_MEAN, bank, 257, S, 128, k, P=16, combine=MEAN, thr0=True, lo=_lib.PF_LO_UNSET)
            assert (p.rows, p.T, p.T_tail, p.has_tail) == (S, S // 256, S // 256, int(S % 256 != 0))
            assert (p.sel, p.tok, p.cnt, p.fold, p.top_t, p.use_lo) == (0, 0, 0, 2, 0, 1)
            assert all(not p.slice[i].tail_sel for i in range(p.n_slices)) and p.slice[p.n_slices - 1].final == 1
            # the bank's own N is no input of the plan: the same bytes whatever bank the S images were selected from
            again = ops.prefilter_plan(_lib.PF_TOKENS_MEAN, bank, 257, S, 128, k, P=16, combine=MEAN, thr0=True, lo=_lib.PF_LO_UNSET)
            assert bytes(p) == bytes(again)
    with pytest.raises(_lib.SkyembError, match="no entry point takes this request"):
        ops.prefilter_plan(_lib.PF_TOKENS_MEAN, _lib.PF_BANK_F16, 257, 2085, 128, 10, P=16, combine=MEAN, n_live=9, direct_sel=1)
    # what the plan refuses, the entry refuses in the plan's words under its own name
    with pytest.raises(_lib.SkyembError) as e:
        ops.prefilter_plan(_lib.PF_TOKENS_MEAN, _lib.PF_BANK_F16, 300, 2085, 128, 10, P=48, combine=MEAN, thr0=False)
    plan_text = str(e.value).split("skyemb_cosine_topk_tokens_mean_prefiltered: ", 1)[1]
    rc, text = _entry(_lib.lib(), P=48)
    assert rc != 0 and text == ENTRY + ": " + plan_text
    assert ops.token_mean_select_prefilter_refusal(300, 2085, 16, 128, 10) is None
    assert "N >= 2048" in ops.token_mean_select_prefilter_refusal(300, 2047, 16, 128, 10)


def test_gather_reference():
    rng = np.random.default_rng(0)
    N, D = 700, 32
    bits = rng.integers(0, 1 << 16, (N, D), dtype=np.uint16)
    rowp = rng.standard_normal((ref.rowp_rows(N), 4)).astype(np.float32)
    rowp[N:] = ref.SENTINEL
    rowp[5] = (0, np.inf, 1, 0)
    for S in (1, 255, 256, 300, 512, 700):
        idx = np.sort(rng.choice(N, S, replace=False))
        if S == 300:
            idx[0] = 5                                             # (5 is below every other pick or among them: keep ascending)
            idx = np.unique(idx)
            S = idx.shape[0]
        ps, rs, tail, m = ref.gather(bits, rowp, idx)
        assert ps.shape == (S, D) and rs.shape == (ref.rowp_rows(S), 4) and m.dtype == np.int32 and (m == idx).all()
        assert (ps == bits[idx]).all() and ref.same_bits(rs[:S], rowp[idx])
        assert ref.same_bits(rs[S:], np.tile(ref.SENTINEL, (rs.shape[0] - S, 1)))
        if S % 256 == 0:
            assert tail is None
        else:
            assert tail.shape == (256, D) and (tail[:S % 256] == ps[S // 256 * 256:]).all() and (tail[S % 256:] == 0).all()
    with pytest.raises(AssertionError):
        ref.gather(bits, rowp, np.array([3, 2]))                   # not ascending
