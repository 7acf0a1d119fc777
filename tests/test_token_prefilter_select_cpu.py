"""CPU: the two-stage many-query patch-token search under a selection of images -- the numpy restatement of what the device
prepares and tests (tests/token_prefilter_select_reference.py) has the properties the design relies on and keeps the candidate
lists of the GPU cases inside their capacity; the route decision is one pure function; the new symbols are exported as declared and
refuse bad arguments before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from sky_embeddings_amd import _lib, ops, search
from tests import token_prefilter_reference as tpr
from tests import token_prefilter_select_reference as tps
from tests import token_search_reference as tsr
from tests import token_select_reference as tsel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("skyemb_token_prefilter_select_prepare", "skyemb_cosine_topk_tokens_prefiltered_sel")


def _rowp(R, rng):
    """Row constants of R rows padded to whole tiles, as skyemb_resident_rowp leaves them: {xn, nx, 1, 0}, the sentinel behind."""
    rows = (R + 255) // 256 * 256
    rowp = np.tile(tps.SENTINEL, (rows, 1))
    rowp[:R] = np.stack([rng.random(R) + 1, rng.random(R) + 2, np.ones(R), np.zeros(R)], axis=1)
    return rowp


@pytest.mark.parametrize("P", [1, 2, 4, 8, 16, 32, 64])
def test_prepare_by_hand_and_its_properties(P):
    rng = np.random.default_rng(P)
    N = (5 * 256 + 64) // P                                         # five whole tiles and a tail of 64 rows
    R = N * P
    rowp = _rowp(R, rng)
    rowp[3 * P] = [0, np.inf, 1, 0]                                 # an unboundable row in image 3 ...
    rowp[(N - 1) * P] = [0, np.inf, 1, 0]                           # ... and in the last image
    per_tile = 256 // P
    f = np.zeros(N, bool)
    f[[0, N - 1]] = True                                            # tile 0 and the tail tile; image 3 deselected
    f[2 * per_tile:3 * per_tile] = True                             # all of tile 2
    m, tiles, cum, last = tps.prepare(rowp, f, P)
    assert tiles.tolist() == [0, 2, 5] and last == 1 and cum.tolist() == [1, 1 + per_tile, 2 + per_tile]
    assert tiles.dtype == np.int32 and cum.dtype == np.int32 and cum[-1] == f.sum()
    on = tps.row_mask(f, P)
    assert np.array_equal(m[:R][on], rowp[:R][on]) and np.isinf(m[(N - 1) * P, 1])
    off = np.setdiff1d(np.arange(rowp.shape[0]), np.flatnonzero(on))
    assert np.isnan(m[off, 1]).all() and (m[off][:, [0, 2, 3]] == 0).all() and np.isnan(m[3 * P, 1])
    # all True: the unmasked constants, padding included (it held the sentinel already); all tiles live; counts end at N
    m, tiles, cum, last = tps.prepare(rowp, np.ones(N, bool), P)
    assert np.array_equal(m, rowp, equal_nan=True) and tiles.tolist() == list(range(6)) and last == 1 and cum[-1] == N
    assert (np.diff(cum) > 0).all()
    # all False: nothing live
    m, tiles, cum, last = tps.prepare(rowp, np.zeros(N, bool), P)
    assert tiles.size == 0 and cum.size == 0 and last == 0 and np.isnan(m[:, 1]).all()
    # random: monotone counts that end at the selected count; a tile without a selected image is not live; the popcount the
    # device takes of its packed words -- whole words down to 32 images per tile, an aligned bit field below -- agrees
    f = rng.random(N) < 0.3
    f[per_tile:2 * per_tile] = False
    m, tiles, cum, last = tps.prepare(rowp, f, P)
    assert 1 not in tiles and (np.diff(cum) > 0).all() and cum[-1] == f.sum()
    words = tsel.pack_words(f)
    pc = []
    for t in range(6):
        first = t * per_tile
        if per_tile >= 32:
            pc.append(sum(bin(int(w)).count("1") for w in words[first // 32:first // 32 + per_tile // 32]))
        else:
            pc.append(bin((int(words[first >> 5]) >> (first & 31)) & ((1 << per_tile) - 1)).count("1") if (first >> 5) < words.size else 0)
    assert [t for t in range(6) if pc[t]] == tiles.tolist() and np.cumsum(pc)[tiles].tolist() == cum.tolist()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("combine", ["min", "max"])
def test_a_deselected_unboundable_row_never_passes(dtype, combine):
    """Without the mask an unboundable row makes its image a candidate of every query under 'max'; under the mask a deselected
    image passes for no query at any threshold, under either combine, and selected images are decided as without a selection."""
    rng = np.random.default_rng(3)
    N, P, D = 64, 4, 128
    q = rng.standard_normal((5, D), dtype=np.float32)
    x = rng.standard_normal((N, P, D), dtype=np.float32)
    x[3, 1, 5] = np.nan
    x[7, 0, 9] = np.inf
    x[8] = np.nan
    _, xw = tpr.to16(x, dtype)
    eps_a = ops.topk_prefilter_eps_a_resident(D, dtype, lo=False)
    lhs, coef, ub = tpr.row_margins(q, xw.reshape(N * P, D), None, dtype, False, tpr.flush_models(dtype)[-1], eps_a)
    f = np.ones(N, bool)
    f[[3, 8, 20]] = False
    for tau in (np.full(5, 1e30), np.full(5, -1e30), np.zeros(5)):
        plain = tpr.image_pass(lhs, coef, ub, tau, P, combine)
        ok = tps.image_pass(lhs, coef, ub, tau, P, combine, f)
        assert not ok[:, ~f].any()
        assert np.array_equal(ok[:, f], plain[:, f])
    if combine == "max":
        assert tpr.image_pass(lhs, coef, ub, np.full(5, 1e30), P, combine)[:, 3].all()      # what the mask prevents
        assert tps.image_pass(lhs, coef, ub, np.full(5, 1e30), P, combine, f)[:, 7].all()   # selected: still kept for every query


def test_first_slice_rule():
    cum = [10, 20, 30, 40, 50]
    assert tps.direct_end(cum, 5, 1) == 5                            # 96 is never reached: the whole list
    assert tps.direct_end([50, 100, 150], 3, 1) == 2                 # position 1 is the first to hold 96
    assert tps.direct_end([96, 100], 2, 1) == 1
    assert tps.direct_end([1000] * 1 + list(range(1001, 1300)), 300, 1) == 2      # never less than n_live / 128
    assert tps.slices(np.arange(17), np.arange(1, 18) * 64, 1, 4096 + 16, 7) == [(0, 11, "direct"), (11, 17, "staged")]
    assert tps.slices(np.array([3, 16]), np.array([64, 65]), 1, 4096 + 16, 7) == [(0, 2, "direct")]


def _selection(count):
    sel = search.Selection.__new__(search.Selection)               # no device: the decision reads the count only
    sel.count = count
    return sel


def _request(**kw):
    tb = search.TokenBank.__new__(search.TokenBank)
    tb._resident = True
    base = dict(who="cosine_topk_tokens", Q=64, N=4096, P=16, D=128, k=10, combine=ops.COMBINE_CODES["min"], metric=None,
                metric_name=None, top_t=0, per_query=False, step=16, idx_offset=0, tokens=None, bank=tb, weights=None, select=None)
    base.update(kw)
    return search.TokenRequest(**base)


def test_route_decision_under_a_selection(monkeypatch):
    """A Selection whose images are themselves a bank the route takes goes two-stage; anything else keeps the grouped route."""
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 17)
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    refusal = search._token_prefilter_refusal
    assert refusal(_request(select=_selection(4096))) is None
    assert refusal(_request(select=_selection(128))) is None        # 128 x 16 = 2048 rows
    assert refusal(_request(select=_selection(10), k=10, P=64, N=4096)) is not None
    for P in (1, 2, 4, 8, 16, 32, 64):
        assert refusal(_request(P=P, N=8192 // P, k=1, select=_selection(2048 // P))) is None
        why = refusal(_request(P=P, N=8192 // P, k=1, select=_selection(2048 // P - 1)))
        assert isinstance(why, str) and "selected images" in why and "N * P" in why
    why = refusal(_request(k=200, select=_selection(199)))          # fewer selected images than k
    assert isinstance(why, str) and "selected images" in why
    assert isinstance(refusal(_request(select=_selection(0))), str)
    for other in (object(), torch.ones(4096, dtype=torch.bool), "all"):
        why = refusal(_request(select=other))
        assert isinstance(why, str) and "Selection" in why
    # every condition that refuses without a selection refuses with one
    plain = search.TokenBank.__new__(search.TokenBank)
    plain._resident = False
    grouped = dict(bank=[plain, None], combine=[ops.COMBINE_CODES["mean"]], top_t=[1, 4], per_query=[True], P=[3, 48, 128], Q=[16, 1],
                   metric=[ops.METRIC_CODES["MSE"]], D=[96, 144, 4128], k=[257], N=[127])
    for field, values in grouped.items():
        for v in values:
            why = refusal(_request(select=_selection(4096), **{field: v}))
            assert isinstance(why, str) and why and "selected images" not in why, (field, v)
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    assert "SKYEMB_TOPK_PREFILTER" in refusal(_request(select=_selection(4096)))
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER")
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 65)
    assert "TOKEN_PREFILTER_MIN_Q" in refusal(_request(select=_selection(4096)))


def test_new_symbols_are_exported_with_the_declared_signatures():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skyemb.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.build())
    for name in NEW:
        m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/skyemb.h"
        assert hasattr(L, name), f"{name} is not exported"
        res, args = _lib.PROTOTYPES[name]
        assert res is (ctypes.c_int64 if m.group(1) == "int64_t" else ctypes.c_int32)
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args), (name, len(params), len(args))
        for p, a in zip(params, args):
            want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float") else
                    ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int32)
            assert a is want, (name, p, a)
    assert callable(ops.token_prefilter_select_prepare) and callable(ops.cosine_topk_tokens_prefiltered_sel)
    assert callable(search.Selection.token_prefilter)


def test_bad_arguments_are_refused_before_any_device_work():
    """Every refusal below returns before the first launch: the pointers are never dereferenced (no GPU is needed to run this)."""
    lib = _lib.lib()
    a, odd = 4096, 4104                                             # a 16-byte aligned address and one that is not

    def search_rc(**kw):
        v = dict(tw=a, qn=a, Q=17, bank=a, dtype=_lib.F16, xn=a, tail=a, rowp=a, tiles=a, n_live=4, last_live=0, direct_end=1, N=1024, P=4,
                 D=128, k=5, combine=_lib.COMBINE_MIN, thr0=None, ws=a, ws_bytes=1 << 40)
        v.update(kw)
        return lib.skyemb_cosine_topk_tokens_prefiltered_sel(v["tw"], v["qn"], v["Q"], v["bank"], v["dtype"], v["xn"], v["tail"], v["rowp"],
                                                             v["tiles"], v["n_live"], v["last_live"], v["direct_end"], v["N"], v["P"],
                                                             v["D"], v["k"], v["combine"], 1e-6, 0, v["thr0"], v["ws"], v["ws_bytes"], a, a,
                                                             a, None)

    def err():
        return lib.skyemb_last_error().decode()

    for name in ("tw", "qn", "bank", "xn", "rowp", "tiles", "ws"):
        assert search_rc(**{name: None}) != 0 and "null argument" in err(), name
    assert search_rc(dtype=_lib.F32) != 0 and "SKYEMB_BF16" in err()
    assert search_rc(combine=_lib.COMBINE_MEAN) != 0 and "min or max" in err()
    assert search_rc(P=3) != 0 and "divisor of 64" in err()
    assert search_rc(N=511) != 0 and "N * P" in err()
    assert search_rc(N=1025, tail=None) != 0 and "tail tile" in err()
    assert search_rc(bank=odd) != 0 and "16-byte aligned" in err()
    assert search_rc(tail=odd) != 0 and "16-byte aligned" in err()
    for n_live in (0, -1, 17):                                       # 1024 x 4 rows: 16 tiles
        assert search_rc(n_live=n_live) != 0 and "n_live" in err(), n_live
    assert search_rc(last_live=2) != 0 and "n_live" in err()
    assert search_rc(N=1025, n_live=1, last_live=1) != 0 and "whole live tile" in err()
    for d in (0, 5, -3):
        assert search_rc(direct_end=d) != 0 and "first slice" in err(), d
    assert search_rc(ws_bytes=16) != 0 and "workspace too small" in err()

    def prepare_rc(words=a, N=1024, P=4, rowp=a, rowp_sel=a, tiles=a, cum=a, info=a):
        return lib.skyemb_token_prefilter_select_prepare(words, N, P, rowp, rowp_sel, tiles, cum, info, None)

    for name in ("words", "rowp", "rowp_sel", "tiles", "cum", "info"):
        assert prepare_rc(**{name: None}) != 0 and "null argument" in err(), name
    for kw in (dict(P=3), dict(P=128), dict(P=0), dict(N=0), dict(N=2 ** 29, P=4)):
        assert prepare_rc(**kw) != 0 and "divisor of 64" in err(), kw


@pytest.mark.parametrize("c", tps.CASES, ids=tps.case_id)
def test_the_lists_of_the_gpu_cases_hold(c):
    """For every GPU case, under every flush model: every image of the compacted oracle's top-k passes the masked image test at
    the query's exact k-th best, and with tau as the design maintains it no candidate list (4096 / 8192) and no 2048-slot staging
    region fills -- the condition behind the GPU test's cap on ``redone``."""
    P, combine, dt, lo, Q, tail, k, weighted, off, kind = c
    dtype = tpr.DTYPES[dt]
    q, bank, xw, w = tps.case_inputs(P, tail, Q, weighted, dt)
    f = tps.case_flags(c)
    N = xw.shape[0]
    assert N <= 4096 + 255 and f.sum() * P >= 2048 and k <= f.sum()
    exact = tsr.combined_scores(q, xw, combine, w)
    ref_s, ref_i = tps.compacted_topk(q, xw, k, combine, f, w, 0)
    tau = ref_s[:, k - 1].astype(np.float64)
    eps_a = ops.topk_prefilter_eps_a_resident(tps.D, dtype, lo=lo)
    worst = None
    for flush in tpr.flush_models(dtype):
        lhs, coef, ub = tpr.row_margins(q, xw.reshape(N * P, tps.D), w, dtype, lo, flush, eps_a)
        ok = tps.image_pass(lhs, coef, ub, tau, P, combine, f)
        assert not ok[:, ~f].any()
        for qi in range(Q):
            top = ref_i[qi][ref_i[qi] >= 0]
            assert ok[qi, top].all(), (flush, qi, top[~ok[qi, top]][:5])
        counts, flagged = tps.simulate(exact, lhs, coef, ub, P, k, combine, lo, f)
        assert not flagged.any(), (flush, int(flagged.sum()), counts.max(axis=1))
        worst = counts.max(axis=1) if worst is None else np.maximum(worst, counts.max(axis=1))
    print(tps.case_id(c), "largest candidate count per slice:", worst.tolist(), "of", tpr.list_cap(k))
