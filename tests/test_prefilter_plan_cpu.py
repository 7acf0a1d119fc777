"""CPU: the host layer of the two-stage searches (csrc/prefilter_plan.h through skyemb_prefilter_plan: no device needed).  The Python
restatements of the schedule -- prefilter_stage1_reference.schedule, token_prefilter_stage_reference.token_schedule,
token_prefilter_reference.slices, token_prefilter_select_reference.slices / direct_end -- are held against the library's own planner
field by field over a sweep; every request the entry points refuse is refused by the planner with the same text; and the launches
traced on a GPU before the planner existed (tests/golden/prefilter_launches.json) are rebuilt from the plan."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

from sky_embeddings_amd import _lib, ops
from tests import prefilter_plan_cases as pc
from tests import prefilter_stage1_reference as sr
from tests import token_prefilter_reference as tpr
from tests import token_prefilter_select_reference as tps
from tests import token_prefilter_stage_reference as tsr

ROWS, TOKENS, MEAN = _lib.PF_ROWS, _lib.PF_TOKENS, _lib.PF_TOKENS_MEAN
F32, F16, BF16 = _lib.PF_BANK_F32, _lib.PF_BANK_F16, _lib.PF_BANK_BF16
UNSET = _lib.PF_LO_UNSET
MIN, MEANC, MAX = _lib.COMBINE_MIN, _lib.COMBINE_MEAN, _lib.COMBINE_MAX
FMT = {F32: "fp32", F16: "fp16", BF16: "bf16"}
BT = 256


def slices_of(p):
    return [p.slice[i] for i in range(p.n_slices)]


def row_launches(p):
    """A row plan in the words of prefilter_stage1_reference.schedule."""
    out = []
    for s in slices_of(p):
        out.append((f"mode{s.mode}", s.t0, s.t1))
        assert s.bucket == (s.mode == 2)
        if s.tail:
            assert not s.tail_sel                                  # rows: bank tile N / BT itself, even under a selection
            out.append(("tail", s.tail_pos))
        out.append(("select", s.final))
    return out


# N: T == first (2048, with k <= 128), first + 1, ragged, k = 129's first = 16 and first + 1, T >= 320 (six distinct ends)
ROW_N = (2048, 2048 + 44, 2304, 2304 + 100, 2560, 4096, 4096 + 255, 4352, 8192 + 1, 320 * BT, 333 * BT + 7, 1000 * BT)


def test_the_row_schedule_restatement_equals_the_planner():
    points = 0
    for N, k, thr0, bank, lo in itertools.product(ROW_N, (1, 5, 128, 129, 192), (False, True), (F32, F16, BF16), (0, 1, UNSET)):
        p = ops.prefilter_plan(ROWS, bank, 300, N, 128, k, thr0=thr0, lo=lo)
        ref = sr.schedule(N, k, thr0, bank != F32)
        for f in ("first", "direct_end", "has_tail", "T", "first_rows", "cap"):
            assert getattr(p, f) == ref[f], (N, k, thr0, bank, f)
        assert list(p.ends) == ref["ends"] and row_launches(p) == ref["launches"], (N, k, thr0, bank)
        assert (p.sel, p.bf, p.tok, p.cnt, p.tok_word, p.top_t) == (0, int(bank == BF16), 0, 0, 0, 0) and p.rows == N
        points += 1
    # the points the schedule's odd corners live at
    empty = ops.prefilter_plan(ROWS, F32, 17, 2048, 128, 5, lo=0)
    assert row_launches(empty) == [("mode0", 0, 8), ("select", 1), ("mode1", 8, 8), ("select", 1)]          # the empty direct launch
    six = ops.prefilter_plan(ROWS, F16, 17, 320 * BT + 7, 128, 5, lo=0)
    assert len(set(six.ends)) == 6 and six.n_slices == 6 and [s.mode for s in slices_of(six)] == [0, 1, 2, 2, 2, 2]
    assert [s.tail for s in slices_of(six)] == [0, 0, 0, 0, 0, 1] and six.slice[5].tail_pos == 320
    floor = ops.prefilter_plan(ROWS, F16, 17, 320 * BT, 128, 5, thr0=True, lo=0)
    assert [(s.mode, s.t0) for s in slices_of(floor)][0] == (2, 0) and floor.n_slices == 5                 # the take-all slice is skipped
    assert ops.prefilter_plan(ROWS, F16, 17, 8192, 128, 129, lo=0).first == 16
    assert points == len(ROW_N) * 5 * 2 * 3 * 3


def test_the_row_schedule_under_a_selection_equals_the_planner():
    for N, bank, k in itertools.product((2560, 2560 + 37, 4096 + 1, 40 * BT + 3), (F32, F16, BF16), (5, 129)):
        tiles_all = -(-N // BT)
        for n_live, last_live in itertools.product(range(1, tiles_all + 1), (0, 1)):
            ragged = bank != F32 and N % BT != 0
            if n_live == 1 and last_live and ragged:
                with pytest.raises(_lib.SkyembError, match="only live tile is the resident bank's tail tile"):
                    ops.prefilter_plan(ROWS, bank, 300, N, 128, k, n_live=1, last_live=1, lo=0)
                continue
            p = ops.prefilter_plan(ROWS, bank, 300, N, 128, k, n_live=n_live, last_live=last_live, lo=0)
            ref = sr.schedule(N, k, False, bank != F32, n_live=n_live, last_live=last_live)
            for f in ("first", "direct_end", "has_tail", "T", "first_rows", "cap"):
                assert getattr(p, f) == ref[f], (N, bank, n_live, last_live, f)
            assert list(p.ends) == ref["ends"] and row_launches(p) == ref["launches"] and p.sel == 1


TOKEN_SHAPES = [(P, N) for P in tsr.PS for N in (2048 // P, 2048 // P + 1, 4096 // P + 3, 20480 // P, 320 * BT // P + 1, 1000 * BT // P)]


def test_the_token_schedule_restatements_equal_the_planner():
    assert {1, 4, 64} <= {P for P, _ in TOKEN_SHAPES}
    for (P, N), k, bank, combine, thr0 in itertools.product(TOKEN_SHAPES, (1, 5, 200), (F16, BF16), (MIN, MAX), (False, True)):
        if k > N:
            continue
        p = ops.prefilter_plan(TOKENS, bank, 24, N, 128, k, P=P, combine=combine, thr0=thr0, lo=UNSET)
        ref = tsr.token_schedule(N, P, k)
        assert (p.T, p.direct_end, list(p.ends)[1:], bool(p.has_tail)) == (ref["T"], ref["direct_end"], ref["ends"], ref["tail_live"])
        assert p.first == 0 and p.first_rows == 0 and p.ends[0] == 0 and p.rows == N * P and p.T_tail == N * P // BT
        got = [(s.t0, s.t1, "direct" if s.mode == 1 else "staged", bool(s.tail)) for s in slices_of(p)]
        assert got == ref["slices"], (P, N, k)
        assert all(s.bucket == (s.mode == 2) and s.final == (s.t1 == p.T) and (not s.tail or (s.tail_pos, s.tail_sel) == (p.T_tail, 0))
                   for s in slices_of(p))
        R = N * P
        assert [(s.t0 * BT, R if s.t1 == p.T else s.t1 * BT, "direct" if s.mode == 1 else "staged") for s in slices_of(p)] == tpr.slices(R, P, k)
        assert (p.tok, p.cnt, p.lgp, p.fold, p.top_t) == (1, 0, P.bit_length() - 1, int(combine == MAX), 0)
        assert p.tok_word == p.lgp | (int(combine == MAX) << 8)


def test_top_t_is_normalised_and_travels_in_the_tok_word():
    for P, top_t, combine in itertools.product((4, 16, 64), (0, 1, 2, 4, 16), (MIN, MAX)):
        if top_t > min(P, 16):
            continue
        p = ops.prefilter_plan(TOKENS, F16, 24, 4096 * 4 // P, 128, 5, P=P, combine=combine, top_t=top_t, lo=UNSET)
        plain = combine == MAX or top_t in (0, P)
        assert p.top_t == (0 if plain else top_t) and p.cnt == int(not plain and top_t > 1)
        stage1, stage2 = ops.token_topt_folds(P, combine, top_t)
        assert {"and": 0, "or": 1, "count": 0}[stage1] == (p.tok_word >> 8) & 1 and (stage1 == "count") == bool(p.cnt)
        assert p.tok_word >> 16 == (top_t if p.cnt else 0) and (stage2 == "top") == (p.top_t != 0)


def test_the_mean_schedule_walks_images():
    for (P, N), k, bank, lo in itertools.product([(1, 2048), (4, 2048 + 9), (64, 2560), (4, 320 * BT + 1)], (5, 200), (F16, BF16), (0, 1, UNSET)):
        p = ops.prefilter_plan(MEAN, bank, 24, N, 128, k, P=P, combine=MEANC, lo=lo, eps=1e-6)
        ref = tsr.token_schedule(N, 1, k)                           # stage 1's rows are images: the token schedule at P = 1
        assert (p.T, p.direct_end, list(p.ends)[1:], bool(p.has_tail)) == (ref["T"], ref["direct_end"], ref["ends"], ref["tail_live"])
        assert [(s.t0, s.t1, "direct" if s.mode == 1 else "staged", bool(s.tail)) for s in slices_of(p)] == ref["slices"]
        assert (p.tok, p.cnt, p.fold, p.rows, p.lgp) == (0, 0, 2, N, P.bit_length() - 1)
        assert p.use_lo == int(lo != 0)                             # the mean rule: hi + lo unless SKYEMB_PREFILTER_LO=0
        dt = {F16: "float16", BF16: "bfloat16"}[bank]
        import torch
        assert p.eps_a == ops.token_mean_prefilter_eps_m(128, getattr(torch, dt), lo=bool(p.use_lo))
        assert p.gfac == np.float32(float(np.float32(1e-6)) / (p.eps_a * (1.0 + 1e-6)) * (1.0 + 1e-6))
    assert np.isnan(ops.prefilter_plan(MEAN, F16, 24, 2048, 128, 5, P=4, combine=MEANC, eps=-1.0).gfac)
    assert ops.prefilter_plan(TOKENS, F16, 24, 2048, 128, 5, P=4).gfac == -1.0


def selection_lists(N, P, dead):
    """(tiles, cum, last_live) of a selection of images that leaves the `dead` tiles without a selected image."""
    R, ipt = N * P, BT // P
    tiles_all = -(-R // BT)
    tiles = [t for t in range(tiles_all) if t not in dead]
    cum = np.cumsum([min((t + 1) * ipt, N) - t * ipt for t in tiles]).tolist()
    return tiles, cum, int(tiles_all - 1 in tiles)


def test_the_selected_token_schedule_restatements_equal_the_planner():
    for P, N, dead, k in itertools.product((1, 4, 64), (4096, 4096 + 3, 40 * BT + 1), ((), (2,), (0, 5, 6)), (1, 5, 40)):
        if P == 64 and N > 4100:
            N = N // 16
        R = N * P
        dead = dead + ((-(-R // BT) - 1,) if k == 40 else ())       # the last tile dead as well
        tiles, cum, last_live = selection_lists(N, P, dead)
        n_live = len(tiles)
        rule = tps.direct_end(cum, n_live, k)
        for direct_sel in sorted({1, rule, max(1, n_live // 2), n_live}):
            p = ops.prefilter_plan(TOKENS, F16, 24, N, 128, min(k, N), P=P, combine=MIN, n_live=n_live, last_live=last_live, direct_sel=direct_sel)
            ref = tsr.token_schedule(N, P, k, n_live=n_live, direct_sel=direct_sel, last_live=last_live)
            assert (p.T, p.direct_end, list(p.ends)[1:], bool(p.has_tail)) == (ref["T"], ref["direct_end"], ref["ends"], ref["tail_live"])
            got = [(s.t0, s.t1, "direct" if s.mode == 1 else "staged", bool(s.tail)) for s in slices_of(p)]
            assert got == ref["slices"] and p.sel == 1
            # the tail under a selection: the SEL instance at the list's own last position
            assert all((s.tail_sel, s.tail_pos) == (1, p.T) for s in slices_of(p) if s.tail)
            if direct_sel == rule:
                assert [(s.t0, n_live if s.t1 == p.T else s.t1, "direct" if s.mode == 1 else "staged") for s in slices_of(p)] == \
                    tps.slices(tiles, cum, last_live, R, k)


def test_constants_variants_and_lds_bytes():
    import torch
    for D, k, Q in itertools.product((128, 768, 4096), (5, 129), (17, 300)):
        for bank, lo in itertools.product((F32, F16, BF16), (0, 1, UNSET)):
            p = ops.prefilter_plan(ROWS, bank, Q, 4096, D, k, lo=lo)
            # the three lo rules: fp16 operands run hi + lo only on =1; bf16 obeys =0 and =1 and falls back to its default (hi only)
            assert p.use_lo == int(lo == 1)
            want = ops.topk_prefilter_eps_a(D, lo=bool(p.use_lo)) if bank == F32 else \
                ops.topk_prefilter_eps_a_resident(D, torch.float16 if bank == F16 else torch.bfloat16, lo=bool(p.use_lo))
            assert p.eps_a == want == sr.eps_a(FMT[bank], D, bool(p.use_lo))
            assert p.eps_a_f32 == sr.eps_a_f32(FMT[bank], D, bool(p.use_lo))
            assert p.cap == sr.cap_of(k) == ops.topk_prefilter_ws_layout(Q, D, k)["cap"] and p.q_padded == -(-Q // 256) * 256
            assert p.lds_stage1 == 4 * 32768 + (sr.qtile(bool(p.use_lo)) + 256) * 16 + sr.SCAP * 8 + 16 <= p.lds_stage1_limit == 155664
            assert (p.lds_close, p.lds_close_limit, p.lds_rescore) == (2 * p.cap * 4 + 272 * 4, 2 * 8192 * 4 + 272 * 4, D * 4 + 256 * 8)
            t = ops.prefilter_plan(TOKENS, max(bank, F16), Q, 4096, D, k, P=4, lo=lo)
            assert t.use_lo == int(lo == 1) and t.lds_rescore == 0 and t.lds_stage1 == p.lds_stage1
            assert (t.lds_close, t.lds_close_limit) == ((256 + t.cap + 256) * 8 + D * 4 + 264 * 4, (512 + 8192) * 8 + 4096 * 4 + 264 * 4)
            assert t.eps_a == ops.topk_prefilter_eps_a_resident(D, torch.bfloat16 if bank == BF16 else torch.float16, lo=bool(t.use_lo))


def test_the_planners_eps_is_the_librarys_at_every_feature_count():
    """csrc/prefilter_plan.h restates the bounds that csrc/topk_prefilter.hip keeps for its eps exports and preparation calls: bit-equal
    doubles at every D the routes take, both variants, every bank kind, mean included."""
    import torch
    L = _lib.lib()
    for D in range(128, 4096 + 1, 32):
        for lo in (0, 1):
            assert ops.prefilter_plan(ROWS, F32, 17, 4096, D, 5, lo=lo).eps_a == L.skyemb_topk_prefilter_eps_a(D, lo, 0)
            for bank, dt in ((F16, torch.float16), (BF16, torch.bfloat16)):
                assert ops.prefilter_plan(ROWS, bank, 17, 4096, D, 5, lo=lo).eps_a == ops.topk_prefilter_eps_a_resident(D, dt, lo=bool(lo))
                assert ops.prefilter_plan(TOKENS, bank, 17, 1024, D, 5, P=4, lo=lo).eps_a == ops.topk_prefilter_eps_a_resident(D, dt, lo=bool(lo))
                assert ops.prefilter_plan(MEAN, bank, 17, 2048, D, 5, P=4, combine=MEANC, lo=lo).eps_a == \
                    ops.token_mean_prefilter_eps_m(D, dt, lo=bool(lo))


def test_lo_minus_one_reads_the_environment(monkeypatch):
    for env, want in ((None, UNSET), ("0", 0), ("1", 1), ("", UNSET), ("yes", UNSET)):
        if env is None:
            monkeypatch.delenv("SKYEMB_PREFILTER_LO", raising=False)
        else:
            monkeypatch.setenv("SKYEMB_PREFILTER_LO", env)
        for kind, bank, kw in ((ROWS, F16, {}), (ROWS, BF16, {}), (MEAN, BF16, dict(P=4, combine=MEANC))):
            assert ops.prefilter_plan(kind, bank, 24 if kind else 17, 4096, 128, 5, **kw).use_lo == \
                ops.prefilter_plan(kind, bank, 24 if kind else 17, 4096, 128, 5, lo=want, **kw).use_lo


# ---------------------------------------------------------------------------------------------------------------------- refusals
A = 4096                                   # a non-null, 16-byte aligned address that is never read


def entry_refusal(L, kind, bank, Q, N, D, k, P=1, combine=MIN, top_t=0, n_live=None, last_live=0, direct_sel=0):
    """(rc, text) of the entry point serving the request, called with pointers that are never read (refused before any launch)."""
    dtype = {F32: _lib.F32, F16: _lib.F16, BF16: _lib.BF16}.get(bank, bank)
    big = 1 << 40
    if kind == ROWS and bank == F32:
        rc = (L.skyemb_cosine_topk_prefiltered(A, A, Q, A, A, A, A, N, D, k, 1e-6, 0, None, A, big, A, A, A, None) if n_live is None else
              L.skyemb_cosine_topk_prefiltered_sel(A, A, Q, A, A, A, A, A, n_live, last_live, N, D, k, 1e-6, 0, A, big, A, A, A, None))
    elif kind == ROWS:
        rc = (L.skyemb_cosine_topk_prefiltered_resident(A, A, Q, A, dtype, A, A, A, N, D, k, 1e-6, 0, None, A, big, A, A, A, None)
              if n_live is None else
              L.skyemb_cosine_topk_prefiltered_resident_sel(A, A, Q, A, dtype, A, A, A, A, n_live, last_live, N, D, k, 1e-6, 0, A, big, A, A, A, None))
    elif kind == MEAN:
        rc = L.skyemb_cosine_topk_tokens_mean_prefiltered(A, A, Q, A, dtype, A, A, A, N, P, D, k, combine, 1e-6, 0, None, A, big, A, A, A, A, None)
    elif n_live is None:
        rc = L.skyemb_cosine_topk_tokens_prefiltered_top(A, A, Q, A, dtype, A, A, A, N, P, D, k, combine, top_t, 1e-6, 0, None, A, big, A, A, A, None)
    else:
        rc = L.skyemb_cosine_topk_tokens_prefiltered_top_sel(A, A, Q, A, dtype, A, A, A, A, n_live, last_live, direct_sel, N, P, D, k, combine, top_t,
                                                             1e-6, 0, None, A, big, A, A, A, None)
    return rc, L.skyemb_last_error().decode()


def plan_refusal(L, kind, bank, Q, N, D, k, P=1, combine=MIN, top_t=0, n_live=None, last_live=0, direct_sel=0):
    r = _lib.PrefilterRequest(kind, bank, Q, P, D, k, N, combine, top_t, 0, int(n_live is not None), n_live or 0, last_live, direct_sel, -1, 1e-6)
    rc = L.skyemb_prefilter_plan(r, _lib.PrefilterPlan())
    return rc, L.skyemb_last_error().decode()


REFUSED = [
    # rows: every limit of skyemb_topk_prefilter_applicable, then the counters' range and the selection's info
    *[dict(kind=ROWS, bank=b, Q=Q, N=N, D=D, k=k) for b in (F32, F16, BF16)
      for Q, N, D, k in ((16, 4096, 128, 5), (17, 2047, 128, 5), (17, 4096, 96, 5), (17, 4096, 144, 5), (17, 4096, 4128, 5), (17, 4096, 128, 0),
                         (17, 4096, 128, 193), (17, 2 ** 31, 128, 5), (600000, 2 ** 31 - 1, 4096, 5))],
    *[dict(kind=ROWS, bank=b, Q=17, N=2560 + 37, D=128, k=5, n_live=n, last_live=l) for b in (F32, F16, BF16)
      for n, l in ((0, 0), (-1, 0), (12, 0), (3, 2), (3, -1))],
    dict(kind=ROWS, bank=F16, Q=17, N=2560 + 37, D=128, k=5, n_live=1, last_live=1),
    dict(kind=ROWS, bank=BF16, Q=17, N=2560 + 37, D=128, k=5, n_live=1, last_live=1),
    # tokens: the cases of test_token_prefilter_select_cpu.py and of the *_applicable tests
    *[dict(kind=TOKENS, bank=F16, Q=17, N=N, P=P, D=D, k=k, combine=c, top_t=t)
      for N, P, D, k, c, t in ((1024, 3, 128, 5, MIN, 0), (511, 4, 128, 5, MIN, 0), (1024, 128, 128, 5, MIN, 0), (1024, 4, 100, 5, MAX, 0),
                               (1024, 4, 128, 257, MIN, 0), (4, 64, 128, 5, MIN, 0), (2 ** 29, 4, 128, 5, MIN, 0), (1024, 4, 128, 5, MEANC, 0),
                               (1024, 4, 128, 5, MEANC, 2), (1024, 4, 128, 5, 7, 0), (1024, 4, 128, 5, 7, 2), (1024, 4, 128, 5, MIN, 5),
                               (1024, 4, 128, 5, MIN, -1), (1024, 64, 128, 5, MIN, 17), (1024, 8, 128, 5, MAX, 9))],
    dict(kind=TOKENS, bank=BF16, Q=600000, N=2 ** 25, P=32, D=4096, k=5, combine=MIN),
    *[dict(kind=TOKENS, bank=F16, Q=17, N=1024, P=4, D=128, k=5, combine=MIN, top_t=t, n_live=n, last_live=l, direct_sel=d)
      for t in (0, 2) for n, l, d in ((0, 0, 1), (-1, 0, 1), (17, 0, 1), (4, 2, 1), (4, 0, 0), (4, 0, 5), (4, 0, -3))],
    dict(kind=TOKENS, bank=F16, Q=17, N=1025, P=4, D=128, k=5, combine=MIN, n_live=1, last_live=1, direct_sel=1),
    # mean
    *[dict(kind=MEAN, bank=b, Q=17, N=N, P=P, D=D, k=k, combine=c) for b in (F16, BF16)
      for N, P, D, k, c in ((2047, 4, 128, 5, MEANC), (2048, 3, 128, 5, MEANC), (2048, 4, 64, 5, MEANC), (2048, 4, 128, 300, MEANC),
                            (2 ** 26, 64, 128, 5, MEANC), (2048, 4, 128, 5, MIN), (2048, 4, 128, 5, MAX))],
]


def test_every_refusal_of_the_entry_points_is_the_planners_with_the_same_text():
    L = _lib.lib()
    for kw in REFUSED:
        rc_e, text_e = entry_refusal(L, **kw)
        rc_p, text_p = plan_refusal(L, **kw)
        assert rc_e == 1 and (rc_p, text_p) == (rc_e, text_e), (kw, text_e, text_p)
    # the texts the existing CPU tests match on, once each
    seen = " | ".join(plan_refusal(L, **kw)[1] for kw in REFUSED)
    for piece in ("outside the prefiltered subset", "Q x N too large", "Q x N P too large", "divisor of 64", "N * P", "min or max",
                  "combines by mean", "top_t under combine mean", "top_t must be 0 (all tokens) or 1 .. min(P, 16)", "whole live tile",
                  "first slice", "skyemb_prefilter_select_prepare's info", "skyemb_token_prefilter_select_prepare's info",
                  "skyemb_cosine_topk_prefiltered_lp_sel:", "skyemb_cosine_topk_prefiltered_resident:", "skyemb_cosine_topk_tokens_prefiltered_top:",
                  "skyemb_cosine_topk_tokens_prefiltered:", "skyemb_cosine_topk_tokens_mean_prefiltered:"):
        assert piece in seen, piece
    # requests no entry point takes
    for kw in (dict(kind=3, bank=F16), dict(kind=TOKENS, bank=F32), dict(kind=ROWS, bank=3), dict(kind=MEAN, bank=F16, n_live=4)):
        rc, text = plan_refusal(L, **{**dict(Q=17, N=4096, D=128, k=5, P=4, combine=MEANC if kw["kind"] == MEAN else MIN), **kw})
        assert rc == 1 and "no entry point takes this request" in text
    assert L.skyemb_prefilter_plan(None, None) == 1 and b"null argument" in L.skyemb_last_error()


# -------------------------------------------------------------------------------------------------------- the golden launch lists
def plan_of(c):
    kind = {"rows": ROWS, "tokens": TOKENS, "mean": MEAN}[c["kind"]]
    bank = {"f32": F32, "f16": F16, "bf16": BF16}[c["bank"]]
    sel = dict(zip(("n_live", "last_live"), pc.selection_info(c))) if c["dead"] is not None else {}
    lo = UNSET if c["lo"] is None else int(c["lo"])
    return ops.prefilter_plan(kind, bank, c["Q"], c["N"], c["D"], c["k"], P=c["P"], combine=ops.COMBINE_CODES[c["combine"]], top_t=c["top_t"],
                              thr0=c["thr0"], direct_sel=c["direct_sel"], lo=lo, **sel), kind, bank


def launches_of(c):
    """The launch list of a case, from the plan alone: the driver's order."""
    p, kind, bank = plan_of(c)
    Q = c["Q"]
    out = [(f"query16_kernel<{p.bf}>", [(p.q_padded + 3) // 4 * 256, 1], 256), ("init_state_kernel", [(p.q_padded + 255) // 256 * 256, 1], 256)]
    if kind != ROWS:
        out.append(("token_state_kernel", [(Q + 255) // 256 * 256, 1], 256))
    suffix = "bf" if p.bf else "lp"

    def stage1(mode, sel):
        return (f"prefilter_kernel<{mode},{p.use_lo},{int(sel)},{p.bf},{p.tok},{p.cnt}>", [256 * 512, 1], 512)

    for s in slices_of(p):
        out.append(stage1(s.mode, p.sel))
        if s.bucket:
            out.append(("bucket_kernel", [8 * 256, 256], 256))
        if s.tail:
            out.append(stage1(1, s.tail_sel))
        out.append((f"select_kernel<{p.sel}>" if kind == ROWS else f"token_rescore_{'top_' if p.top_t else ''}{suffix}_kernel", [Q * 256, 1], 256))
    if kind == ROWS:
        out.append((f"rescore_{'' if bank == F32 else suffix + '_'}kernel<{p.sel}>", [Q * 256, 1], 256))
    return [{"kernel": k, "grid": g, "workgroup": w} for k, g, w in out]


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prefilter_launches.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_golden_covers_the_cases():
    assert list(GOLDEN) == [c["id"] for c in pc.CASES] and len(set(GOLDEN)) == len(pc.CASES)
    kernels = {r["kernel"] for rows in GOLDEN.values() for r in rows}
    stage1 = {k for k in kernels if k.startswith("prefilter_kernel")}
    assert len(stage1) >= 30, len(stage1)                         # of the 56 instances
    assert {"rescore_kernel<0>", "rescore_kernel<1>", "rescore_lp_kernel<1>", "rescore_bf_kernel<1>", "select_kernel<1>", "token_rescore_top_bf_kernel",
            "token_rescore_top_lp_kernel", "token_rescore_lp_kernel", "token_rescore_bf_kernel"} <= kernels


@pytest.mark.parametrize("c", pc.CASES, ids=[c["id"] for c in pc.CASES])
def test_the_plan_rebuilds_the_traced_launches(c):
    assert launches_of(c) == GOLDEN[c["id"]]
