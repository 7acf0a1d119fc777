"""GPU: the two-stage many-query search under a selection -- ``cosine_topk(queries, PreparedBank(bank), k, select=...)`` over an
fp32 and a resident fp16 bank.  The reference is tests/prefilter_select_reference.topk_select: ``cosine_topk_np`` over the compacted
bank (the widened one for fp16), indices mapped back; scores and indices must be bit-equal.

Shapes: N = 40 x 256 + 37, D = 128 -- at k = 5 the phases of the unselected schedule end at tiles 8, 9, 20 and 40 (take-all, direct
append, staged), and the fp16 bank has a tail tile of 37 rows.  On every parent of this feature the calls are a ValueError."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import similarity_oracle as so
from tests import prefilter_select_reference as psr

N0, D0, BT = 40 * 256 + 37, 128, 256
DTYPES = [np.float32, np.float16]


@functools.lru_cache(maxsize=None)
def _base(dtype, D=D0, Q=300):
    """Queries, bank (rows of very different scale, planted exact ties; for fp16: rounded once, the reference sees it widened) and
    weights, drawn as in test_prefiltered_many_query_topk_is_bit_exact."""
    rng = np.random.default_rng(Q * 7 + N0 + D)
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = (rng.standard_normal((N0, D)) * rng.uniform(0.2, 5.0, size=(N0, 1))).astype(np.float32).astype(dtype)
    sc0 = so.cosine_scores_np(q[:1], x.astype(np.float32), None)[0]
    best = np.argsort(-sc0)[:3]
    x[N0 - 1], x[N0 // 2 + 1], x[7] = x[best[0]], x[best[1]], x[best[2]]      # exact ties: lower index first
    w = (1.0 / (rng.random(D, dtype=np.float32) + 0.05) ** 2).astype(np.float32)
    w /= w.sum()
    return q, x, w


def _pb(x, w, idx_offset=0):
    from sky_embeddings_amd import search
    return search.PreparedBank(torch.from_numpy(x).cuda(), None if w is None else torch.from_numpy(w).cuda(), idx_offset)


def _search(q, pb, k, select, **kw):
    from sky_embeddings_amd import search
    stats = {}
    sel = torch.from_numpy(select) if isinstance(select, np.ndarray) else select
    s, i = search.cosine_topk(torch.from_numpy(q).cuda(), pb, k, stats=stats, select=sel, **kw)
    return s.cpu().numpy(), i.cpu().numpy(), stats


def _assert_equal(got, ref, stats=None):
    (s, i), (ref_s, ref_i) = got[:2], ref
    assert np.array_equal(i, ref_i), (stats, np.argwhere(i != ref_i)[:5])
    assert np.array_equal(s.view(np.uint32), ref_s.view(np.uint32)), stats


def _check(q, x, w, k, flags, cap=True, idx_offset=0):
    """One search against the reference; returns its stats.  cap: the redo cap of the unselected tests on these inputs."""
    got = _search(q, _pb(x, w, idx_offset), k, flags)
    print(got[2])
    _assert_equal(got, psr.topk_select(q, x.astype(np.float32), k, flags, w, idx_offset=idx_offset), got[2])
    assert got[2]["path"] == "prefiltered" and got[2]["selected"] == int(flags.sum())
    live = psr.live_tiles(flags)[0].size
    assert got[2]["tiles"] == (live, (x.shape[0] + BT - 1) // BT)
    if cap:
        assert got[2]["redone"] <= q.shape[0] // 10, got[2]
    return got[2]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Q,k", [(17, 5), (300, 100), (17, 192)])
def test_all_true_selection_equals_the_unselected_search(dtype, Q, k):
    from sky_embeddings_amd import search
    q, x, w = _base(dtype)
    q = q[:Q]
    pb = _pb(x, w)
    flags = np.ones(N0, bool)
    got = _search(q, pb, k, flags)
    ref = so.cosine_topk_np(q, x.astype(np.float32), k, w)
    _assert_equal(got, ref, got[2])
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] <= Q // 10 and got[2]["tiles"] == (41, 41)
    s0, i0 = search.cosine_topk(torch.from_numpy(q).cuda(), pb, k)
    assert np.array_equal(s0.cpu().numpy().view(np.uint32), got[0].view(np.uint32)) and np.array_equal(i0.cpu().numpy(), got[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frac,Q,k", [(0.5, 300, 5), (0.1, 17, 5), (0.1, 300, 100), (0.5, 17, 192)])
def test_random_selections(dtype, frac, Q, k):
    """50 % and 10 %: every tile stays live, so at k = 5 the take-all, direct-append and staged phases all run (tiles 8, 9, 20, 40)."""
    q, x, w = _base(dtype)
    flags = np.random.default_rng(int(frac * 100) + Q).random(N0) < frac
    stats = _check(q[:Q], x, w, k, flags)
    assert stats["tiles"] == (41, 41)


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_selection_two_pass_variant(dtype, monkeypatch):
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", "1")
    q, x, w = _base(dtype)
    _check(q, x, w, 5, np.random.default_rng(77).random(N0) < 0.5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_selection_at_768_features(dtype):
    q, x, w = _base(dtype, 768, 17)
    _check(q, x, w, 100, np.random.default_rng(768).random(N0) < 0.5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_best_rows_deselected(dtype):
    """Near-copies of several queries are planted and deselected: the answer must change, so a search that ignored the mask fails."""
    q, x, w = _base(dtype)
    q, x = q[:40], x.copy()
    rng = np.random.default_rng(3)
    planted = []
    for j, qq in enumerate((0, 7, 16, 17, 39)):
        rows = np.array([100 + j, 2600 + 300 * j, N0 - 2 - j])           # first slice, later slices, the tail tile
        x[rows] = ((1.5 + j) * q[qq] + 1e-3 * rng.standard_normal((3, D0))).astype(np.float32).astype(dtype)
        planted.append(rows)
    flags = np.ones(N0, bool)
    flags[np.concatenate(planted)] = False
    k = 5
    ref = psr.topk_select(q, x.astype(np.float32), k, flags, w)
    whole = so.cosine_topk_np(q, x.astype(np.float32), k, w)
    for qq in (0, 7, 16, 17, 39):
        assert not np.array_equal(ref[1][qq], whole[1][qq])
    got = _search(q, _pb(x, w), k, flags)
    _assert_equal(got, ref, got[2])


def _tile_flags(tiles_on, tail_rows=()):
    f = np.zeros(N0, bool)
    for t in tiles_on:
        f[t * BT:(t + 1) * BT] = True
    f[list(tail_rows)] = True
    return f


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tail", ["some", "none"])
def test_whole_tiles_deselected(dtype, tail):
    """Tile 0, the last whole tile (39) and a run in the middle are deselected; the partial last tile holds three selected rows, or
    none (then a resident fp16 bank's tail tile is not launched)."""
    q, x, w = _base(dtype)
    on = [t for t in range(40) if t not in (0, 5, 6, 7, 8, 20, 39)]
    flags = _tile_flags(on, (40 * BT, 40 * BT + 17, N0 - 1) if tail == "some" else ())
    flags &= np.random.default_rng(9).random(N0) < 0.8
    flags[N0 - 1] = tail == "some"
    stats = _check(q, x, w, 5, flags)
    assert stats["tiles"] == (33 + (tail == "some"), 41)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_first_slice(dtype):
    """The first eight live tiles hold one selected row each (k = 100: the first slice has no k-th lower bound to raise the threshold
    from, and its 2040 masked pairs must not count); the rest is selected at 10 %, so no list can overflow: at most
    8 + 30 x 256 x ~0.1 candidates reach the direct-append phase, far below the 4096 slots.  Hence the usual redo cap holds."""
    q, x, w = _base(dtype)
    flags = np.random.default_rng(5).random(N0) < 0.1
    flags[:12 * BT] = False
    for j, t in enumerate((1, 2, 3, 5, 6, 8, 10, 11)):
        flags[t * BT + 31 * j] = True
    assert psr.live_tiles(flags)[0][:8].tolist() == [1, 2, 3, 5, 6, 8, 10, 11]
    _check(q[:17], x, w, 100, flags)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fewer_selected_rows_than_k_none_and_a_small_selection(dtype):
    q, x, w = _base(dtype)
    q = q[:17]
    flags = np.zeros(N0, bool)
    flags[np.arange(10) * 4 * BT + 3] = True                     # 10 live tiles, one row each
    flags[np.arange(40) * BT + 200] = True                       # 50 rows in all over 40 tiles
    stats = _check(q, x, w, 100, flags, cap=False)
    assert stats["redone"] == 0 and stats["selected"] == 50
    # none selected: all (-inf, -1), no stage-1 launch
    none = np.zeros(N0, bool)
    s, i, stats = _search(q, _pb(x, w), 100, none)
    assert np.isneginf(s).all() and (i == -1).all() and stats["selected"] == 0 and stats["redone"] == 0
    # fewer than 8 live whole tiles: the token search, the same answer
    few = np.zeros(N0, bool)
    few[2 * BT:5 * BT] = True
    few[N0 - 5:] = True
    got = _search(q, _pb(x, w), 100, few)
    _assert_equal(got, psr.topk_select(q, x.astype(np.float32), 100, few, w), got[2])
    assert got[2]["path"] == "tokens" and got[2]["tiles"] == (4, 41)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_deselected_rows_change_nothing(dtype):
    """NaN, inf, zero and 2^-120-scale rows (fp16: subnormal-scale) among the deselected: bit-equal to the same bank with ordinary
    rows there -- in particular the 'keep for every query' constant of an unboundable row is overridden by the mask."""
    q, x, w = _base(dtype)
    flags = np.random.default_rng(6).random(N0) < 0.5
    bad = np.flatnonzero(~flags)
    hostile = x.copy()
    hostile[bad[0::4]] = np.nan
    hostile[bad[1::4], 7] = np.inf
    hostile[bad[2::4]] = 0
    hostile[bad[3::4]] = (np.float32(2.0 ** -120) if dtype == np.float32 else np.float16(2.0 ** -24)) * np.ones(D0, dtype)
    a = _search(q[:40], _pb(x, w), 5, flags)
    b = _search(q[:40], _pb(hostile, w), 5, flags)
    _assert_equal(b, a[:2], b[2])
    assert b[2]["redone"] == a[2]["redone"]
    _assert_equal(b, psr.topk_select(q[:40], x.astype(np.float32), 5, flags, w), b[2])


@pytest.mark.parametrize("dtype", DTYPES)
def test_forced_redo_under_a_selection(dtype):
    """Hundreds of selected near-duplicates around the k-th score: more candidates than the re-score quota, the query is flagged
    and re-run by the token search under the same selection."""
    rng = np.random.default_rng(5)
    Q, D, k = 96, 128, 60
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = rng.standard_normal((N0, D), dtype=np.float32)
    x[1000:1600] = q[3] + 1e-5 * rng.standard_normal((600, D)).astype(np.float32)
    x[2000:2300] = 2.5 * q[10] + 1e-6 * rng.standard_normal((300, D)).astype(np.float32)
    x = x.astype(dtype)
    w = rng.random(D, dtype=np.float32) + 0.1
    w /= w.sum()
    flags = rng.random(N0) < 0.5
    flags[1000:1600] = True
    flags[2000:2300:2] = True
    stats = _check(q, x, w, k, flags, cap=False)
    assert stats["redone"] >= 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_shards_with_idx_offset_merge_to_the_single_bank(dtype):
    from sky_embeddings_amd import ops
    q, x, w = _base(dtype)
    q, k = q[:40], 5
    flags = np.random.default_rng(8).random(N0) < 0.5
    cut = 20 * BT + 100
    parts = []
    for lo, hi in ((0, cut), (cut, N0)):
        shard = np.ascontiguousarray(x[lo:hi])
        got = _search(q, _pb(shard, w, lo), k, flags[lo:hi])
        _assert_equal(got, psr.topk_select(q, shard.astype(np.float32), k, flags[lo:hi], w, idx_offset=lo), got[2])
        assert got[2]["path"] == "prefiltered" and got[2]["redone"] <= 40 // 10, got[2]
        parts.append((torch.from_numpy(got[0]).cuda(), torch.from_numpy(got[1]).cuda()))
    gs = torch.stack([p[0] for p in parts], dim=1).contiguous()
    gi = torch.stack([p[1] for p in parts], dim=1).contiguous()
    out_s, out_i = torch.empty(40, k, device="cuda"), torch.empty(40, k, device="cuda", dtype=torch.int64)
    ops.topk_merge(gs, gi, 40, 2, k, out_s, out_i)
    _assert_equal((out_s.cpu().numpy(), out_i.cpu().numpy()), psr.topk_select(q, x.astype(np.float32), k, flags, w))


def test_a_selection_is_prepared_once_per_bank_and_weights(monkeypatch):
    from sky_embeddings_amd import ops, search
    q, x, w = _base(np.float32)
    q, k = q[:17], 5
    x16 = _base(np.float16)[1]
    flags = np.random.default_rng(10).random(N0) < 0.5
    calls = []
    real = ops.prefilter_select_prepare
    monkeypatch.setattr(ops, "prefilter_select_prepare", lambda *a: (calls.append(1), real(*a))[1])
    sel = search.Selection(torch.from_numpy(flags).cuda())
    pb32, pb16 = _pb(x, w), _pb(x16, w)
    ref32 = psr.topk_select(q, x, k, flags, w)
    ref16 = psr.topk_select(q, x16.astype(np.float32), k, flags, w)
    for _ in range(2):
        _assert_equal(_search(q, pb32, k, sel), ref32)
        _assert_equal(_search(q, pb16, k, sel), ref16)
    assert len(calls) == 2                                       # once per bank
    w2 = np.roll(w, 3).copy()
    pb32.set_weights(torch.from_numpy(w2).cuda())
    _assert_equal(_search(q, pb32, k, sel), psr.topk_select(q, x, k, flags, w2))
    _assert_equal(_search(q, pb32, k, sel), psr.topk_select(q, x, k, flags, w2))
    _assert_equal(_search(q, pb16, k, sel), ref16)
    assert len(calls) == 3                                       # the weights of pb32 changed: prepared anew, once
    # a bool tensor on the host: packed and prepared on every call
    _assert_equal(_search(q, pb32, k, flags), psr.topk_select(q, x, k, flags, w2))
    _assert_equal(_search(q, pb32, k, flags), psr.topk_select(q, x, k, flags, w2))
    assert len(calls) == 5


def test_argument_errors_before_any_launch(monkeypatch):
    from sky_embeddings_amd import ops, search
    q, x, w = _base(np.float32)
    qd = torch.from_numpy(q[:17]).cuda()
    pb = _pb(x, w)
    rng = np.random.default_rng(0)
    pb160 = _pb(rng.standard_normal((4096, 160), dtype=np.float32), None)
    q160 = torch.from_numpy(rng.standard_normal((17, 160), dtype=np.float32)).cuda()

    def no_launch(*a, **k):
        raise AssertionError("a launch before the argument check")
    for name in ("prefilter_select_prepare", "cosine_topk_prefiltered_sel", "pack_select", "weighted_norms", "cosine_token_topk",
                 "bank16_prepare"):
        monkeypatch.setattr(ops, name, no_launch)
    with pytest.raises(ValueError, match="select describes"):
        search.cosine_topk(qd, pb, 5, select=torch.ones(N0 - 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool tensor"):
        search.cosine_topk(qd, pb, 5, select=torch.ones(N0, dtype=torch.uint8))
    with pytest.raises(ValueError, match="bool tensor"):
        search.cosine_topk(qd, pb, 5, select=torch.ones(N0, 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="D % 64 == 0"):        # the limits of the route the uncertified queries take
        search.cosine_topk(q160, pb160, 5, select=torch.ones(4096, dtype=torch.bool))
    with pytest.raises(ValueError, match="per-query weights"):
        search.cosine_topk(qd, pb, 5, weights=torch.ones(17, D0), select=torch.ones(N0, dtype=torch.bool))
    with pytest.raises(ValueError, match="cosine_topk_tokens"):   # Q = 1: the two-stage route does not apply -- as ever
        search.cosine_topk(qd[:1], pb, 5, select=torch.ones(N0, dtype=torch.bool))
    monkeypatch.undo()
    if torch.cuda.device_count() > 1:
        other = search.Selection(torch.ones(N0, dtype=torch.bool), device=torch.device("cuda", 1))
        with pytest.raises(ValueError, match="packed on"):
            search.cosine_topk(qd, pb, 5, select=other)
    else:                                                         # one GPU: the same refusal through the check itself
        sel = search.Selection(torch.ones(N0, dtype=torch.bool))
        with pytest.raises(ValueError, match="packed on"):
            search._selection_arg(sel, N0, "cosine_topk", torch.device("cuda", 1))


def test_the_prepared_selection_is_the_restatement():
    """ops.prefilter_select_prepare against tests/prefilter_select_reference: the live tiles in order, the last-tile flag and the
    masked row constants -- sentinel in every deselected and every padding row, the 'keep for every query' constant of an inf row
    overridden when the row is deselected and kept when it is selected."""
    from sky_embeddings_amd import ops, search
    from tests import token_select_reference as tsel
    rng = np.random.default_rng(21)
    N = 9 * BT + 37
    x = rng.standard_normal((N, 64), dtype=np.float32)
    x[5, 3] = x[300, 0] = np.inf                                 # unboundable rows: 5 stays selected, 300 is deselected
    pb = _pb(x, None)
    rowp = pb.half_image()[1]
    assert rowp.shape == (10 * BT, 4)
    for tail in (True, False):
        flags = np.zeros(N, bool)
        flags[[0, 5, 255, 2 * BT + 31, 2 * BT + 32, 7 * BT, 8 * BT + 255]] = True     # tiles 0, 2, 7, 8; word and tile edges
        flags[4 * BT:5 * BT] = rng.random(BT) < 0.5                                   # tile 4
        flags[[N - 1, 9 * BT]] = tail                                                 # the partial tile 9
        words = torch.from_numpy(tsel.pack_words(flags).view(np.int32)).cuda()
        sel = search.Selection(torch.from_numpy(flags))
        assert torch.equal(sel.words, words)
        rowp_sel, tiles, n_live, last_live = ops.prefilter_select_prepare(sel.words, N, rowp)
        ref_tiles, ref_last = psr.live_tiles(flags)
        assert ref_tiles.tolist() == [0, 2, 4, 7, 8] + [9] * tail
        assert n_live == ref_tiles.size and last_live == ref_last == int(tail)
        assert tiles.dtype == torch.int32 and tiles[:n_live].cpu().numpy().tolist() == ref_tiles.tolist()
        got, ref = rowp_sel.cpu().numpy(), psr.masked_rowp(rowp.cpu().numpy(), flags)
        assert np.array_equal(got.view(np.uint32) & 0x7fffffff, ref.view(np.uint32) & 0x7fffffff)     # bit for bit, up to a NaN's sign
        assert np.isinf(got[5, 1]) and got[5, 2] == 1 and np.isnan(got[300, 1]) and got[300, 2] == 0
        assert np.isnan(got[N:, 1]).all() and (got[N:, 2] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_selected_nan_row_with_fewer_rows_than_k(dtype):
    """Fewer selected rows than k, some of them with a NaN: such a row scores -inf and is not returned, wherever it lies (as in the
    token search, which serves the small selections and the re-run queries) -- the answer is that of the selection without them.
    With k rows or more above -inf the rule never shows: -inf ranks last."""
    q, x, w = _base(dtype)
    q, x = q[:17], x.copy()
    flags = np.zeros(N0, bool)
    flags[np.arange(40) * BT + 9] = True
    x[3 * BT + 9, 5] = np.nan                                    # selected, in the take-all slice
    x[30 * BT + 9] = np.nan                                      # selected, in a later slice
    x[3 * BT + 10] = np.nan                                      # deselected
    finite = flags.copy()
    finite[[3 * BT + 9, 30 * BT + 9]] = False
    ref = psr.topk_select(q, x.astype(np.float32), 100, finite, w)
    assert (ref[1][:, 38:] == -1).all()
    got = _search(q, _pb(x, w), 100, flags)
    _assert_equal(got, ref, got[2])
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] == 0
