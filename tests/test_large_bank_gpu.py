"""The bank searches past 2^31 elements and 2^32 bytes: every kernel of csrc/topk*.hip, distance_tokens.hip and lp_bank.hip on
banks of [2 800 192, 768] -- the smallest that cross the lines -- against tests/large_bank_reference.py (slices of the score
outputs against the oracles, screen + oracle for the top-k lists), bit for bit.  A 32-bit slip in an address or an index does not
fault: it wraps and scores the wrong, in-bounds rows, which the oracle tests at 1 M x 768 (7.7e8 elements, 3.1e9 bytes) cannot see.

  H  fp16, 4.30 GB: row 2 796 202 straddles element 2^31 = byte 2^32; 3 989 rows lie beyond.  N = 64 x 43 753 (a whole token bank
     for P = 1, 4, 16, 64) and N % 256 = 64 (the resident two-stage path has a tail tile, whose base subtraction exceeds 2^32).
  G  fp32, 8.60 GB: row 1 398 101 straddles byte 2^32, row 2 796 202 element 2^31 and byte 2^33.
  B  bf16, H's shape: the norms and one score case.

Planted in all of them: near-copies of a common direction `base` (queries 0 .. 2 are base + 0.3 noise, so each scores > 0.9
against every one of them) at row 7, before / on / after both lines and at row N - 1; an exact duplicate of the row before the
last line at a row after it; a NaN row and a zero row beyond the last line; the 64-row image that holds the last line filled
with mild copies (score ~0.3), so that it leads under min and mean too; 300 near-copies of query FLOOD beyond the last line.

One bank is resident at a time (``banks``): the tests are ordered G, H, B and each bank is built once.
"""
import gc
import time

import numpy as np
import pytest
import torch

from oracle import similarity_oracle as so
from tests import large_bank_reference as lbr
from tests import token_distance_reference as tdr
from tests import token_pq_reference as tpq
from tests import token_search_reference as tsr
from tests import token_topt_reference as ttr

pytestmark = pytest.mark.gpu

N, D, K = 2_800_192, 768, 100
LINE32 = 1_398_101          # the row of an fp32 bank that straddles byte 2^32
LINE31 = 2_796_202          # the row that straddles element 2^31 (fp16: byte 2^32; fp32: byte 2^33)
QMANY, FLOOD = 33, 20
STRONG = (7, LINE32 - 1, LINE32, LINE32 + 1, LINE31 - 1, LINE31, LINE31 + 1, N - 1)
BLOCK = LINE31 // 64 * 64   # first row of the P = 64 image that holds the last line
DUP, NAN_ROW, ZERO_ROW, FLOOD0, NFLOOD = 2_796_300, 2_796_400, 2_796_401, 2_796_500, 300
PLANTED = np.unique(np.concatenate((STRONG, np.arange(BLOCK, BLOCK + 64), [DUP, NAN_ROW, ZERO_ROW], np.arange(FLOOD0, FLOOD0 + NFLOOD))))
DTYPES = {"G": torch.float32, "H": torch.float16, "B": torch.bfloat16}
NEED_GB = {"G": 21, "H": 9, "B": 7}     # the bank + what the tests on it allocate beside it
assert (LINE32 * D * 4 < 2 ** 32 < (LINE32 + 1) * D * 4) and (LINE31 * D < 2 ** 31 < (LINE31 + 1) * D) and N % 256 == 64 and N % 64 == 0


def _host_parts():
    rng = np.random.default_rng(20261019)
    base = rng.standard_normal(D, dtype=np.float32)
    q = rng.standard_normal((QMANY, D), dtype=np.float32) * rng.uniform(0.5, 2.0, (QMANY, 1)).astype(np.float32)
    q[:3] = base + np.float32(0.3) * rng.standard_normal((3, D), dtype=np.float32)
    w = (rng.random(D, dtype=np.float32) + np.float32(0.1)).astype(np.float32)
    strong = base + np.float32(0.05) * rng.standard_normal((len(STRONG), D), dtype=np.float32)
    mild = np.float32(0.35) * base + rng.standard_normal((64, D), dtype=np.float32)
    flood = q[FLOOD] + np.float32(0.01) * np.abs(q[FLOOD]).mean() * rng.standard_normal((NFLOOD, D), dtype=np.float32)
    wq = (rng.random((3, D), dtype=np.float32) + np.float32(0.1)).astype(np.float32)      # per-query weights of the _pq case
    return q, w, strong, mild, flood, wq


Q_H, W_H, _STRONG_H, _MILD_H, _FLOOD_H, WQ_H = _host_parts()


def _build(name):
    dtype = DTYPES[name]
    g = torch.Generator(device="cuda").manual_seed(2026)
    bank = torch.empty(N, D, device="cuda", dtype=dtype)
    for lo in range(0, N, 50_000):
        n = min(50_000, N - lo)
        x = torch.randn(n, D, device="cuda", generator=g)
        scale = 0.2 * 25.0 ** torch.rand(n, 1, device="cuda", generator=g)          # rows scaled over 0.2 .. 5
        bank[lo:lo + n] = (x * scale).to(dtype)
    put = lambda rows, v: bank.index_copy_(0, torch.as_tensor(np.asarray(rows), device="cuda"), torch.from_numpy(v).cuda().to(dtype))
    put(np.arange(BLOCK, BLOCK + 64), _MILD_H)
    put(STRONG, _STRONG_H)
    put(np.arange(FLOOD0, FLOOD0 + NFLOOD), _FLOOD_H)
    bank[DUP] = bank[LINE31 - 1]
    bank[NAN_ROW, 5] = float("nan")
    bank[ZERO_ROW] = 0
    return bank


class _Banks:
    """The one resident bank and what the tests derive from it once (``cache``); asking for another bank frees both first."""

    def __init__(self):
        self.name, self.bank, self.cache, self.built, self.survivors = None, None, {}, [], 0

    def get(self, name):
        if self.name != name:
            self.name, self.bank = None, None
            self.cache.clear()
            gc.collect()
            torch.cuda.empty_cache()
            free = torch.cuda.mem_get_info()[0]
            if free < NEED_GB[name] * 2 ** 30:
                pytest.skip(f"bank {name} and its tests need {NEED_GB[name]} GiB of device memory, {free / 2 ** 30:.1f} GiB are free")
            assert name not in self.built, f"bank {name} would be built twice: keep the tests ordered by bank"
            self.bank, self.name = _build(name), name
            self.built.append(name)
        return self.bank

    def once(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]


@pytest.fixture(scope="module")
def banks():
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    b = _Banks()
    yield b
    b.bank = None
    b.cache.clear()
    gc.collect()
    torch.cuda.empty_cache()
    print(f"\n[large-bank] banks built: {b.built}; peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB; largest survivor "
          f"count of the screen {b.survivors}; module wall time {time.time() - t0:.1f} s")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _eq(got_s, got_i, want_s, want_i, what=""):
    got_s, got_i = got_s.cpu().numpy(), got_i.cpu().numpy()
    bad = np.argwhere(got_i != want_i)
    assert bad.size == 0, (what, "first differing (query, rank)", bad[:3].tolist(), got_i[tuple(bad[0])], want_i[tuple(bad[0])])
    assert np.array_equal(got_s, want_s), (what, np.argwhere(got_s != want_s)[:3].tolist())


def _row_slices():
    return lbr.slices(N, (LINE32, LINE31))


def _norm_oracle(rows, w):
    """skyemb_weighted_norms' chain acc = fma(w[d] x[d], x[d], acc), one IEEE square root: tests/token_pq_reference.py's restatement,
    pinned to the C oracle bit for bit by tests/test_token_pq_cpu.py."""
    xw = rows if w is None else (w * rows).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(tpq.chain_rows(xw, rows)).astype(np.float32)


def _check_norms(bank, fn):
    sl = _row_slices()
    rows = lbr.gather_host(bank, sl)
    out = torch.empty(N, device="cuda")
    for w in (W_H, None):
        out.fill_(-1.0)
        fn(bank, None if w is None else _dev(w), out)
        got = out.cpu().numpy()
        assert np.array_equal(got[sl], _norm_oracle(rows, w), equal_nan=True), np.argwhere(got[sl] != _norm_oracle(rows, w))[:3]
        assert np.isnan(got).sum() == 1 and np.nanmin(got) >= 0      # every slot written (the NaN row's norm is NaN)


def _flat_expected(banks):
    """(scores [33, K], rows [33, K]) of the flat weighted search over the resident bank: screen + C oracle, computed once."""
    def make():
        bank = banks.bank
        s64 = lbr.cosine_fp64(_dev(Q_H), bank, _dev(W_H))
        s, i, most = lbr.screen_topk(s64, K, PLANTED, lambda qi, idx: so.cosine_topk_np(Q_H[qi:qi + 1], lbr.gather_host(bank, idx), K, W_H))
        banks.survivors = max(banks.survivors, most)
        print(f"[large-bank] flat {banks.name}: largest survivor count {most} (k = {K}, {len(PLANTED)} planted)")
        for j in range(3):
            assert set(STRONG) <= set(i[j].tolist()) and float(s[j, len(STRONG)]) > 0.9       # the planted rows lead, ...
            both = i[j].tolist()
            assert both.index(LINE31 - 1) + 1 == both.index(DUP)                           # ... the duplicate right behind its original
        assert set(i[FLOOD].tolist()) <= set(range(FLOOD0, FLOOD0 + NFLOOD))
        assert NAN_ROW not in i and ZERO_ROW not in i[:3]
        return s, i
    return banks.once("flat", make)


def _prepared(banks):
    from sky_embeddings_amd import search
    return banks.once("pb", lambda: search.PreparedBank(banks.bank, _dev(W_H)))


# ---------------------------------------------------------------------------------------------------------------- G (fp32)
def test_fp32_norms_across_the_lines(banks):
    from sky_embeddings_amd import ops
    _check_norms(banks.get("G"), ops.weighted_norms)


@pytest.mark.parametrize("prune", [True, False], ids=["floor", "nofloor"])
@pytest.mark.parametrize("Q", [3, 16])
def test_fp32_flat_topk_of_a_few_queries(banks, Q, prune):
    """The streaming kernel: its per-wave row ranges and the floor's strided sample both span the lines."""
    from sky_embeddings_amd import search
    banks.get("G")
    want_s, want_i = _flat_expected(banks)
    stats = {}
    s, i = search.cosine_topk(_dev(Q_H[:Q]), _prepared(banks), K, prune=prune, stats=stats)
    assert stats["path"] == "exact"
    _eq(s, i, want_s[:Q], want_i[:Q], f"Q={Q} prune={prune}")
    s, i = search.cosine_topk(_dev(Q_H[:Q]), _prepared(banks), 1, prune=prune)
    _eq(s, i, want_s[:Q, :1], want_i[:Q, :1], f"k=1 Q={Q} prune={prune}")


def test_fp32_flat_scores_across_the_lines(banks):
    from sky_embeddings_amd import search
    bank = banks.get("G")
    sl = _row_slices()
    for Q in (3, 16):
        got = search.cosine_scores(_dev(Q_H[:Q]), _prepared(banks)).index_select(1, _dev(sl)).cpu().numpy()
        want = so.cosine_scores_np(Q_H[:Q], lbr.gather_host(bank, sl), W_H)
        assert np.array_equal(got, want, equal_nan=True), (Q, sl[np.argwhere(got != want)[:3, 1]])


def test_fp32_flat_topk_of_many_queries(banks, monkeypatch):
    """Q = 33 on the two-stage path (skyemb_bank16_prepare's image + the fp32 re-score) and on the exact tiled kernel."""
    from sky_embeddings_amd import search
    banks.get("G")
    want_s, want_i = _flat_expected(banks)
    st = {}
    s, i = search.cosine_topk(_dev(Q_H), _prepared(banks), K, stats=st)
    assert st["path"] == "prefiltered"
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    ste = {}
    se, ie = search.cosine_topk(_dev(Q_H), _prepared(banks), K, stats=ste)
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER")
    assert ste["path"] == "exact"
    _eq(se, ie, want_s, want_i, "exact")
    _eq(s, i, want_s, want_i, "prefiltered")
    assert torch.equal(s, se) and torch.equal(i, ie)
    assert 1 <= st["redone"] <= 1 + QMANY // 10, st                  # the flooded query, and at most Q // 10 others
    _redone_holds_the_flood(banks, st)


def _redone_holds_the_flood(banks, st):
    """The flooded query must be among the re-done ones: without it the same search re-does one query fewer."""
    from sky_embeddings_amd import search
    keep = [j for j in range(QMANY) if j != FLOOD]
    st2 = {}
    search.cosine_topk(_dev(Q_H[keep]), _prepared(banks), K, stats=st2)
    assert st2["path"] == "prefiltered" and st2["redone"] == st["redone"] - 1 and st2["redone"] <= QMANY // 10, (st, st2)


def test_fp32_standardise_to_fp16_across_the_lines(banks):
    """The element-wise grid whose N * D / 4 float4s cross 2^29: the oracle's value rounded once, on the slices."""
    from sky_embeddings_amd import search
    bank = banks.get("G")
    rng = np.random.default_rng(5)
    mu, sd = rng.standard_normal(D, dtype=np.float32), rng.random(D, dtype=np.float32) + np.float32(0.5)
    out = search.standardise_to(bank, _dev(mu), _dev(sd), torch.float16)
    assert out.dtype == torch.float16 and out.shape == bank.shape
    sl = _row_slices()
    want = torch.from_numpy(so.standardise_np(lbr.gather_host(bank, sl), mu, sd)).to(torch.float16).float().numpy()
    got = lbr.gather_host(out, sl)
    assert np.array_equal(got, want, equal_nan=True), sl[np.argwhere(got != want)[:3, 0]]


# ---------------------------------------------------------------------------------------------------------------- H (fp16)
def test_fp16_norms_across_the_lines(banks):
    from sky_embeddings_amd import ops
    _check_norms(banks.get("H"), ops.weighted_norms_lp)


def test_fp16_flat_topk_of_many_queries(banks):
    """Q = 33 over the resident fp16 bank: skyemb_bank16_rowp_lp, the tail tile (its base lies 2^32 bytes and more below the tile)
    and the token route of the uncertified queries."""
    from sky_embeddings_amd import search
    banks.get("H")
    want_s, want_i = _flat_expected(banks)
    pb = _prepared(banks)
    st = {}
    s, i = search.cosine_topk(_dev(Q_H), pb, K, stats=st)
    assert st["path"] == "prefiltered" and pb.tail_tile is not None and pb.tail_tile.shape == (256, D)
    _eq(s, i, want_s, want_i, "prefiltered, resident fp16")
    assert N - 1 in want_i[0]                                        # a row of the tail tile is in the answer
    assert 1 <= st["redone"] <= 1 + QMANY // 10, st
    _redone_holds_the_flood(banks, st)


def _token_bank(banks, P):
    from sky_embeddings_amd import search
    return banks.once(("tb", P), lambda: search.TokenBank(banks.bank.view(N // P, P, D), _dev(W_H)))


def _tok64(banks):
    return banks.once("tok64", lambda: lbr.cosine_fp64(_dev(Q_H[:16]), banks.bank, _dev(W_H)))


def _images(rows, P):
    return np.unique(np.asarray(rows) // P)


def _token_oracle(bank, P, fn):
    """oracle(qi, images) of screen_topk from fn(qi, tokens [n, P, D] fp32 numpy) -> (s, i)."""
    return lambda qi, idx: fn(qi, lbr.gather_host(bank, lbr.rows_of_images(idx, P)).reshape(len(idx), P, D))


def _image_slices(P):
    return lbr.slices(N // P, (LINE32 // P, LINE31 // P), width=max(32, 2048 // P), sample=max(64, 4096 // P))


@pytest.mark.parametrize("combine", lbr.COMBINES)
@pytest.mark.parametrize("P", [4, 16, 64])
def test_fp16_token_search_across_the_lines(banks, P, combine):
    from sky_embeddings_amd import search
    bank = banks.get("H")
    Q = 16 if P == 16 else 3
    tb = _token_bank(banks, P)
    q = _dev(Q_H[:Q])
    sl = _image_slices(P)
    got = search.cosine_token_scores(q, tb, combine).index_select(1, _dev(sl)).cpu().numpy()
    want = tsr.combined_scores(Q_H[:Q], lbr.gather_host(bank, lbr.rows_of_images(sl, P)).reshape(len(sl), P, D), combine, W_H)
    assert np.array_equal(got, want), sl[np.argwhere(got != want)[:3, 1]]
    planted = _images(PLANTED, P)
    want_s, want_i, most = lbr.screen_topk(lbr.combine_fp64(_tok64(banks)[:Q], P, combine), K, planted,
                                           _token_oracle(bank, P, lambda qi, t: tsr.topk_tokens(Q_H[qi:qi + 1], t, K, combine, W_H)))
    banks.survivors = max(banks.survivors, most)
    for j in range(3):
        whole = set(range(BLOCK // P, (BLOCK + 64) // P))          # images made of planted rows only: they lead under every combine
        assert whole <= set(want_i[j].tolist())
        if combine == "max":
            assert set(_images(STRONG, P).tolist()) <= set(want_i[j].tolist())
    for prune in (True, False):
        st = {}
        s, i = search.cosine_topk_tokens(q, tb, K, combine, prune=prune, stats=st)
        assert st["pruned"] == (prune and N // P >= 8 * 256 * K)   # (the floor's size rule: only P = 4 has images enough)
        _eq(s, i, want_s, want_i, f"P={P} {combine} prune={prune}")


def test_fp16_token_search_top_t(banks):
    from sky_embeddings_amd import search
    bank, P, t = banks.get("H"), 16, 5
    q = _dev(Q_H[:3])
    for combine in ("min", "mean"):
        want_s, want_i, _ = lbr.screen_topk(lbr.combine_fp64(_tok64(banks)[:3], P, combine, top_t=t), K, _images(PLANTED, P),
                                            _token_oracle(bank, P, lambda qi, x: ttr.topk_tokens_top(Q_H[qi:qi + 1], x, K, combine, t, W_H)))
        s, i = search.cosine_topk_tokens(q, _token_bank(banks, P), K, combine, top_t=t)
        _eq(s, i, want_s, want_i, f"top_t {combine}")
        assert LINE31 // P in want_i[0]


def test_fp16_token_search_with_a_selection_beyond_the_last_line(banks):
    """Every image before the last line is deselected, a random half of those after it selected: what is found lies past 2^31."""
    from sky_embeddings_amd import search
    bank, P, k = banks.get("H"), 4, 50
    n = N // P
    first = LINE31 // P + 1                                          # the first image that lies wholly beyond the line
    flags = np.zeros(n, bool)
    flags[first:] = np.random.default_rng(3).random(n - first) < 0.5
    assert k < flags.sum() < 600
    comb = lbr.combine_fp64(_tok64(banks)[:3], P, "max").clone()
    comb[:, _dev(~flags)] = -np.inf
    planted = np.array([m for m in _images(PLANTED, P) if flags[m]])
    want_s, want_i, _ = lbr.screen_topk(comb, k, planted, _token_oracle(bank, P, lambda qi, x: tsr.topk_tokens(Q_H[qi:qi + 1], x, k, "max", W_H)))
    assert want_i.min() >= first
    st = {}
    s, i = search.cosine_topk_tokens(_dev(Q_H[:3]), _token_bank(banks, P), k, "max", select=_dev(flags), stats=st)
    assert st["selected"] == int(flags.sum())
    _eq(s, i, want_s, want_i, "select")
    got = search.cosine_token_scores(_dev(Q_H[:3]), _token_bank(banks, P), "max", select=_dev(flags))
    assert bool(torch.isinf(got[:, _dev(~flags)]).all()) and bool((got[:, _dev(flags)] > -np.inf).all())


def test_fp16_token_search_with_per_query_weights(banks):
    from sky_embeddings_amd import search
    bank, P, k = banks.get("H"), 16, 30
    tok = lbr.cosine_fp64(_dev(Q_H[:3]), bank, _dev(WQ_H))
    want_s, want_i, _ = lbr.screen_topk(lbr.combine_fp64(tok, P, "max"), k, _images(np.concatenate((STRONG, [DUP])), P),
                                        _token_oracle(bank, P, lambda qi, x: tpq.topk_tokens_pq(Q_H[qi:qi + 1], x, k, "max", WQ_H[qi:qi + 1])))
    st = {}
    s, i = search.cosine_topk_tokens(_dev(Q_H[:3]), bank.view(N // P, P, D), k, "max", weights=_dev(WQ_H), stats=st)
    assert st["per_query_weights"] is True
    _eq(s, i, want_s, want_i, "per-query weights")
    assert {LINE31 // P, (N - 1) // P, 0} <= set(want_i[0].tolist())


def test_fp16_token_search_returns_an_index_offset_past_32_bits_unclipped(banks):
    from sky_embeddings_amd import search
    bank, P, off = banks.get("H"), 16, 5 * 2 ** 32
    want_s, want_i, _ = lbr.screen_topk(lbr.combine_fp64(_tok64(banks)[:3], P, "max"), K, _images(PLANTED, P),
                                        _token_oracle(bank, P, lambda qi, x: tsr.topk_tokens(Q_H[qi:qi + 1], x, K, "max", W_H)), idx_offset=off)
    tb = search.TokenBank(bank.view(N // P, P, D), _dev(W_H), idx_offset=off)
    s, i = search.cosine_topk_tokens(_dev(Q_H[:3]), tb, K, "max")
    _eq(s, i, want_s, want_i, "idx_offset")
    assert int(i.min()) >= off and int(i.max()) == off + (N - 1) // P


@pytest.mark.parametrize("P", [4, 16])
@pytest.mark.parametrize("metric", tdr.METRICS)
def test_fp16_distance_search_across_the_lines(banks, metric, P):
    from sky_embeddings_amd import search
    bank = banks.get("H")
    q, tokens = _dev(Q_H[:3]), bank.view(N // P, P, D)
    c = search.prepare_distance_weights(_dev(W_H), D, bank.device)
    c_h = c.cpu().numpy()                                            # the library's own c (torch sums in another order than NumPy)
    sl = _image_slices(P)
    got = search.distance_token_scores(q, tokens, metric, "mean", _dev(W_H)).index_select(1, _dev(sl)).cpu().numpy()
    rows = lbr.gather_host(bank, lbr.rows_of_images(sl, P)).reshape(len(sl), P, D)
    want = tdr.combine_distances(tdr.token_distances(c_h, Q_H[:3], rows, metric), "mean")
    assert np.array_equal(got, want), sl[np.argwhere(got != want)[:3, 1]]
    d64 = banks.once(("d64", metric), lambda: lbr.distance_fp64(c, q, bank, metric))
    want_s, want_i, most = lbr.screen_topk(lbr.combine_fp64(d64, P, "mean", distance=True), K, _images(PLANTED, P),
                                           _token_oracle(bank, P, lambda qi, x: tdr.distance_topk_tokens(c_h, Q_H[qi:qi + 1], x, K, metric, "mean")),
                                           smallest=True)
    banks.survivors = max(banks.survivors, most)
    s, i = search.distance_topk_tokens(q, tokens, K, metric, "mean", _dev(W_H))
    _eq(s, i, want_s, want_i, f"{metric} P={P}")


# ---------------------------------------------------------------------------------------------------------------- B (bf16)
def test_bf16_norms_across_the_lines(banks):
    from sky_embeddings_amd import ops
    _check_norms(banks.get("B"), ops.weighted_norms_lp)


def test_bf16_token_scores_across_the_lines(banks):
    from sky_embeddings_amd import search
    bank, P = banks.get("B"), 16
    sl = _image_slices(P)
    got = search.cosine_token_scores(_dev(Q_H[:16]), bank.view(N // P, P, D), "mean", _dev(W_H)).index_select(1, _dev(sl)).cpu().numpy()
    want = tsr.combined_scores(Q_H[:16], lbr.gather_host(bank, lbr.rows_of_images(sl, P)).reshape(len(sl), P, D), "mean", W_H)
    assert np.array_equal(got, want), sl[np.argwhere(got != want)[:3, 1]]
