"""tests/large_bank_reference.py proved on banks small enough for the oracles to score whole: screen + oracle must equal the
oracle run on the whole bank, bit for bit, for flat and token banks (cosine min / mean / max, MSE / MAE), on fp32 and fp16
values, with exact duplicates, near-ties closer than the margin, NaN / inf / zero rows and a zero query."""
import numpy as np
import pytest
import torch

from oracle import similarity_oracle as so
from tests import large_bank_reference as lbr
from tests import token_distance_reference as tdr
from tests import token_search_reference as tsr

D, K = 64, 20


def _bank(rows, half, seed):
    """(bank [rows, D] fp32 numpy, queries [5, D], weights [D], planted row indices): queries 0 .. 3 are ordinary, query 4 is zero."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, D), dtype=np.float32) * rng.uniform(0.2, 5.0, (rows, 1)).astype(np.float32)
    q = rng.standard_normal((5, D), dtype=np.float32)
    q[4] = 0.0
    planted = []
    for j in range(3):                                              # near-copies of query j, far apart, and exact duplicates of them
        a, b, c = 7 + j, rows // 2 + j, rows - 1 - j
        x[a] = q[j] * np.float32(1.5) + np.float32(0.05) * rng.standard_normal(D, dtype=np.float32)
        x[b] = x[a]                                                # exact duplicate: the tie goes to the lower index
        x[c] = x[a] * (np.float32(1) + np.float32(2e-7))           # a near-tie far closer than the margin
        planted += [a, b, c]
    near = rows // 3
    x[near:near + 6] = x[near] + np.float32(1e-6) * rng.standard_normal((6, D), dtype=np.float32)   # six rows within the margin of each other
    x[rows // 4] = 0.0
    x[rows // 4 + 1, 3] = np.nan
    x[rows // 4 + 2, 5] = np.inf
    x[rows // 4 + 3, 9] = -np.inf
    planted += [rows // 4, rows // 4 + 1, rows // 4 + 2, rows // 4 + 3]
    if half:
        with np.errstate(over="ignore"):
            x, q = x.astype(np.float16).astype(np.float32), q.astype(np.float16).astype(np.float32)
    w = (rng.random(D, dtype=np.float32) + np.float32(0.1)).astype(np.float32)
    return x, q, w, np.array(planted)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_screen_plus_oracle_equals_the_oracle_on_a_flat_bank(half):
    x, q, w, planted = _bank(4000, half, 1)
    for weights in (w, None):
        want_s, want_i = so.cosine_topk_np(q[:4], x, K, weights)
        s64 = lbr.cosine_fp64(torch.from_numpy(q[:4]), torch.from_numpy(x), None if weights is None else torch.from_numpy(weights))
        got_s, got_i, most = lbr.screen_topk(s64, K, planted, lambda qi, idx: so.cosine_topk_np(q[qi:qi + 1], x[idx], K, weights),
                                             idx_offset=0)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s)
        assert K <= most <= 2 * K + len(planted)
        top3 = want_i[0, :3].tolist()
        assert sorted(top3) == [7, 2000, 3999] and top3.index(7) + 1 == top3.index(2000)   # the duplicate pair, lower index first
    # ... and with an index offset past 32 bits
    got_s, got_i, _ = lbr.screen_topk(s64, K, planted, lambda qi, idx: so.cosine_topk_np(q[qi:qi + 1], x[idx], K, None), idx_offset=5 << 32)
    assert np.array_equal(got_i, want_i + (5 << 32))


def test_a_zero_query_ties_every_row_and_the_cap_says_so():
    """Every row scores exactly 0 against a zero query: on a bank within the cap the screen keeps all of it and the lower indices
    win; on a larger bank the helper refuses (its cap is alive) instead of handing a whole bank to the oracle."""
    x, q, w, planted = _bank(4000, False, 2)
    small = np.ascontiguousarray(x[:2 * K])                         # (holds none of the NaN / inf rows)
    s64 = lbr.cosine_fp64(torch.from_numpy(q[4:5]), torch.from_numpy(small), torch.from_numpy(w))
    assert bool((s64 == 0).all())
    got_s, got_i, most = lbr.screen_topk(s64, K, [], lambda qi, idx: so.cosine_topk_np(q[4:5], small[idx], K, w))
    want_s, want_i = so.cosine_topk_np(q[4:5], small, K, w)
    assert most == 2 * K and np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s)
    assert got_i[0].tolist() == list(range(K))
    s64 = lbr.cosine_fp64(torch.from_numpy(q[4:5]), torch.from_numpy(x), torch.from_numpy(w))
    with pytest.raises(AssertionError, match="survivors"):
        lbr.screen_topk(s64, K, [], lambda qi, idx: so.cosine_topk_np(q[4:5], x[idx], K, w))


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("P", [4, 16])
def test_screen_plus_oracle_equals_the_oracle_on_a_token_bank(P, half):
    x, q, w, planted_rows = _bank(250 * 16, half, 3 + P)
    N = x.shape[0] // P
    bank = x.reshape(N, P, D)
    for j in range(3):                                              # one image made of near-copies of query j: it leads under every combine
        bank[40 + j] = q[j] * np.float32(1.5) + np.float32(0.05) * np.random.default_rng(j).standard_normal((P, D), dtype=np.float32)
    if half:
        bank = bank.astype(np.float16).astype(np.float32)
    planted = np.unique(np.concatenate((planted_rows // P, [40, 41, 42])))
    tok = lbr.cosine_fp64(torch.from_numpy(q[:4]), torch.from_numpy(bank.reshape(-1, D)), torch.from_numpy(w))
    for combine in lbr.COMBINES:
        want_s, want_i = tsr.topk_tokens(q[:4], bank, K, combine, w)
        got_s, got_i, _ = lbr.screen_topk(lbr.combine_fp64(tok, P, combine), K, planted,
                                          lambda qi, idx: tsr.topk_tokens(q[qi:qi + 1], bank[idx], K, combine, w))
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), combine
        assert 40 in want_i[0, :4] and 42 in want_i[2, :4]          # (under max the images of the single planted rows are up there too)
    c = tdr.prepare_c(w, D)
    for metric in tdr.METRICS:
        d64 = lbr.distance_fp64(torch.from_numpy(c), torch.from_numpy(q[:4]), torch.from_numpy(bank.reshape(-1, D)), metric)
        for combine in lbr.COMBINES:
            want_s, want_i = tdr.distance_topk_tokens(c, q[:4], bank, K, metric, combine)
            got_s, got_i, _ = lbr.screen_topk(lbr.combine_fp64(d64, P, combine, distance=True), K, planted,
                                              lambda qi, idx: tdr.distance_topk_tokens(c, q[qi:qi + 1], bank[idx], K, metric, combine),
                                              smallest=True)
            assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), (metric, combine)


def test_top_t_combine_in_fp64_follows_the_documented_rule():
    from tests import token_topt_reference as ttr
    x, q, w, _ = _bank(200 * 16, False, 9)
    bank = x.reshape(200, 16, D)
    tok = lbr.cosine_fp64(torch.from_numpy(q[:4]), torch.from_numpy(x), torch.from_numpy(w))
    for combine in lbr.COMBINES:
        want = ttr.combined_scores_top(q[:4], bank, combine, 5, w)
        got = lbr.combine_fp64(tok, 16, combine, top_t=5).numpy()
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(got)) and np.abs(got[fin] - want[fin]).max() < 2e-6, combine


def test_slices_hold_both_ends_every_line_and_a_strided_sample():
    sl = lbr.slices(100000, lines=(33333, 66666), width=64, sample=128)
    assert sl[0] == 0 and sl[-1] == 99999 and np.all(np.diff(sl) > 0)
    for must in (63, 99936, 33333 - 32, 33333, 33333 + 31, 66666, 781 * 5):
        assert must in sl
    assert len(sl) <= 4 * 64 + 128
    assert lbr.rows_of_images([2, 5], 4).tolist() == [8, 9, 10, 11, 20, 21, 22, 23]
