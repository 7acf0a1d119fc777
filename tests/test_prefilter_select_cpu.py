"""CPU: the restatement of the two-stage search under a selection (tests/prefilter_select_reference.py) against hand-written
small cases -- the live-tile list, where the sentinel goes, the partial last tile, the take-all slots -- and the compacted-bank
mapping, ties across a deselected row included."""
import numpy as np

from oracle import similarity_oracle as so
from tests import prefilter_select_reference as psr
from tests import token_select_reference as tsel


def test_live_tile_list_and_tail_tile_by_hand():
    N = 3 * 256 + 37                                    # tiles 0, 1, 2 whole; tile 3 holds the last 37 rows
    f = np.zeros(N, bool)
    f[300] = True                                       # tile 1
    f[767] = True                                       # last row of tile 2
    tiles, last = psr.live_tiles(f)
    assert tiles.tolist() == [1, 2] and last == 0 and tiles.dtype == np.int32
    f[768] = True                                       # first row of the partial tile
    tiles, last = psr.live_tiles(f)
    assert tiles.tolist() == [1, 2, 3] and last == 1
    f[:] = False
    assert psr.live_tiles(f)[0].size == 0 and psr.live_tiles(f)[1] == 0
    f[:] = True
    assert psr.live_tiles(f)[0].tolist() == [0, 1, 2, 3]
    # the same list from the packed words the device reads: a popcount over the 8 words of a tile
    f[:] = False
    f[[0, 255, 256 + 31, 3 * 256 + 36]] = True
    words = tsel.pack_words(f)
    pc = [sum(bin(int(w)).count("1") for w in words[t * 8:t * 8 + 8]) for t in range(4)]
    assert pc == [2, 1, 0, 1] and psr.live_tiles(f)[0].tolist() == [t for t in range(4) if pc[t]]


def test_sentinel_placement_overrides_every_constant():
    N = 256 + 3
    rowp = np.arange(512 * 4, dtype=np.float32).reshape(512, 4) + 1
    rowp[5] = [0, np.inf, 1, 0]                         # an unboundable row: "keep for every query"
    rowp[6] = [0, np.inf, 1, 0]
    rowp[N:] = psr.SENTINEL                             # the padding the bank's own preparation wrote
    f = np.zeros(N, bool)
    f[[0, 6, 256, 258]] = True
    m = psr.masked_rowp(rowp, f)
    assert m.shape == rowp.shape
    for r in (0, 6, 256, 258):
        assert np.array_equal(m[r], rowp[r])
    assert np.isinf(m[6, 1]) and m[6, 2] == 1           # selected: still kept for every query
    off = np.setdiff1d(np.arange(512), [0, 6, 256, 258])
    assert np.isnan(m[off, 1]).all() and (m[off][:, [0, 2, 3]] == 0).all()     # row 5 and the padding included
    # NaN fails the candidate test t >= 0 whatever the other terms are
    assert not (np.float32(1e30) + np.float32(1.0) * m[5, 1] >= 0)


def test_take_all_slots_count_positions_not_bank_tiles():
    tiles = np.array([2, 5, 9], np.int32)
    assert psr.take_all_slot(0, 0) == 0 and psr.take_all_slot(1, 7) == 263 and psr.take_all_slot(2, 255) == 3 * 256 - 1
    assert int(tiles[1]) * psr.BT + 7 == 1287           # the index stored in slot 263


def test_compacted_bank_mapping_and_ties_across_a_deselected_row():
    rng = np.random.default_rng(0)
    Q, N, D, k = 3, 40, 16, 6
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = rng.standard_normal((N, D), dtype=np.float32)
    x[[4, 9, 30]] = q[0]                                # three exact ties at the top of query 0
    f = np.ones(N, bool)
    f[9] = False                                        # the middle one is deselected
    f[[0, 1, 2]] = False
    s, i = psr.topk_select(q, x, k, f, None, idx_offset=100)
    assert i[0, 0] == 104 and i[0, 1] == 130 and s[0, 0] == s[0, 1]          # lower bank row first, 9 skipped
    assert not np.isin(i - 100, [0, 1, 2, 9]).any()
    # equal to the whole-bank oracle with the deselected rows' scores removed
    full_s, full_i = so.cosine_topk_np(q, x, N, None)
    for qq in range(Q):
        keep = f[full_i[qq]]
        assert np.array_equal(i[qq] - 100, full_i[qq][keep][:k]) and np.array_equal(s[qq], full_s[qq][keep][:k])


def test_fewer_selected_rows_than_k_and_none():
    rng = np.random.default_rng(1)
    q = rng.standard_normal((2, 8), dtype=np.float32)
    x = rng.standard_normal((20, 8), dtype=np.float32)
    f = np.zeros(20, bool)
    f[[3, 17]] = True
    s, i = psr.topk_select(q, x, 5, f)
    assert set(i[0, :2].tolist()) == {3, 17} and (i[:, 2:] == -1).all() and np.isneginf(s[:, 2:]).all()
    f[:] = False
    s, i = psr.topk_select(q, x, 5, f)
    assert (i == -1).all() and np.isneginf(s).all()


def test_deselected_rows_change_nothing():
    rng = np.random.default_rng(2)
    q = rng.standard_normal((4, 8), dtype=np.float32)
    x = rng.standard_normal((64, 8), dtype=np.float32)
    f = rng.random(64) < 0.5
    ref = psr.topk_select(q, x, 7, f)
    y = x.copy()
    y[~f] = np.nan
    got = psr.topk_select(q, y, 7, f)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
