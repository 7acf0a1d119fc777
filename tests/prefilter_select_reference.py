"""CPU restatement of the two-stage many-query search under a selection of the bank's rows (``select=`` of
sky_embeddings_amd.search.cosine_topk over a PreparedBank; csrc/topk_prefilter.hip).  Used by tests/test_prefilter_select_gpu.py
(bit for bit) and checked on the CPU by tests/test_prefilter_select_cpu.py.

The one rule: the search returns exactly what ``oracle.similarity_oracle.cosine_topk_np`` returns over the compacted bank
``x[flags]``, every index mapped back through ``flatnonzero(flags)`` and then offset by ``idx_offset``.  The mapping is monotone, so
the order (score desc, index asc) carries over and exact ties go to the lower bank row.  Entries past the selected count are
(-inf, -1).  For a resident fp16 bank ``x`` is the widened bank.

What the device prepares from the packed words (tests/token_select_reference.pack_words) is restated too:
  live tiles      the 256-row tiles with at least one selected row, ascending; the last tile may be a partial one
  masked rowp     the row constants [rows padded to whole tiles, 4] with the padding sentinel {0, NaN, 0, 0} in every deselected row
                  and every row past N -- whatever the row held before, the {0, inf, 1, 0} "keep for every query" constant included
"""
import numpy as np

from oracle import similarity_oracle as so

BT = 256                                   # bank rows per tile (csrc/topk_prefilter.hip)
NINF = np.float32(-np.inf)
SENTINEL = np.array([0.0, np.nan, 0.0, 0.0], np.float32)


def live_tiles(flags):
    """bool [N] -> (tiles int32 ascending, last_live): the tiles of ceil(N / BT) that hold a selected row, and whether the last
    bank tile (whole or partial) is one of them."""
    flags = np.asarray(flags, dtype=bool)
    N = flags.shape[0]
    tiles_all = (N + BT - 1) // BT
    padded = np.zeros(tiles_all * BT, bool)
    padded[:N] = flags
    live = padded.reshape(tiles_all, BT).any(axis=1)
    return np.flatnonzero(live).astype(np.int32), int(live[-1])


def masked_rowp(rowp, flags):
    """rowp f32 [rows_padded, 4], bool [N] -> the masked copy."""
    flags = np.asarray(flags, dtype=bool)
    rowp = np.asarray(rowp, np.float32)
    assert rowp.shape[0] % BT == 0 and 0 <= rowp.shape[0] - flags.shape[0] < BT
    out = np.tile(SENTINEL, (rowp.shape[0], 1))
    out[:flags.shape[0]][flags] = rowp[:flags.shape[0]][flags]
    return out


def take_all_slot(position, row_in_tile):
    """Slot of a (query, row) pair in the take-everything slice under a live-tile list: by POSITION in the list, not by bank
    tile; the index stored in the slot is the real bank row, ``tiles[position] * BT + row_in_tile``."""
    return position * BT + row_in_tile


def map_back(s, i, flags, idx_offset=0):
    where = np.flatnonzero(np.asarray(flags, dtype=bool)).astype(np.int64)
    out = np.full(i.shape, -1, np.int64)
    ok = i >= 0
    out[ok] = where[i[ok]] + idx_offset
    return s, out


def topk_select(queries, x, k, flags, weights=None, eps=1e-6, idx_offset=0):
    """(scores [Q, k] f32, indices [Q, k] i64) of the search under ``flags``: the compaction rule on ``cosine_topk_np``."""
    flags = np.asarray(flags, dtype=bool)
    assert flags.shape == (x.shape[0],)
    Q = np.asarray(queries).shape[0]
    s = np.full((Q, k), NINF, np.float32)
    i = np.full((Q, k), -1, np.int64)
    count = int(flags.sum())
    if count:
        kk = min(k, count)
        cs, ci = so.cosine_topk_np(queries, np.ascontiguousarray(np.asarray(x, np.float32)[flags]), kk, weights, eps)
        s[:, :kk], i[:, :kk] = map_back(cs, ci, flags, idx_offset)
    return s, i
