"""NumPy restatement of skyemb_token_mean_select_gather (include/skyemb.h): the compacted pooled image of a selection of images,
its row constants, its tail tile and the map compacted position -> image.  Bit patterns throughout: nothing is computed, rows are
copied.  No test lives here."""
import numpy as np

BT = 256
SENTINEL = np.array([0.0, np.nan, 0.0, 0.0], np.float32)         # the padding row of every rowp: its NaN fails the candidate test


def rowp_rows(S):
    return -(-S // BT) * BT


def gather(pooled_bits, rowp, idx):
    """pooled_bits u16 [N, D], rowp f32 [rows(N), 4], idx i64 [S] ascending -> (pooled_sel u16 [S, D], rowp_sel f32 [rows(S), 4],
    tail_sel u16 [256, D] or None when S is a whole number of tiles, map i32 [S])."""
    idx = np.asarray(idx, np.int64)
    S, D = idx.shape[0], pooled_bits.shape[1]
    assert S >= 1 and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < pooled_bits.shape[0]
    pooled_sel = pooled_bits[idx].copy()
    rowp_sel = np.tile(SENTINEL, (rowp_rows(S), 1))
    rowp_sel[:S] = rowp[idx]
    tail = None
    if S % BT:
        tail = np.zeros((BT, D), np.uint16)
        tail[:S % BT] = pooled_sel[S // BT * BT:]
    return pooled_sel, rowp_sel, tail, idx.astype(np.int32)


def same_bits(a, b):
    """Bitwise equality of two float32 arrays (NaN == NaN, +0 != -0)."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
