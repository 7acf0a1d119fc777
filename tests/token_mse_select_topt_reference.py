"""NumPy restatement of what the two-stage weighted-MSE token search adds under ``top_t`` and under a selection of images
(include/skyemb.h, skyemb_distance_topk_tokens_prefiltered_top / _sel / _top_sel): the key-space mapping of a distance request, the
combine under top_t, the selection's live tiles and the limits the select route asks of them.  The token distances themselves are
tests/token_mse_prefilter_reference.contract_distances; tests/test_token_mse_select_topt_cpu.py holds these rules against
tests/token_distance_reference.py and the library's own answers."""
import numpy as np

BT = 256                                # rows of a bank tile
MIN_LIVE_WHOLE_TILES = 8                # search.SELECT_MIN_LIVE_TILES
MIN_ROWS = 2048                         # the library's shape rule, applied to the selected images


def key_space_request(combine, top_t, P):
    """(key-space combine, the top_t stage 1 and 2 run under) of a DISTANCE request: keys are -distance, so distance 'min' is the
    key-space max -- a[0] whatever top_t says: the plain call --, distance 'max' the key-space min; there top_t == 0 and
    top_t == P are the plain call (a[P-1] is the max) and 1 <= top_t < P is the top_t-th largest key."""
    assert combine in ("min", "max") and 0 <= (top_t or 0) <= min(P, 16)
    if combine == "min":
        return "max", 0
    return "min", 0 if not top_t or top_t == P else top_t


def stage_folds(combine, top_t, P):
    """(stage 1 fold, stage 2 fold) in key space: 'or' | 'and' | 'count', 'max' | 'min' | 'top'."""
    key, t = key_space_request(combine, top_t, P)
    if key == "max":
        return "or", "max"
    if t == 0:
        return "and", "min"
    return ("or" if t == 1 else "count"), "top"


def combine_under_top_t(a, combine, top_t=None):
    """[Q, N, P] fp32 token distances -> [Q, N]: a NaN distance ranks as +inf; with a[0] <= a[1] <= ... 'min' is a[0] and 'max' is
    a[top_t-1] (top_t None / 0: a[P-1]); an image with fewer than top_t finite distances scores +inf under 'max'."""
    a = np.where(np.isnan(a), np.float32(np.inf), a).astype(np.float32)
    s = np.sort(a, axis=2)
    if combine == "min":
        return s[:, :, 0].copy()
    return s[:, :, (top_t or a.shape[2]) - 1].copy()


def topk(a, k, combine, top_t=None, flags=None, idx_offset=0):
    """(distances [Q, k] ascending, images [Q, k]) of the selected images (flags None: all), order (distance asc, image asc); an image
    that scores +inf is never returned; missing entries are (+inf, -1)."""
    d = combine_under_top_t(a, combine, top_t)
    Q, N = d.shape
    if flags is not None:
        d = np.where(np.asarray(flags, bool)[None, :], d, np.float32(np.inf))
    out_s = np.full((Q, k), np.inf, np.float32)
    out_i = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        order = np.lexsort((np.arange(N), d[q]))
        order = order[d[q][order] < np.inf][:k]
        out_s[q, :len(order)] = d[q][order]
        out_i[q, :len(order)] = order + idx_offset
    return out_s, out_i


def live_tiles(flags, P):
    """The selection as skyemb_token_prefilter_select_prepare reports it: (tiles -- the live 256-row tiles, ascending --, cum -- the
    selected images up to and including each --, last_live, whole -- the live WHOLE tiles)."""
    flags = np.asarray(flags, bool)
    R = flags.shape[0] * P
    rows = np.repeat(flags, P)
    n_tiles = -(-R // BT)
    padded = np.zeros(n_tiles * BT, bool)
    padded[:R] = rows
    per_tile = padded.reshape(n_tiles, BT).sum(axis=1) // P        # whole images: P divides 64 divides BT
    tiles = np.nonzero(per_tile)[0]
    cum = np.cumsum(per_tile)[tiles]
    last_live = bool(per_tile[-1] > 0)
    whole = len(tiles) - (1 if last_live and R % BT else 0)
    return tiles, cum, last_live, whole


def select_route_takes(flags, P, k):
    """True when the select route serves the selection: at least 8 live whole tiles, selected x P >= 2048 rows, k <= selected."""
    count = int(np.asarray(flags, bool).sum())
    return live_tiles(flags, P)[3] >= MIN_LIVE_WHOLE_TILES and count * P >= MIN_ROWS and k <= count


def direct_end(cum, k):
    """The live-list position at which the first slice ends (search.py): the first whose count reaches 96 k, at least n_live / 128."""
    n_live = len(cum)
    first = int(np.searchsorted(np.asarray(cum), 96 * k, side="left")) + 1
    return min(max(first, n_live // 128, 1), n_live)
