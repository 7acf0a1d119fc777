"""numpy restatement of the two-stage many-query patch-token search under a SELECTION of images (csrc/topk_prefilter.hip,
skyemb_token_prefilter_select_prepare / skyemb_cosine_topk_tokens_prefiltered_sel), built on tests/token_prefilter_reference.py, and
the inputs of the bit-exact GPU cases (shared by tests/test_token_prefilter_select_cpu.py and _gpu.py).

The selection is per IMAGE, the row constants and the 256-row tiles are per token ROW (row i belongs to image i // P):
  masked rowp   row i keeps its constants iff image i // P is selected; every other row and every padding row holds the sentinel
                {0, NaN, 0, 0}, whatever it held before -- the {0, inf, 1, 0} of an unboundable row included
  live tiles    the tiles with a row of a selected image, ascending; last_live: the bank's last tile (whole or partial) is one
  cum           for each live tile the number of selected images that begin in the tiles up to and including it
  image test    ``tpr.image_pass`` with every row of a deselected image failing (and never "unboundable")
  schedule      the unselected slices over POSITIONS of the live list; the first ends at the first position whose cum reaches 96 k
                (at least n_live / 128, at least 1); a live tail tile rides with the last slice as the list's last position
"""
import bisect
import functools

import numpy as np

from tests import token_prefilter_reference as tpr
from tests import token_search_reference as tsr

BT = tpr.BT
SENTINEL = np.array([0.0, np.nan, 0.0, 0.0], np.float32)


def row_mask(flags, P):
    return np.repeat(np.asarray(flags, dtype=bool), P)


def prepare(rowp, flags, P):
    """rowp f32 [rows padded to whole tiles, 4], bool [N], P in 1 .. 64 -> (masked rowp, tiles i32, cum i32, last_live)."""
    flags = np.asarray(flags, dtype=bool)
    rowp = np.asarray(rowp, np.float32)
    N = flags.shape[0]
    R = N * P
    assert 1 <= P <= 64 and rowp.shape[0] % BT == 0 and 0 <= rowp.shape[0] - R < BT
    rows = row_mask(flags, P)
    out = np.tile(SENTINEL, (rowp.shape[0], 1))
    out[:R][rows] = rowp[:R][rows]
    tiles_all = rowp.shape[0] // BT
    padded = np.zeros(tiles_all * BT, bool)
    padded[:R] = rows
    live = padded.reshape(tiles_all, BT).any(axis=1)
    begins = np.zeros(tiles_all, np.int64)                              # selected images that begin in each tile
    np.add.at(begins, (np.flatnonzero(flags) * P) // BT, 1)
    cum = np.cumsum(begins)
    tiles = np.flatnonzero(live).astype(np.int32)
    return out, tiles, cum[tiles].astype(np.int32), int(live[-1]) if tiles_all else 0


def image_pass(lhs, coef, ub, tau, P, combine, flags):
    """[Q, N] bool: the image test under the mask -- a row of a deselected image holds the sentinel: NaN fails, never unboundable."""
    rows = row_mask(flags, P)
    return tpr.image_pass(np.where(rows[None, :], lhs, np.nan), coef, ub & rows, tau, P, combine)


def direct_end(cum, n_live, k):
    """Position at which the first slice ends: the driver's rule (sky_embeddings_amd.search._topk_tokens_prefiltered)."""
    return min(max(bisect.bisect_left(list(cum), 96 * k) + 1, n_live // 128, 1), n_live)


def slices(tiles, cum, last_live, R, k):
    """[(first position, end position, 'direct' | 'staged')] over the live list; the last slice takes a live tail tile along."""
    n_live = len(tiles)
    tail_live = int(R % BT != 0 and last_live)
    T = n_live - tail_live
    assert T >= 1
    out, t0, first = [], 0, True
    for t1 in (min(direct_end(cum, n_live, k), T), T // 32, T // 8, T // 2, T):
        if t1 <= t0:
            continue
        out.append((t0, n_live if t1 == T else t1, "direct" if first else "staged"))
        t0, first = t1, False
    return out


def bootstrap_images(flags, k):
    """The strided sample of SELECTED whole images whose k-th best combined score is the first threshold."""
    where = np.flatnonzero(flags)
    S = min(where.size, max(16 * k, 256))
    return where[np.arange(S) * (where.size // S)]


def simulate(exact, lhs, coef, ub, P, k, combine, lo, flags):
    """``tpr.simulate`` under the selection -> (counts [phases, Q], flagged [Q] bool)."""
    flags = np.asarray(flags, dtype=bool)
    Q, N = exact.shape
    R = N * P
    rowp = np.zeros(((R + BT - 1) // BT * BT, 4), np.float32)
    _, tiles, cum, last_live = prepare(rowp, flags, P)
    sel_exact = np.where(flags[None, :], exact, -np.inf)
    tau = np.nextafter(tpr.kth_best(exact[:, bootstrap_images(flags, k)], k), np.float32(-np.inf)).astype(np.float64)
    ok_all = None
    counts, flagged, seen = [], np.zeros(Q, bool), np.zeros(N, bool)
    whole = R // BT
    for p0, p1, mode in slices(tiles, cum, last_live, R, k):
        ok_all = image_pass(lhs, coef, ub, tau, P, combine, flags)
        cand = np.zeros((Q, N), bool)
        for t in tiles[p0:p1]:
            i0, i1 = t * BT // P, min((t + 1) * BT // P, N)
            cand[:, i0:i1] = ok_all[:, i0:i1]
            seen[i0:i1] = True
            if mode == "staged" and t < whole:                          # (the tail tile appends directly)
                for qt in range(0, Q, tpr.QT[lo]):
                    item = cand[qt:qt + tpr.QT[lo], i0:i1]
                    if item.sum() > tpr.SCAP:
                        flagged[qt:qt + tpr.QT[lo]] |= item.any(axis=1)
        counts.append(cand.sum(axis=1))
        flagged |= counts[-1] > tpr.list_cap(k)
        tau = np.maximum(tau, tpr.kth_best(sel_exact[:, seen], k))
    return np.array(counts), flagged


# ---- the bit-exact GPU cases ----------------------------------------------------------------------------------------------------------
ROWS = 4096                                 # N P = ROWS + tail rows: 16 whole tiles, just above two of the route's minimum
KINDS = ("all", "half", "runs", "tail", "above")


def selection(kind, N, P, tail, k, seed=0):
    """bool [N].  all: every image; half: 50 % at random; runs: whole tiles deselected -- the first, two neighbours, one more and the
    tail tile -- with six in seven of the images of the others; tail: the tail tile's images (the last tile's, without a tail) and the whole
    tiles 5 .. 12; above / below: the first images of a 40 % random draw that make exactly 2048 rows / one image fewer."""
    rng = np.random.default_rng(1000 * seed + 7 * P + tail + len(kind))
    tile_of = (np.arange(N) * P) // BT
    last = int(tile_of[-1])
    if kind == "all":
        return np.ones(N, bool)
    if kind == "half":                                                  # exactly ceil(N / 2) images: at least 2048 rows
        f = np.zeros(N, bool)
        f[rng.permutation(N)[:(N + 1) // 2]] = True
        return f
    if kind == "runs":                                                  # 11 or 12 live tiles, one image in seven of them dropped
        f = ~np.isin(tile_of, [0, 3, 4, 9, last])
        on = np.flatnonzero(f)
        f[rng.permutation(on)[:on.size // 7]] = False
        return f
    if kind == "tail":
        return np.isin(tile_of, [5, 6, 7, 8, 9, 10, 11, 12, last])
    assert kind in ("above", "below")
    need = 2048 // P - (kind == "below")
    order = np.flatnonzero(rng.random(N) < 0.4)
    if order.size < need:
        order = np.arange(N)
    f = np.zeros(N, bool)
    f[order[:need]] = True
    return f


def _grid():
    """(P, combine, dtype, lo, Q, tail rows, k, weighted, idx_offset, kind): every P, dtype, combine, variant, tail and kind."""
    out, n = [], 0
    tails = lambda P: (0, P, 256 - P if P > 1 else 255)
    for P in (1, 4, 16, 32, 64):
        for kind in KINDS:
            dt, lo = (("f16", False), ("bf16", False), ("f16", True), ("bf16", True))[n % 4]
            combine = ("min", "max")[(n // 2 + P) % 2]
            Q = (17, 130)[n % 2]
            tail = tails(P)[(n + (kind == "tail")) % 3]
            if kind == "tail" and tail == 0:
                tail = P
            N = (ROWS + tail) // P
            ks = [kk for kk in (1, 7, 100) if kk <= 2048 // P]
            out.append((P, combine, dt, lo, Q, tail, ks[n % len(ks)], n % 3 == 0, (0, 1000003)[n % 2], kind))
            n += 1
    return out


CASES = _grid()
ORACLE_CASES = [next(c for c in CASES if c[2] == dt and c[9] == "half") for dt in ("f16", "bf16")]   # one per dtype, also vs numpy
D = 128


def case_id(c):
    P, combine, dt, lo, Q, tail, k, weighted, off, kind = c
    return f"P{P}-{combine}-{dt}-{'hilo' if lo else 'hi'}-Q{Q}-tail{tail}-k{k}-{'w' if weighted else 'u'}-off{off}-{kind}"


@functools.lru_cache(maxsize=None)
def case_inputs(P, tail, Q, weighted, dt):
    """``tpr.case_inputs`` at N P = ROWS + tail rows: (q, bank 16-bit [N, P, D] torch, its widened fp32 array, w or None)."""
    N = (ROWS + tail) // P
    rng = np.random.default_rng(P * 1000 + tail + Q + 5)
    q = rng.standard_normal((Q, D), dtype=np.float32)
    centre = rng.standard_normal((N, 1, D))
    x = (centre + 0.7 * rng.standard_normal((N, P, D))) * rng.uniform(0.2, 5.0, size=(N, 1, 1))
    w = None
    if weighted:
        w = (1.0 / (rng.random(D, dtype=np.float32) + 0.05) ** 2).astype(np.float32)
        w /= w.sum()
    bank, xw = tpr.to16(x, tpr.DTYPES[dt])
    return q, bank, xw, w


def case_flags(c):
    P, combine, dt, lo, Q, tail, k, weighted, off, kind = c
    return selection(kind, (ROWS + tail) // P, P, tail, k)


def compacted_topk(q, xw, k, combine, flags, w, idx_offset):
    """The numpy oracle on the compacted widened bank ``xw[flags]``, indices mapped back."""
    s, i = tsr.topk_tokens(q, np.ascontiguousarray(xw[flags]), k, combine, w)
    where = np.flatnonzero(flags).astype(np.int64)
    out = np.full(i.shape, -1, np.int64)
    out[i >= 0] = where[i[i >= 0]] + idx_offset
    return s, out
