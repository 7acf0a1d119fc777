"""CPU statements of the two-stage token search under the top-t combine (``top_t``, the reference's n_top_sims; kernels:
prefilter_kernel<.., TOK, CNT> and the token_rescore_top kernels of csrc/topk_prefilter.hip), for
tests/test_token_topt_prefilter_{cpu,gpu}.py.

The rule.  With d[0] >= d[1] >= ... an image's token scores (-inf for a NaN score), 'min' under top_t = t scores d[t-1].
d[t-1] >= tau needs at least t tokens with an exact score >= tau; each of them passes the row test of stage 1 (U_i >= e_i, and a
row the bound gives up on passes every test), so the image is a candidate iff the COUNT of its passing rows is >= t.  t = P is the
AND fold of the plain 'min', t = 1 the OR fold of 'max'.  Scores are tests/token_topt_reference.py's; the row test, its sandwich
and the workspace read-back are tests/prefilter_stage1_reference.py's and tests/token_prefilter_stage_reference.py's, unchanged.

``count_fold_lanes`` restates the kernel's fold as it is written: bit-sliced ripple adders over the DPP row shifts and the two
nibble steps, the comparison with t plane by plane; ``count_candidates`` is the brute-force count it must equal."""
import functools

import numpy as np

from tests import prefilter_stage1_reference as sr
from tests import token_prefilter_stage_reference as tr
from tests import token_topt_reference as ttr

INF = sr.INF
BT = sr.BT
PS = tr.PS
MAX_TOP_T = ttr.MAX_TOP_T
# the (P, t) pairs of the GPU file: every DPP step, both nibble steps, the ends of the range (t = 1: the OR fold, t = P: the AND fold)
PAIRS = ((2, 1), (4, 2), (8, 5), (16, 2), (16, 15), (16, 16), (32, 3), (32, 16), (64, 9), (64, 16))


def all_pairs():
    return [(P, t) for P in PS for t in range(1, min(P, MAX_TOP_T) + 1)]


# ------------------------------------------------------------------------------------------------------------------ the candidate rule
def count_candidates(row_pass, P, t):
    """Candidate images [Q, N] from per-row pass bits [Q, N P]: at least t of the image's P rows passed."""
    r = np.asarray(row_pass, dtype=bool).reshape(row_pass.shape[0], -1, P)
    return r.sum(axis=2) >= t


def folds(P, combine, top_t):
    """(stage 1, stage 2) of the library under top_t (include/skyemb.h): 'and' | 'or' | 'count', 'min' | 'max' | 'top'."""
    if combine == "max":
        return "or", "max"
    assert combine == "min" and 0 <= top_t <= min(P, MAX_TOP_T)
    if top_t in (0, P):
        return "and", "min"
    return ("or" if top_t == 1 else "count"), "top"


def _row_shl(v, o):
    """DPP row_shl:o with bound_ctrl off and old = the lane's own value, over the last axis of 16 lanes: lane l takes lane l + o,
    a lane whose source lies outside the row keeps its own."""
    out = v.copy()
    out[..., :16 - o] = v[..., o:]
    return out


def _planes_add(c, y, npl):
    carry = np.zeros_like(c[0])
    for b in range(npl):
        x, g = c[b] ^ y[b], c[b] & y[b]
        c[b] = x ^ carry
        carry = g | (carry & x)
    c[npl] = carry


def count_fold_lanes(m, lgp, t):
    """The kernel's count_fold on uint32 words m [..., 16] (the 16 lanes of a DPP row; bit 4 i + j of a word is row fragment j of
    query block i): -> the words it leaves.  The first lane of every aligned group of 2^min(lgp, 4) lanes holds, at bit j (P <= 16),
    bits 0 and 2 (P = 32) or bit 0 (P = 64) of each nibble, whether at least t of the image's rows passed; everything else is 0."""
    m = np.asarray(m, dtype=np.uint32)
    lg16 = min(lgp, 4)
    c = [m.copy()] + [np.zeros_like(m) for _ in range(6)]
    for s in range(lg16):
        _planes_add(c, [_row_shl(p, 1 << s) for p in c], s + 1)
    if lgp >= 5:
        _planes_add(c, [p >> np.uint32(1) for p in c], 5)
    if lgp >= 6:
        _planes_add(c, [p >> np.uint32(2) for p in c], 6)
    ge = np.full_like(m, 0xFFFFFFFF)
    for b in range(7):
        ge = (c[b] & ge) if (t >> b) & 1 else (c[b] | ge)
    if lgp >= 5:
        ge &= np.uint32(0x55555555)
    if lgp >= 6:
        ge &= np.uint32(0x11111111)
    lanes = np.arange(16)
    return np.where((lanes & ((1 << lg16) - 1)) == 0, ge, np.uint32(0)).astype(np.uint32)


def strip_words(row_pass_strip):
    """Pass bits of one wave's strip, boolean [8 blocks, 64 rows] (row = 16 j + lane), as the lanes' words uint32 [16]."""
    b = np.asarray(row_pass_strip, dtype=bool).reshape(8, 4, 16)
    w = np.zeros(16, dtype=np.uint32)
    for i in range(8):
        for j in range(4):
            w |= (b[i, j].astype(np.uint32) << np.uint32(4 * i + j))
    return w


def strip_images(words, lgp):
    """The image bits of folded words [16] -> boolean [8 blocks, 64 >> lgp images of the strip], read where the append walk reads
    them: the image's first row (lane, bit j)."""
    P = 1 << lgp
    out = np.zeros((8, 64 // P), dtype=bool)
    for i in range(8):
        for g in range(64 // P):
            row = g * P
            out[i, g] = (int(words[row & 15]) >> (4 * i + (row >> 4))) & 1
    return out


# ------------------------------------------------------------------------------------------------------------------ the image sandwich
def image_sandwich_top(must_in_rows, must_out_rows, P, t):
    """The per-row sandwich [Q, N P] folded by the count: must-be-in iff at least t rows are must-be-in, must-be-out iff fewer than
    t rows are NOT must-be-out.  A row the bound gives up on is in neither class: it may pass, so it never helps an image out."""
    Q = must_in_rows.shape[0]
    mi = np.asarray(must_in_rows, dtype=bool).reshape(Q, -1, P)
    mo = np.asarray(must_out_rows, dtype=bool).reshape(Q, -1, P)
    must_in, must_out = mi.sum(axis=2) >= t, (~mo).sum(axis=2) < t
    assert not (must_in & must_out).any()
    return must_in, must_out


# ------------------------------------------------------------------------------------------------------------------------ inputs
QSTAR = tr.QSTAR


def case_k(P, N):
    """k of a case, from {1, 100, 256}: one the bank holds, whose first slice covers every whole tile, and which leaves the k-th
    best score among the ordinary images (P = 8 has 128 of them and some 80 planted images that reach t: k = 100, not 256)."""
    return 256 if P == 2 else 100 if N >= 100 else 1


@functools.lru_cache(maxsize=4)
def planted_case(P, t, fmt, lo, D=128, Q=24, seed=0):
    """A token bank for the designated query q* whose planted images hold exactly m "high" tokens (cosine ~ 0.999 with q*) and
    P - m "low" ones (their negation), m = t - 1, t, t + 1 (inside 0 .. P), at token positions that differ from image to image:
    every lane and nibble bit of the fold carries a decisive bit somewhere.  Tile layout (256 rows each): 4 ordinary tiles (Gaussian
    images), one tile per m, one tile of alternating all-high / all-low images, then a partial tail tile (1 .. 5 images) with one
    image per m: N P is just above 2048 and no multiple of 256.  thr0: a valid floor per query (below), in force during the one
    slice the search makes (asserted: one slice)."""
    from oracle import similarity_oracle as so
    rng = np.random.default_rng(7000 * seed + 100 * P + t + 3 * (fmt == "bf16") + 5 * lo)
    ipt = BT // P
    ms = sorted({m for m in (t - 1, t, t + 1) if 0 <= m <= P})
    lead = 4
    T = lead + len(ms) + 1
    T = max(T, 8)
    lead = T - len(ms) - 1
    tail_images = min(5, ipt - 1)
    assert tail_images >= 1
    N = T * ipt + tail_images
    k = case_k(P, N)
    q = rng.standard_normal((Q, D), dtype=np.float32)
    tw, qn = so.prep_queries_np(q, None)
    x = rng.standard_normal((N, 1, D)) + 0.7 * rng.standard_normal((N, P, D))
    highs = np.full(N, -1, dtype=np.int64)                       # planted images: their number of high tokens

    def plant(i, m, start):
        h = tw[QSTAR].astype(np.float64) * (1.0 + 0.05 * rng.standard_normal((P, D)))
        where = np.zeros(P, dtype=bool)
        if m:
            pos = (start + rng.permutation(P)[:m]) % P if i % 2 else (start + np.arange(m)) % P   # scattered / a run that wraps
            where[pos] = True
        h[~where] = -h[~where]
        x[i] = h
        highs[i] = m

    for n, m in enumerate(ms):
        for pos in range(ipt):
            plant((lead + n) * ipt + pos, m, pos)
    for pos in range(ipt):
        plant((lead + len(ms)) * ipt + pos, P if pos % 2 == 0 else 0, 0)
    for j in range(tail_images):
        plant(T * ipt + j, ms[j % len(ms)], j)
    xw = sr.store(x.reshape(N * P, D), fmt).reshape(N, P, D)
    flat = np.ascontiguousarray(xw.reshape(N * P, D))
    sched = tr.token_schedule(N, P, k)
    assert len(sched["slices"]) == 1 and sched["tail_live"], sched
    with np.errstate(all="ignore"):
        xn = so.wnorms_np(flat)
        rows = so.cosine_scores_np(q, flat, None)
        tok = np.where(np.isnan(rows), np.float32(-INF), rows).astype(np.float32).reshape(Q, N, P)
        combined = ttr.combine_top(tok, "min", t)
    qref = sr.query_constants(tw, qn, fmt, D, sr.eps_a_f32(fmt, D, lo))
    rref = sr.row_constants(flat, xn, fmt, D)
    den = sr.den32(qn, xn)
    score = sr.scores64(tw, flat, qn, xn)
    hw = sr.half_width(qref, rref, den)
    # a valid floor that stays far below the planted high tokens: the k-th best over the ordinary images when there are k of them,
    # else over the whole bank (then fewer than k planted images reach t high tokens)
    ordinary = np.flatnonzero(highs < 0)
    thr0 = tr.kth_finite(combined[:, ordinary] if len(ordinary) >= k else combined, k)
    assert (thr0 > -INF).all() and (thr0[QSTAR] < 0.9)
    c = dict(P=P, t=t, fmt=fmt, lo=lo, D=D, Q=Q, N=N, k=k, q=q, tw=tw, qn=qn, xw=xw, flat=flat, xn=xn, score=score, hw=hw, rows=rows,
             combined=combined, thr0=thr0, highs=highs, sched=sched)
    # the condition of the inputs: for q* every planted image is decided by its count alone
    must_in, must_out = image_classes(c, thr0)
    planted = highs >= 0
    assert must_in[QSTAR][planted & (highs >= t)].all() and must_out[QSTAR][planted & (highs < t)].all()
    assert (planted & (highs >= t)).any() and (planted & (highs < t)).any()
    return c


def image_classes(c, tau):
    mi, mo = sr.sandwich(tau, c["score"], c["hw"], c["rows"])
    return image_sandwich_top(mi, mo, c["P"], c["t"])


# ---- the random banks of the full-search tests: a centre per image plus token noise, N P just above 2048 rows and no multiple of 256
def random_bank(P, D, dtype, seed, rows=2048 + 3 * 64 + 0, Q=256):
    import torch
    rng = np.random.default_rng(seed)
    N = -(-rows // P) + (1 if (-(-rows // P) * P) % 256 == 0 else 0)
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = (rng.standard_normal((N, 1, D)) + 0.7 * rng.standard_normal((N, P, D))).astype(np.float32)
    bank = torch.from_numpy(x).to(dtype)
    return q, bank, bank.to(torch.float32).numpy()
