"""Statement, route predicates and case tables of the exact similarity search -- skyemb_cosine_topk, skyemb_cosine_scores,
skyemb_cosine_sample_floor, skyemb_weighted_norms[_lp] and skyemb_kth_largest_floor (csrc/topk.hip, topk_stream.hip,
topk_stream.h) -- for tests/test_exact_search_elementwise_gpu.py.  Pinned on the CPU by tests/test_exact_search_reference_cpu.py.

Statement.  The bits are those of the C oracle (oracle/topk_oracle.c through oracle.similarity_oracle): cosine_scores_np for a
score, wnorms_np / prep_queries_np for a norm and for tw = w t.  Every bar in this file is equality of the integer views.
    one partial list    the first min(k, m) of the m rows of the list's row range whose oracle score is STRICTLY above thr0[q]
                        (-inf when absent; a NaN score is -inf and therefore never kept), ordered by (score desc, index asc),
                        indices plus idx_offset; if m < k, entry m is (-inf, negative index).  The slots behind that terminator
                        are unspecified (include/skyemb.h).
    row ranges          streaming kernel: ceil(ceil(N / nlists) / 16) 16 rows per wavefront; tiled kernel: ceil(ceil(N / nchunks)
                        / BT) BT rows per chunk (BT = 256, or 128 under SKYEMB_TOPK_NW=4).  A range that starts at or behind N is
                        empty: its list is a lone terminator.
    merge               (score desc, index asc) over the valid prefixes, the first k, padded with (-inf, -1).
    sample floor        nextafter(k-th largest of the 16-row tile maxima of the oracle scores, -inf).
    k-th floor          nextafter(k-th largest of the row with NaN ranked as -inf, -inf); -0.0 and 0.0 step to the same number.
check_lists does not know the ranges (it holds whatever cut of the bank the kernel chose to the contract of the header);
check_ranges holds every list to its own range.  The route predicates restate the host dispatch of topk.hip / topk_stream.hip;
the CPU test compares their list counts with the library's for every case.
"""
from collections import namedtuple

import numpy as np

from oracle import similarity_oracle as so

INF = np.float32(np.inf)
EPS = 1e-6
LDS_CAP = 160 * 1024
PITCH = 20                                  # floats per staged operand row of the tiled kernel (BK + 4)
IDX_OFFSETS = (0, 2 ** 31 + 5, 2 ** 40)

TOPK_ROUTES = ("stream8", "stream4", "tile16", "tile64x256", "tile64x128")
SCORE_ROUTES = ("scores_stream", "scores16", "scores64")
NORM_ROUTES = ("rows<0,0>", "rows<0,1>", "rows<1,0>", "rows<1,1>", "flat")
KTH_ROUTES = ("wave", "bisect", "radix")
TILE = {"tile16": (16, 256, 4), "tile64x256": (64, 256, 8), "tile64x128": (64, 128, 4)}     # route -> (QT, BT, waves)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------- routes
def stream_applicable(Q, D, k):
    return Q <= 16 and k <= 128 and D % 64 == 0 and D <= 1024


def stream_waves(D, k):
    """8 wavefronts while the A image (64 D bytes) and 8 x 16 private lists of k (score, index) pairs fit in 160 KiB."""
    return 8 if 64 * D + 1024 * k <= LDS_CAP else 4


def stream_lists(N, D, k):
    w, blocks = stream_waves(D, k), 256
    while blocks > 1 and blocks * w * 64 > N:
        blocks >>= 1
    return blocks * w


def small_tile(Q, k):
    return Q <= 16 or k > 128


def tiled_chunks(N, Q, k, nw4=False):
    QT, BT = (16, 256) if small_tile(Q, k) else (64, 128 if nw4 else 256)
    want = max(1, 1024 // ceil_div(Q, QT))
    return max(1, min(want, ceil_div(N, BT * 8)))


def route(Q, N, D, k, stream_on=True, nw4=False):
    """-> (kernel of skyemb_cosine_topk, the list count skyemb_cosine_topk_chunks gives)."""
    if stream_on and stream_applicable(Q, D, k):
        return "stream%d" % stream_waves(D, k), stream_lists(N, D, k)
    name = "tile16" if small_tile(Q, k) else ("tile64x128" if nw4 else "tile64x256")
    return name, tiled_chunks(N, Q, k, nw4)


def tile_lds_bytes(name, k, scores_only=False):
    """Dynamic LDS of cosine_topk_kernel: two double-buffered operand tiles, the score slab, the lists (launch_topk)."""
    QT, BT, NW = TILE[name]
    slab = 128 if NW > 4 else BT
    return 4 * (2 * QT * PITCH + 2 * BT * PITCH + QT * (slab + 1) + (0 if scores_only else 2 * QT * k))


def largest_k(name):
    """The largest k launch_topk accepts on this tile (smem <= 160 KiB)."""
    QT = TILE[name][0]
    return (LDS_CAP - tile_lds_bytes(name, 0)) // (8 * QT)


def list_ranges(name, N, nlists):
    """The row range [lo, hi) of each list (hi <= lo: empty)."""
    if name.startswith("stream"):
        step = ceil_div(ceil_div(N, nlists), 16) * 16
    else:
        BT = TILE[name][1]
        step = ceil_div(ceil_div(N, nlists), BT) * BT
    return [(l * step, min(N, (l + 1) * step)) for l in range(nlists)]


def scores_route(Q, N, D, stream_on=True):
    if stream_on and Q <= 16 and D % 64 == 0 and D <= 1024 and N <= (1 << 20):
        return "scores_stream"
    return "scores16" if Q <= 16 else "scores64"


def sample_floor_applicable(Q, S, D, k, stream_on=True):
    if Q <= 0 or S <= 0 or D <= 0 or k < 1:
        return False
    tiles = ceil_div(S, 16)
    return scores_route(Q, S, D, stream_on) == "scores_stream" and tiles <= 2048 and k <= tiles


def norms_route(N, D, has_w, has_out, aligned=True):
    if N <= 16 and (N + 1) * (D + 4) * 4 <= 64 * 1024 and aligned:
        return "rows<%d,%d>" % (has_w, has_out)
    return "flat"


def kth_route(S):
    return "wave" if S <= 2048 else ("bisect" if S <= 32 * 1024 else "radix")


# ------------------------------------------------------------------------------------------------------------- statement
def topk_reference(srow, k, thr=-INF, idx_offset=0, lo=0, hi=None):
    """-> (scores[k], idx[k], m): the statement of one list over rows [lo, hi) of one query's oracle scores, padded with
    (-inf, -1) behind its m valid rows."""
    hi = len(srow) if hi is None else hi
    rows = np.arange(lo, max(lo, hi), dtype=np.int64)
    s = srow[lo:max(lo, hi)]
    keep = s > thr
    rows, s = rows[keep], s[keep]
    order = np.lexsort((rows, -s))[:k]
    out_s, out_i = np.full(k, -INF, np.float32), np.full(k, -1, np.int64)
    m = len(order)
    out_s[:m], out_i[:m] = s[order], rows[order] + idx_offset
    return out_s, out_i, int(keep.sum())


def valid_len(idx):
    neg = np.flatnonzero(idx < 0)
    return int(neg[0]) if neg.size else len(idx)


def merge_reference(part_s, part_i, k):
    """numpy merge of the valid prefixes of [Q, L, k] lists -> ([Q, k], [Q, k])."""
    Q, L, _ = part_s.shape
    out_s, out_i = np.full((Q, k), -INF, np.float32), np.full((Q, k), -1, np.int64)
    for q in range(Q):
        n = [valid_len(part_i[q, l]) for l in range(L)]
        s = np.concatenate([part_s[q, l, :n[l]] for l in range(L)])
        i = np.concatenate([part_i[q, l, :n[l]] for l in range(L)])
        order = np.lexsort((i, -s))[:k]
        out_s[q, :len(order)], out_i[q, :len(order)] = s[order], i[order]
    return out_s, out_i


def search_reference(scores_ref, k, thr0=None, idx_offset=0):
    """The merged answer: top-k of {rows: score > thr0[q]} per query, padded with (-inf, -1)."""
    Q = scores_ref.shape[0]
    out_s, out_i = np.empty((Q, k), np.float32), np.empty((Q, k), np.int64)
    for q in range(Q):
        out_s[q], out_i[q], _ = topk_reference(scores_ref[q], k, -INF if thr0 is None else thr0[q], idx_offset)
    return out_s, out_i


def restrict_by_floor(rs, ri, thr0=None, idx_offset=0):
    """cosine_topk_np's answer with the rows at or below the floor (and the -inf scores the oracle pads short banks with)
    removed: what the merged lists of skyemb_cosine_topk must equal."""
    out_s, out_i = np.full_like(rs, -INF), np.full_like(ri, -1)
    for q in range(rs.shape[0]):
        keep = rs[q] > (-INF if thr0 is None else thr0[q])
        m = int(keep.sum())
        assert keep[:m].all()                                           # sorted by score: the kept rows are a prefix
        out_s[q, :m], out_i[q, :m] = rs[q, :m], ri[q, :m] + idx_offset
    return out_s, out_i


def check_lists(part_s, part_i, scores_ref, N, k, thr0=None, idx_offset=0):
    """Hold [Q, L, k] partial lists to the contract of include/skyemb.h without knowing how the bank was cut into L ranges."""
    Q, L, kk = part_s.shape
    assert kk == k and part_i.shape == part_s.shape and scores_ref.shape == (Q, N)
    ref_bits = bits(scores_ref)
    for q in range(Q):
        thr = -INF if thr0 is None else thr0[q]
        rows_q = []
        for l in range(L):
            where = "query %d list %d" % (q, l)
            n = valid_len(part_i[q, l])
            s, i = part_s[q, l, :n], part_i[q, l, :n]
            if n < k:
                assert part_s[q, l, n] == -INF and part_i[q, l, n] < 0, \
                    "missing terminator: %s ends with (%r, %d) behind %d rows" % (where, part_s[q, l, n], part_i[q, l, n], n)
            rows = i - idx_offset
            assert ((rows >= 0) & (rows < N)).all(), "index outside the bank: %s has %s" % (where, i[(rows < 0) | (rows >= N)][:4])
            same = bits(s) == ref_bits[q, rows]
            assert same.all(), "wrong score bits: %s entry %d, row %d: %r for %r" % (
                where, np.flatnonzero(~same)[0], rows[~same][0], s[~same][0], scores_ref[q, rows[~same][0]])
            assert (s > thr).all(), "row at or below the floor %r: %s keeps %r" % (thr, where, s[~(s > thr)][:4])
            if n > 1:
                ordered = (s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] < i[1:]))
                assert ordered.all(), "not ordered by (score desc, index asc): %s at entry %d" % (where, np.flatnonzero(~ordered)[0])
            rows_q.append(rows)
        allrows = np.concatenate(rows_q)
        uniq, cnt = np.unique(allrows, return_counts=True)
        assert len(uniq) == len(allrows), "duplicate row across lists: query %d holds row(s) %s more than once" % (q, uniq[cnt > 1][:4])
    ms, mi = merge_reference(part_s, part_i, k)
    es, ei = search_reference(scores_ref, k, thr0, idx_offset)
    assert np.array_equal(mi, ei) and np.array_equal(bits(ms), bits(es)), \
        "merged lists differ from the top-k of the rows above the floor (first query %d)" % np.flatnonzero((mi != ei).any(1) | (bits(ms) != bits(es)).any(1))[0]


def check_ranges(part_s, part_i, scores_ref, k, thr0, idx_offset, ranges):
    """Every list against the statement over its own row range, terminator included."""
    Q, L, _ = part_s.shape
    assert L == len(ranges)
    for q in range(Q):
        thr = -INF if thr0 is None else thr0[q]
        for l, (lo, hi) in enumerate(ranges):
            es, ei, m = topk_reference(scores_ref[q], k, thr, idx_offset, lo, hi)
            n = min(k, m)
            assert np.array_equal(part_i[q, l, :n], ei[:n]) and np.array_equal(bits(part_s[q, l, :n]), bits(es[:n])), \
                "query %d list %d (rows %d..%d) differs from its statement" % (q, l, lo, hi)
            if n < k:
                assert part_s[q, l, n] == -INF and part_i[q, l, n] < 0, "query %d list %d: no terminator behind %d rows" % (q, l, n)


def statement_lists(scores_ref, k, thr0, idx_offset, ranges):
    """[Q, L, k] lists built from the statement; the slots behind a terminator hold junk (they are unspecified)."""
    Q = scores_ref.shape[0]
    ps, pi = np.full((Q, len(ranges), k), np.float32(3.25)), np.full((Q, len(ranges), k), 12345, np.int64)
    for q in range(Q):
        for l, (lo, hi) in enumerate(ranges):
            es, ei, m = topk_reference(scores_ref[q], k, -INF if thr0 is None else thr0[q], idx_offset, lo, hi)
            n = min(k, m + 1)
            ps[q, l, :n], pi[q, l, :n] = es[:n], ei[:n]
    return ps, pi


# ------------------------------------------------------------------------------------------------------------- data
def search_data(Q, N, D, weighted, seed):
    """-> (queries, bank, weights | None).  From 9 rows on: rows 0, 2 and N - 1 are exact duplicates (inside one 16-row step and
    across two ranges), row 5 holds a NaN, row 6 one inf, row 7 is zero; from 3 queries on, query 2 is zero (every finite row
    then scores 0: one long tie, resolved by index).  The oracle defines all of them."""
    g = np.random.default_rng(seed)
    q = g.standard_normal((Q, D), dtype=np.float32)
    x = g.standard_normal((N, D), dtype=np.float32)
    w = (g.random(D, dtype=np.float32) + np.float32(0.1)) if weighted else None
    if N >= 9:
        x[2] = x[0]
        x[N - 1] = x[0]
        x[5, 1 % D] = np.nan
        x[6, 0] = np.inf
        x[7] = 0
    if Q >= 3:
        q[2] = 0
    return q, x, w


FLOOR_FORMS = ("absent", "below_kth", "equal_to_a_score", "above_all")


def make_floors(scores_ref, k, shift=0):
    """-> (thr0 [Q] f32, the form of each query).  Query q takes form (q + shift) % 4: -inf (the kernel's own `absent`),
    nextafter(true k-th best, -inf), exactly the score in the middle of the top-k (that row and everything below it must go),
    and nextafter(best score, +inf) (every list of the query is a lone terminator)."""
    Q = scores_ref.shape[0]
    thr, forms = np.full(Q, -INF, np.float32), []
    for q in range(Q):
        ts, _, m = topk_reference(scores_ref[q], k)
        m = min(m, k)
        form = FLOOR_FORMS[(q + shift) % 4] if m > 0 else "absent"
        if form == "below_kth":
            thr[q] = np.nextafter(ts[m - 1], -INF)
        elif form == "equal_to_a_score":
            thr[q] = ts[m // 2]
        elif form == "above_all":
            thr[q] = np.nextafter(ts[0], INF)
        forms.append(form)
    return thr, forms


# ------------------------------------------------------------------------------------------------------------- top-k cases
TopkCase = namedtuple("TopkCase", "Q N D k weighted idx_offset nchunks route")


def _topk_cases(rows, **kw):
    out = []
    for n, r in enumerate(rows):
        Q, N, D, k = r[:4]
        nchunks = r[4] if len(r) > 4 else None
        out.append(TopkCase(Q, N, D, k, n % 2 == 0, IDX_OFFSETS[n % 3], nchunks, route(Q, N, D, k, **kw)[0]))
    return out


def topk_id(c):
    return "Q%d-N%d-D%d-k%d-%s-off%d%s" % (c.Q, c.N, c.D, c.k, "w" if c.weighted else "ones", IDX_OFFSETS.index(c.idx_offset),
                                          "" if c.nchunks is None else "-chunks%d" % c.nchunks)


# streaming kernel: N around one wavefront's 64 rows and around the workgroup's 64 w (w = 8 | 4 wavefronts), a slice that ends
# inside a 16-row step, Q on every 4g + r lane pattern, both sides of the wave switch (D = 768: k = 112 | 113; D = 1024: 96 | 97)
STREAM_CASES = _topk_cases([
    (1, 1, 64, 2), (3, 15, 64, 2), (5, 17, 64, 2), (15, 63, 64, 2), (16, 511, 64, 2), (1, 513, 64, 2), (3, 1024, 64, 2),
    (5, 2100, 64, 2), (5, 513, 192, 1), (16, 2100, 192, 128),
    (16, 2100, 768, 112), (16, 2100, 768, 113), (3, 257, 768, 128), (15, 255, 768, 113), (1, 512, 768, 128), (5, 511, 768, 1),
    (5, 63, 768, 128), (3, 15, 768, 113), (1, 1, 768, 113), (16, 17, 768, 128), (15, 17, 768, 2),           # N < k on both kernels
    (16, 2100, 1024, 96), (16, 2100, 1024, 97), (5, 513, 1024, 96), (3, 257, 1024, 97), (1, 63, 1024, 97),
])

# tiled kernel: Q around the 16- and 64-query tiles, k on both sides of 128 (the switch to the 16-query tile for any Q), D that
# is no multiple of the 16-wide k-step, D = 1028 (the first D the streaming kernel does not take), caller-chosen chunk counts
TILED_CASES = _topk_cases([
    (1, 257, 4, 1), (16, 2049, 1028, 128), (16, 255, 12, 129), (1, 1, 100, 1), (5, 256, 36, 300),
    (17, 256, 36, 128), (63, 2049, 100, 1), (64, 257, 36, 128), (65, 2049, 12, 128), (129, 255, 100, 1), (17, 1, 4, 1),
    (129, 255, 100, 129), (65, 257, 36, 300), (17, 2049, 1028, 129),
    (5, 300, 100, 10, 1), (5, 300, 100, 10, 3), (5, 300, 100, 10, 5),           # 3: a ragged second chunk and an empty third
    (65, 300, 36, 10, 1), (65, 300, 36, 10, 3), (65, 300, 36, 10, 6),           # 5 | 6: three | four trailing chunks empty
])

# the same rows under the two switches (read once per process: the GPU test runs them in child processes)
NW4_CASES = [c._replace(route="tile64x128") for c in TILED_CASES if route(c.Q, c.N, c.D, c.k, nw4=True)[0] == "tile64x128"]
STREAM_OFF_CASES = [c._replace(route=route(c.Q, c.N, c.D, c.k, stream_on=False)[0]) for c in STREAM_CASES + TILED_CASES if c.Q <= 16]


def case_nlists(c, **kw):
    return c.nchunks if c.nchunks is not None else route(c.Q, c.N, c.D, c.k, **kw)[1]


# ------------------------------------------------------------------------------------------------------------- scores
ScoreCase = namedtuple("ScoreCase", "Q N D weighted route")
SCORE_CASES = [ScoreCase(Q, N, D, n % 2 == 0, scores_route(Q, N, D)) for n, (Q, N, D) in enumerate([
    (1, 1, 64), (5, 15, 192), (16, 16, 768), (5, 17, 1024), (16, 1000, 64), (1, 4097, 192),
    (1, 1, 4), (5, 15, 100), (16, 16, 1028), (5, 17, 36), (16, 1000, 12), (5, 4097, 100),
    (17, 1, 4), (65, 15, 36), (17, 16, 100), (65, 17, 12), (17, 1000, 1028), (65, 4097, 100)])]
SCORE_STREAM_OFF_CASES = [c._replace(route=scores_route(c.Q, c.N, c.D, stream_on=False)) for c in SCORE_CASES if c.Q <= 16]


def score_id(c):
    return "Q%d-N%d-D%d-%s" % (c.Q, c.N, c.D, "w" if c.weighted else "ones")


# ------------------------------------------------------------------------------------------------------------- sample floor
FLOOR_TILE_LIMIT = 2048
FLOOR_S = (16, 40, 2050, 16 * 2048, 16 * 2048 - 7)
FLOOR_D = 64
FLOOR_CASES = [(Q, S, kk) for Q, S in zip((1, 5, 16, 16, 3), FLOOR_S) for kk in ("one", "tiles")]
# (Q, S, D, k): more than 2048 tiles, k above the tile count, D % 64, more than 16 queries
FLOOR_REFUSALS = [(4, 16 * 2048 + 1, 64, 1), (4, 40, 64, 4), (4, 40, 96, 1), (17, 40, 64, 1)]


def floor_id(c):
    return "Q%d-S%d-k_%s" % c


def floor_k(S, kk):
    return 1 if kk == "one" else ceil_div(S, 16)


def sample_floor_reference(scores_ref, k):
    """nextafter(k-th largest of the 16-row tile maxima, -inf); -> (floor [Q], tile maxima [Q, tiles])."""
    Q, S = scores_ref.shape
    tiles = ceil_div(S, 16)
    pad = np.full((Q, tiles * 16), -INF, np.float32)
    pad[:, :S] = scores_ref
    tmax = pad.reshape(Q, tiles, 16).max(axis=2)
    kth = -np.sort(-tmax, axis=1)[:, k - 1]
    return np.nextafter(kth, -INF).astype(np.float32), tmax


# ------------------------------------------------------------------------------------------------------------- weighted norms
NormCase = namedtuple("NormCase", "N D has_w has_out aligned route")
NORM_SHAPES = ((1, 64), (16, 100), (16, 956), (16, 960), (17, 100))      # N = 16: D = 956 is the last that fits 64 KiB of LDS
NORM_CASES = [NormCase(N, D, hw, ho, al, norms_route(N, D, hw, ho, al)) for N, D in NORM_SHAPES for hw in (0, 1) for ho in (0, 1)
              for al in ((True, False) if (N, D) == (16, 100) else (True,))]


def norm_id(c):
    return "N%d-D%d-w%d-out%d-%s" % (c.N, c.D, c.has_w, c.has_out, "aligned" if c.aligned else "off4")


def norm_data(N, D, seed=0):
    g = np.random.default_rng(seed + 31 * N + D)
    return g.standard_normal((N, D), dtype=np.float32), g.random(D, dtype=np.float32) + np.float32(0.1)


def norms_reference(x, w):
    """-> (norms [N], xw = w x [N, D]) in the oracle's own arithmetic (w None: ones, xw = x)."""
    xw, qn = so.prep_queries_np(x, w)
    norms = so.wnorms_np(x, w)
    assert np.array_equal(bits(norms), bits(qn))                        # the query norm and the bank norm are one chain
    return norms, xw


# ------------------------------------------------------------------------------------------------------------- k-th floor
KTH_S = (1, 2048, 2049, 32768, 32769)
KTH_RUN = 1500                                                            # equal values in row 1: more than the 1024-key pool
KTH_ROWS = ("normal", "run", "all_equal", "all_nan", "signed_zeros", "subnormals", "minus_inf")
KTH_CASES = [(S, kk) for S in KTH_S for kk in (("one",) if S == 1 else ("one", "S", "in_run"))]


def kth_id(c):
    return "S%d-k_%s" % c


def kth_data(S):
    g = np.random.default_rng(S)
    x = g.standard_normal((len(KTH_ROWS), S), dtype=np.float32)
    if S >= 2048:
        x[1, g.permutation(S)[:KTH_RUN]] = np.float32(0.25)
    x[2] = np.float32(3.5)
    x[3] = np.nan
    x[4] = np.where(g.random(S) < 0.5, np.float32(0.0), np.float32(-0.0))
    x[5] = (g.integers(1, 1 << 23, S).astype(np.int32) | (g.integers(0, 2, S).astype(np.int32) << 31)).view(np.float32)
    x[6, g.random(S) < 0.5] = -INF
    return x


def kth_k(x, kk):
    """k = 1, S, or a rank in the middle of row 1's run of equal values."""
    S = x.shape[1]
    return {"one": 1, "S": S}.get(kk) or int((x[1] > np.float32(0.25)).sum()) + KTH_RUN // 2


def kth_reference(x, k):
    v = np.where(np.isnan(x), -INF, x).astype(np.float32)
    kth = -np.sort(-v, axis=1)[:, k - 1]
    return np.nextafter(kth, -INF).astype(np.float32)
