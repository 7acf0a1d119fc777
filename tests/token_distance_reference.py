"""CPU restatement of the weighted MSE / MAE patch-token search (sky_embeddings_amd.search.distance_token_scores /
distance_topk_tokens, kernels in csrc/distance_tokens.hip), NumPy fp32 in the contract's exact operation order.  Used by
tests/test_token_distance_gpu.py (bit for bit) and pinned on the CPU against the reference goldens by
tests/test_token_distance_cpu.py.

Arithmetic contract (include/skyemb.h and csrc/distance_tokens.hip state the same, word for word):
  All arithmetic is fp32, every operation rounds to nearest even on its own, and there is no fused multiply-add anywhere in
  the score.  With c = fp32(w / sum(w)) [D] prepared by the caller, t [D] the query and x [D] a bank row (a 16-bit row is
  widened exactly on load):
    term[d] = c[d] * v[d],  v[d] = |x[d] - t[d]| for MAE,  v[d] = (x[d] - t[d]) * (x[d] - t[d]) for MSE;
    16 partial sums: p[j] = 0, then p[j] = p[j] + term[d] over the elements with (d >> 2) & 15 == j, in ascending d;
    four folds: p[j] = p[j] + p[j ^ 8], then p[j] = p[j] + p[j ^ 4], then p[j] = p[j] + p[j ^ 2], then p[j] = p[j] + p[j ^ 1]
    (every fold on all 16 partials at once; addition commutes, so afterwards all 16 are equal);
    dist = p[0] / (float)D, one IEEE division.
  The order does not depend on Q, launch geometry, wave, P, bank dtype, top_t or the selection.

NumPy rounds every float32 operation on its own and never fuses, so the loops below ARE that contract: vectorised over the rows
and the 16 partials, D / 16 sequential steps (element d = 64 m + 4 j + e of partial j at step (m, e)), four folds, one division.

Combine per (query, image).  A NaN token distance counts as +inf (torch would propagate the NaN).  With a[0] <= a[1] <= ... the
top_t smallest token distances (top_t None: all P):
  min   a[0], for every top_t;
  max   the largest of those used: a[top_t - 1], or the plain max;
  mean  acc = 0; acc = acc + a[j] for j = 0 .. top_t - 1, smallest first; acc / float32(top_t).  top_t None: token order
        p = 0 .. P-1, divided by float32(P) -- so top_t == P differs from the plain mean by the summation order only.
A +inf token distance is ignored by min and makes max and mean +inf, as does an image with fewer than top_t finite token
distances under max and mean.  top-k: lexsort on (distance, image); images whose combined distance is +inf are never returned;
missing entries are (+inf, -1).  Selection: the search over the compacted bank, indices mapped back (tests/token_select_reference.py).

Error bound of the contract against the reference formula mean_d(v[d] * c[d]) evaluated in fp64 from the same fp32 inputs
(c, t, x), for c >= 0.  u = 2^-24 is the unit roundoff, every fl() below is one rounding (1 + delta), |delta| <= u:
  * a term: fl(x - t) is one rounding; |.| is exact, the square is fl(d * d) with d carrying one rounding already, i.e. three
    factors; times c one more.  MAE: 2 roundings per term, MSE: 4.
  * every term is >= 0, so nothing cancels: in a sum of non-negative numbers each partial result's rounding scales the terms
    it contains by (1 + delta), and the relative error of the whole sum is at most that of its worst term.  A term passes
    through at most D / 16 - 1 roundings inside its partial (the first add, to 0, is exact; a partial has D / 16 terms), then
    through the 4 folds, then through the division: D / 16 + 4 roundings.
  * together at most n = D / 16 + 4 + 4 = D / 16 + 8 factors (1 + delta) on any term, so
        |dist - exact| <= ((1 + u)^n - 1) * exact <= gamma(n) * exact,   gamma(n) = n u / (1 - n u),   n = D / 16 + 8.
  * combine: min, max and the order statistics a[j] select values, they round nothing, and an order statistic of perturbed
    positive values moves by no more than the largest relative perturbation; mean adds T - 1 roundings in its sum (the first
    add is exact) and one in its division: n = D / 16 + 8 + T with T = top_t, or P for the plain mean.
D = 64: 12 u = 7.2e-7 for a token distance.
"""
import numpy as np

from tests import token_select_reference as tsel

METRICS = ("MSE", "MAE")
COMBINES = ("min", "mean", "max")
MAX_TOP_T = 16
PINF = np.float32(np.inf)
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def distance_bound(D, combine="min", count=1):
    """Relative bound of a combined distance against the fp64 formula (the docstring's derivation): count = top_t or P for mean."""
    return gamma(D // 16 + 8 + (count if combine == "mean" else 0))


def prepare_c(weights, D):
    """c = fp32(w / sum(w)) as NumPy rounds it; the GPU tests read the library's own c back instead (torch sums in another order)."""
    w = np.ones(D, np.float32) if weights is None else np.asarray(weights, np.float32)
    return (w / w.sum(dtype=np.float32)).astype(np.float32)


def token_distances(c, queries, bank, metric):
    """[Q, N, P] fp32 token distances; NaN stays NaN here (the combine ranks it)."""
    assert metric in METRICS
    bank = np.ascontiguousarray(bank, dtype=np.float32)
    N, P, D = bank.shape
    assert D % 64 == 0
    x = bank.reshape(N * P, D)
    c = np.asarray(c, np.float32)
    q = np.asarray(queries, np.float32)
    out = np.empty((q.shape[0], N * P), np.float32)
    j = np.arange(16)
    with np.errstate(invalid="ignore", over="ignore"):
        for qi in range(q.shape[0]):
            p = np.zeros((N * P, 16), np.float32)
            for m in range(D // 64):
                for e in range(4):
                    cols = 64 * m + 4 * j + e
                    d = x[:, cols] - q[qi, cols]
                    v = np.abs(d) if metric == "MAE" else d * d
                    p = p + c[cols] * v
            for f in (8, 4, 2, 1):
                p = p + p[:, j ^ f]
            out[qi] = p[:, 0] / np.float32(D)
    assert out.dtype == np.float32
    return out.reshape(-1, N, P)


def exact_token_distances(c, queries, bank, metric):
    """The reference formula in fp64 from the same fp32 inputs: mean over d of c[d] * v[d]."""
    x = np.asarray(bank, np.float32).astype(np.float64)
    d = x[None] - np.asarray(queries, np.float32).astype(np.float64)[:, None, None, :]
    v = np.abs(d) if metric == "MAE" else d * d
    return (v * np.asarray(c, np.float32).astype(np.float64)).mean(axis=-1)


def combine_distances(a, combine, top_t=None):
    """[Q, N, P] fp32 token distances -> [Q, N]."""
    assert a.dtype == np.float32 and combine in COMBINES
    a = np.where(np.isnan(a), PINF, a).astype(np.float32)
    P = a.shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        if top_t is None:
            if combine == "min":
                return a.min(axis=2)
            if combine == "max":
                return a.max(axis=2)
            used, count = a, P
        else:
            assert 1 <= top_t <= min(P, MAX_TOP_T)
            s = np.sort(a, axis=2)                                  # ascending, +inf last
            if combine == "min":
                return s[:, :, 0].copy()
            if combine == "max":
                return s[:, :, top_t - 1].copy()
            used, count = s, top_t
        acc = np.zeros(a.shape[:2], np.float32)
        for p in range(count):
            acc = acc + used[:, :, p]
        out = acc / np.float32(count)
    return np.where(np.isnan(out), PINF, out).astype(np.float32)


def topk_of_distances(dc, k, idx_offset=0):
    """[Q, N] -> (distances [Q, k] f32 ascending, image indices [Q, k] i64), order (distance asc, image asc)."""
    Q, N = dc.shape
    out_s = np.full((Q, k), PINF, np.float32)
    out_i = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        order = np.lexsort((np.arange(N), dc[q]))
        order = order[dc[q][order] < PINF][:k]                      # +inf images never enter a list
        out_s[q, :len(order)] = dc[q][order]
        out_i[q, :len(order)] = order + idx_offset
    return out_s, out_i


def topk_of_token_distances(a, k, combine, top_t=None, flags=None, idx_offset=0):
    """Top-k from the [Q, N, P] token distances of the WHOLE bank.  flags (bool [N]): the compaction rule -- a token distance
    depends on its own row only, so a[:, flags] is the compacted bank's tensor; indices are mapped back, then offset."""
    if flags is None:
        return topk_of_distances(combine_distances(a, combine, top_t), k, idx_offset)
    flags = np.asarray(flags, dtype=bool)
    assert flags.shape == (a.shape[1],)
    if not flags.any():
        return np.full((a.shape[0], k), PINF, np.float32), np.full((a.shape[0], k), -1, np.int64)
    s, i = topk_of_distances(combine_distances(np.ascontiguousarray(a[:, flags]), combine, top_t), k, 0)
    return tsel._map_back(s, i, flags, idx_offset)


def scores_of_token_distances(a, combine, top_t=None, flags=None):
    """[Q, N] combined distances: those of the compacted bank in the selected columns, +inf in the others."""
    if flags is None:
        return combine_distances(a, combine, top_t)
    flags = np.asarray(flags, dtype=bool)
    out = np.full(a.shape[:2], PINF, np.float32)
    if flags.any():
        out[:, flags] = combine_distances(np.ascontiguousarray(a[:, flags]), combine, top_t)
    return out


def distance_topk_tokens(c, queries, bank, k, metric, combine, top_t=None, flags=None, idx_offset=0):
    """Straight from the bank: with flags the COMPACTED bank is scored (the rule itself, not its shortcut above)."""
    if flags is None:
        return topk_of_token_distances(token_distances(c, queries, bank, metric), k, combine, top_t, None, idx_offset)
    flags = np.asarray(flags, dtype=bool)
    if not flags.any():
        return np.full((np.asarray(queries).shape[0], k), PINF, np.float32), np.full((np.asarray(queries).shape[0], k), -1, np.int64)
    a = token_distances(c, queries, np.ascontiguousarray(np.asarray(bank)[flags]), metric)
    s, i = topk_of_distances(combine_distances(a, combine, top_t), k, 0)
    return tsel._map_back(s, i, flags, idx_offset)
