"""CPU restatement of the patch-token search with per-query feature weights (``weights`` [Q, D] of
sky_embeddings_amd.search.cosine_token_scores / cosine_topk_tokens / cosine_topk, the PQW kernels in csrc/topk_tokens.hip), NumPy
fp32 in the contract's exact operation order.  Used by tests/test_token_pq_gpu.py (bit for bit) and checked on the CPU by
tests/test_token_pq_cpu.py.  Combine, top-t, selection and top-k are those of tests/token_search_reference.py,
tests/token_topt_reference.py and tests/token_select_reference.py; the distance metrics with per-query weights need no
restatement of their own: query q IS tests/token_distance_reference.py with c = row q.

The score of query q (t = queries[q], w = weights[q]) against bank row x, all fp32, fma = one rounding:
    tw[d]  = w[d] * t[d]                                         (one rounding; the oracle's prep_queries)
    dot    = acc = 0; acc = fma(tw[d], x[d], acc)  over d = 0, 1, 2, ...     (the contract's chain, oracle/topk_oracle.c)
    qn     = sqrt(acc), acc = 0; acc = fma(tw[d], t[d], acc)                 (the same chain)
    x2[d]  = x[d] * x[d]                                         (one rounding)
    xn     = sqrt(acc), acc = 0; acc = fma(w[d], x2[d], acc)                 (the same chain with (w, x o x) as operands)
    score  = dot / fma(qn, xn, eps);  NaN -> -inf
Only xn differs from the search with one shared weight vector, whose bank norm is skyemb_weighted_norms' chain
acc = fma(w[d] * x[d], x[d], acc).  A negative acc under the root (negative weights) gives NaN, hence -inf.

The oracle exposes the chain only inside its finished score (``oracle.similarity_oracle.cosine_scores_np``), so ``chain`` below
restates it: NumPy has no fma, ``fma32`` computes one exactly (the product of two fp32 is exact in fp64; the fp64 sum is taken
with its exact error term (TwoSum) and rounded to odd, which makes the second rounding to fp32 the correct single rounding).
tests/test_token_pq_cpu.py pins ``chain`` to the oracle bit for bit by rebuilding ``cosine_scores_np`` from it.

Error bounds, for w >= 0 and eps > 0.  u = 2^-24, gamma(n) = n u / (1 - n u); every fl() is one factor (1 + delta), |delta| <= u;
gamma(a) + gamma(b) + gamma(a) gamma(b) <= gamma(a + b).  T = sqrt(sum w t^2), X = sqrt(sum w x^2) the exact norms,
s* = sum(w t x) / (T X + eps) the exact score: |s*| < 1 by Cauchy-Schwarz.
  * dot: term d carries the rounding of tw and at most D roundings of the chain: |dot - sum w t x| <= gamma(D + 1) sum |w t x|
    <= gamma(D + 1) T X.  The sum may cancel, so this error is absolute, not relative to dot.
  * qn: the terms w t^2 are >= 0, nothing cancels: acc = T^2 (1 + theta), |theta| <= gamma(D + 1); a square root moves the
    relative error no further and rounds once: qn = T (1 + a), |a| <= gamma(D + 2).  xn likewise (x2 takes the place of tw's
    rounding): xn = X (1 + b), |b| <= gamma(D + 2) -- for this chain and for skyemb_weighted_norms' alike.
  * den = fl(qn xn + eps) = (T X + eps)(1 + eta), |eta| <= gamma(2 D + 5) (both summands >= 0, eps exact).
  * score = fl(dot / den):
        |score - s*| <= gamma(D + 1) T X / (T X + eps) (1 + gamma(2 D + 6)) + |s*| gamma(2 D + 6) <= gamma(3 D + 8),  absolute.
  * combine: min, max and order statistics select values (an order statistic of perturbed values moves by no more than the
    largest perturbation); a mean of n scores (n = P, or top_t) adds n roundings on values of magnitude <= 1: gamma(3 D + 8 + n).
``score_bound`` returns that.

Per-query weights with Q identical rows w against the search with the one vector w: tw, dot and qn are the same bits; the two
bank norms are X (1 + b1) and X (1 + b2) with |b1|, |b2| <= gamma(D + 2).  The denominators differ by a factor within
gamma(2 (D + 2) + 2) = gamma(2 D + 6), the quotients by two more roundings:
        |score_pq - score_shared| <= gamma(2 D + 8) |score_shared| <= gamma(2 D + 8) (1 + gamma(3 D + 8)) <= gamma(2 D + 9),  absolute.
A mean of n such scores: each side is within gamma(n) of the exact mean of its own scores, and those two differ by the bound
above: gamma(2 D + 9 + 2 n).  ``shared_bound`` returns that.
"""
import numpy as np

from tests import token_search_reference as tsr
from tests import token_select_reference as tsel
from tests import token_topt_reference as ttr

COMBINES = tsr.COMBINES
NINF = np.float32(-np.inf)
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def score_bound(D, combine="min", count=1):
    """Absolute bound of a combined score against the fp64 formula (the docstring's derivation); count = P or top_t for mean."""
    return gamma(3 * D + 8 + (count if combine == "mean" else 0))


def shared_bound(D, combine="min", count=1):
    """Absolute bound between per-query weights with identical rows and the search with that one shared vector."""
    return gamma(2 * D + 9 + (2 * count if combine == "mean" else 0))


def fma32(a, b, c):
    """fp32 fma(a, b, c) = a * b + c with ONE rounding, elementwise on broadcastable fp32 arrays."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                                   # exact: 24 + 24 bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                             # TwoSum: p + c == s + err exactly
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)   # round to odd: the neighbour on the exact sum's side
        return s.astype(np.float32)


def chain(a, b):
    """a [Q, D], b [R, D] -> [Q, R]: acc = 0; acc = fma(a[q, d], b[r, d], acc) over d = 0, 1, 2, ..."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for d in range(a.shape[1]):
        acc = fma32(a[:, d, None], b[None, :, d], acc)
    return acc


def chain_rows(a, b):
    """a, b [Q, D] -> [Q]: the same chain, row q of a with row q of b."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros(a.shape[0], np.float32)
    for d in range(a.shape[1]):
        acc = fma32(a[:, d], b[:, d], acc)
    return acc


def prepare(queries, weights):
    """(tw [Q, D], qn [Q]) of queries [Q, D] under weights [Q, D]."""
    q, w = np.asarray(queries, np.float32), np.asarray(weights, np.float32)
    assert q.shape == w.shape
    tw = (w * q).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return tw, np.sqrt(chain_rows(tw, q)).astype(np.float32)


def finish(dot, qn, xn, eps):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = (dot / fma32(qn, xn, np.float32(eps))).astype(np.float32)
    return np.where(np.isnan(s), NINF, s).astype(np.float32)


def token_scores_pq(queries, bank, weights, eps=1e-6):
    """[Q, N, P] fp32 token scores, query q under weights[q]."""
    bank = np.ascontiguousarray(bank, dtype=np.float32)
    N, P, D = bank.shape
    x = bank.reshape(N * P, D)
    w = np.asarray(weights, np.float32)
    tw, qn = prepare(queries, w)
    with np.errstate(invalid="ignore", over="ignore"):
        x2 = (x * x).astype(np.float32)
        xn = np.sqrt(chain(w, x2)).astype(np.float32)
    return finish(chain(tw, x), qn[:, None], xn, eps).reshape(-1, N, P)


def token_scores_shared(queries, bank, w, eps=1e-6):
    """tsr.token_scores(queries, bank, w) rebuilt from ``chain``: the oracle's own operation order, bank norm included.  Exists to
    pin ``chain`` / ``fma32`` to the C oracle bit for bit."""
    bank = np.ascontiguousarray(bank, dtype=np.float32)
    N, P, D = bank.shape
    x = bank.reshape(N * P, D)
    q, w = np.asarray(queries, np.float32), np.asarray(w, np.float32)
    tw, qn = prepare(q, np.broadcast_to(w, q.shape))
    with np.errstate(invalid="ignore", over="ignore"):
        xn = np.sqrt(chain_rows((w * x).astype(np.float32), x)).astype(np.float32)
    return finish(chain(tw, x), qn[:, None], xn[None], eps).reshape(-1, N, P)


def exact_token_scores_pq(queries, bank, weights, eps=1e-6):
    """The reference formula (utils/similarity.py:149-172) in fp64 from the same fp32 inputs: [Q, N, P]."""
    x = np.asarray(bank, np.float32).astype(np.float64)
    q, w = np.asarray(queries, np.float32).astype(np.float64), np.asarray(weights, np.float32).astype(np.float64)
    dot = np.einsum("qd,npd->qnp", w * q, x)
    tn = np.sqrt((w * q * q).sum(axis=1))
    xn = np.sqrt(np.einsum("qd,npd->qnp", w, x * x))
    return dot / (tn[:, None, None] * xn + eps)


def combine(s, combine_name, top_t=None):
    """[Q, N, P] token scores -> [Q, N]: the plain (top_t None) or the top-t combine."""
    return tsr.combine_scores(s, combine_name) if top_t is None else ttr.combine_top(s, combine_name, top_t)


def topk_of_token_scores(s, k, combine_name, top_t=None, flags=None, idx_offset=0):
    """Top-k from the [Q, N, P] token scores of the whole bank; flags (bool [N]): the compaction rule of a selection."""
    if flags is None:
        return tsr.topk_of_scores(combine(s, combine_name, top_t), k, idx_offset)
    return tsel.topk_of_token_scores_select(s, k, combine_name, flags, top_t, idx_offset)


def topk_tokens_pq(queries, bank, k, combine_name, weights, top_t=None, flags=None, eps=1e-6, idx_offset=0):
    return topk_of_token_scores(token_scores_pq(queries, bank, weights, eps), k, combine_name, top_t, flags, idx_offset)
