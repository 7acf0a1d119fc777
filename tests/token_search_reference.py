"""CPU restatement of the patch-token search (sky_embeddings_amd.search.cosine_token_scores / cosine_topk_tokens, kernels in
csrc/topk_tokens.hip).  Used by tests/test_token_search_gpu.py (bit for bit) and pinned on the CPU against the reference goldens
by tests/test_token_search_cpu.py.

bank [N, P, D] -> token scores: ``oracle.similarity_oracle.cosine_scores_np`` on the [N * P, D] view (the bit-exact contract of
oracle/topk_oracle.c: fp32 fma chain over d = 0, 1, 2, ..., NaN -> -inf).  Combine per (query, image) in NumPy fp32:

  min / max   exact (a -inf token gives -inf for min and is ignored by max);
  mean        acc = 0; for p = 0 .. P-1: acc = acc + s[p]   (token order, one fp32 rounding per add);  acc / float32(P), one IEEE
              division; a NaN result (only +inf and -inf tokens in one image) ranks as -inf like any NaN score.

top-k: lexsort on (-score, image index); images whose combined score is -inf are not returned, missing entries are (-inf, -1).
"""
import numpy as np

from oracle import similarity_oracle as so

COMBINES = ("min", "mean", "max")


def token_scores(queries, bank, weights=None, eps=1e-6):
    """[Q, N, P] fp32 token scores."""
    bank = np.ascontiguousarray(bank, dtype=np.float32)
    N, P, D = bank.shape
    s = so.cosine_scores_np(queries, bank.reshape(N * P, D), weights, eps)
    s = np.where(np.isnan(s), np.float32(-np.inf), s).astype(np.float32)
    return s.reshape(-1, N, P)


def combine_scores(s, combine):
    """[Q, N, P] -> [Q, N] in the documented order."""
    assert s.dtype == np.float32
    if combine == "min":
        return s.min(axis=2)
    if combine == "max":
        return s.max(axis=2)
    assert combine == "mean"
    acc = np.zeros(s.shape[:2], np.float32)
    with np.errstate(invalid="ignore"):
        for p in range(s.shape[2]):
            acc = (acc + s[:, :, p]).astype(np.float32)
        out = (acc / np.float32(s.shape[2])).astype(np.float32)
    return np.where(np.isnan(out), np.float32(-np.inf), out).astype(np.float32)


def combined_scores(queries, bank, combine, weights=None, eps=1e-6):
    return combine_scores(token_scores(queries, bank, weights, eps), combine)


def topk_of_scores(sc, k, idx_offset=0):
    """[Q, N] -> (scores [Q, k] f32, image indices [Q, k] i64), order (score desc, index asc)."""
    Q, N = sc.shape
    out_s = np.full((Q, k), -np.inf, np.float32)
    out_i = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        order = np.lexsort((np.arange(N), -sc[q]))
        order = order[np.isfinite(sc[q][order]) | (sc[q][order] > 0)][:k]     # -inf images never enter a list
        out_s[q, :len(order)] = sc[q][order]
        out_i[q, :len(order)] = order + idx_offset
    return out_s, out_i


def topk_tokens(queries, bank, k, combine, weights=None, eps=1e-6, idx_offset=0):
    return topk_of_scores(combined_scores(queries, bank, combine, weights, eps), k, idx_offset)
