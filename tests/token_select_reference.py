"""CPU restatement of the patch-token search restricted to a selection of images (``select=`` of
sky_embeddings_amd.search.cosine_topk_tokens / cosine_token_scores / cosine_topk, the SEL kernels in csrc/topk_tokens.hip).  Used
by tests/test_token_select_gpu.py (bit for bit) and checked on the CPU by tests/test_token_select_cpu.py.

The one rule: a search with a selection returns exactly what the same search returns over the compacted bank ``bank[flags]``,
every image index mapped back through ``nonzero(flags)`` and then offset by ``idx_offset``.  The mapping is monotone, so the order
(score desc, image asc) carries over.  The searches themselves are tests/token_search_reference.py's (all tokens) and
tests/token_topt_reference.py's (``top_t``).  ``cosine_token_scores`` writes every [Q, N] slot: -inf for a deselected image.

Packed words (what the kernels read, what skyemb_pack_select writes): bit ``i & 31`` of 32-bit word ``i >> 5`` is image i;
``ceil(N / 32)`` words; the padding bits of the last word are zero.
"""
import numpy as np

from tests import token_search_reference as tsr
from tests import token_topt_reference as ttr

NINF = np.float32(-np.inf)


def pack_words(flags):
    """bool [N] -> uint32 [ceil(N / 32)]."""
    flags = np.asarray(flags, dtype=bool)
    N = flags.shape[0]
    words = np.zeros((N + 31) // 32, np.uint32)
    for i in np.nonzero(flags)[0]:
        words[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words


def unpack_words(words, N):
    """uint32 [ceil(N / 32)] -> bool [N]."""
    i = np.arange(N)
    return ((np.asarray(words, np.uint32)[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)


def _map_back(s, i, flags, idx_offset):
    where = np.nonzero(np.asarray(flags, dtype=bool))[0].astype(np.int64)
    out = np.full(i.shape, -1, np.int64)
    ok = i >= 0
    out[ok] = where[i[ok]] + idx_offset
    return s, out


def _empty(Q, k):
    return np.full((Q, k), NINF, np.float32), np.full((Q, k), -1, np.int64)


def topk_tokens_select(queries, bank, k, combine, flags, top_t=None, weights=None, eps=1e-6, idx_offset=0):
    """The compaction rule on top of tsr.topk_tokens / ttr.topk_tokens_top: (scores [Q, k] f32, images [Q, k] i64)."""
    flags = np.asarray(flags, dtype=bool)
    assert flags.shape == (bank.shape[0],)
    if not flags.any():
        return _empty(np.asarray(queries).shape[0], k)
    compact = np.ascontiguousarray(bank[flags])
    if top_t is None:
        s, i = tsr.topk_tokens(queries, compact, k, combine, weights, eps, 0)
    else:
        s, i = ttr.topk_tokens_top(queries, compact, k, combine, top_t, weights, eps, 0)
    return _map_back(s, i, flags, idx_offset)


def combine(s, combine_name, top_t=None):
    """[Q, n, P] token scores -> [Q, n] in the documented order of the plain (top_t None) or the top-t combine."""
    return tsr.combine_scores(s, combine_name) if top_t is None else ttr.combine_top(s, combine_name, top_t)


def topk_of_token_scores_select(s, k, combine_name, flags, top_t=None, idx_offset=0):
    """The same rule from the [Q, N, P] token scores of the WHOLE bank: a token score depends on its own bank row only, so
    ``s[:, flags]`` is bit for bit the token-score tensor of the compacted bank (test_token_select_cpu.py checks that); combine
    and top-k then run on the compacted tensor.  Lets many selections of one bank share one pass of the fma chain."""
    flags = np.asarray(flags, dtype=bool)
    assert flags.shape == (s.shape[1],)
    if not flags.any():
        return _empty(s.shape[0], k)
    sc = combine(np.ascontiguousarray(s[:, flags]), combine_name, top_t)
    return _map_back(*tsr.topk_of_scores(sc, k, 0), flags, idx_offset)


def scores_of_token_scores_select(s, combine_name, flags, top_t=None):
    """[Q, N] combined scores: those of the compacted bank in the selected columns, -inf in the others."""
    flags = np.asarray(flags, dtype=bool)
    out = np.full(s.shape[:2], NINF, np.float32)
    if flags.any():
        out[:, flags] = combine(np.ascontiguousarray(s[:, flags]), combine_name, top_t)
    return out


def token_scores_select(queries, bank, combine_name, flags, top_t=None, weights=None, eps=1e-6):
    """[Q, N] combined scores from the bank: the compacted bank is scored, deselected images get -inf."""
    flags = np.asarray(flags, dtype=bool)
    out = np.full((np.asarray(queries).shape[0], bank.shape[0]), NINF, np.float32)
    if flags.any():
        out[:, flags] = combine(tsr.token_scores(queries, np.ascontiguousarray(bank[flags]), weights, eps), combine_name, top_t)
    return out
