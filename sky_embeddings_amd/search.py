"""Batched weighted-cosine top-k over an embedding bank resident in HBM.

Build-level formulation of the reference search (utils/similarity.py: one mean target vector +
inverse-variance weights scored against streamed batches, best ``n_save`` kept by cat+argsort):
``cosine_topk(queries[Q,D], bank[N,D], k, weights)`` returns the exact top-k (score desc, index
asc) per query; Q = 1 with ``weights`` reproduces ``compute_similarity(metric='cosine')`` +
``update_best_scores``.  Multi-GPU: the bank is sharded by rows (one process per GPU), every rank
scores its shard, the per-rank [Q,k] results are all-gathered over RCCL and merged with the same
order, so the result is identical to the single-GPU one.
"""
from __future__ import annotations

import torch

from . import ops


class PreparedBank:
    """Bank rows + their weighted norms (recomputed only when the weights change)."""

    def __init__(self, bank: torch.Tensor, weights: torch.Tensor | None = None, idx_offset: int = 0):
        assert bank.is_cuda and bank.dtype == torch.float32 and bank.is_contiguous() and bank.dim() == 2
        self.bank, self.idx_offset = bank, int(idx_offset)
        self.norms = torch.empty(bank.shape[0], device=bank.device)
        self._sample = None
        self._half = None
        self.set_weights(weights)

    def set_weights(self, weights):
        self.weights = None if weights is None else weights.to(self.bank.device, torch.float32).contiguous()
        ops.weighted_norms(self.bank, self.weights, self.norms)
        self._sample = None
        self._half = None

    def half_image(self):
        """(bank16, rowp): the fp16 image + per-row constants the prefiltered many-query search runs on; built on first
        use (one pass over the bank, +50 % bank memory) and kept until the weights change."""
        if self._half is None:
            self._half = ops.bank16_prepare(self.bank, self.norms)
        return self._half

    def sample(self, rows: int):
        """A strided row sample (bank rows + norms) used to derive the pruning floor of a search."""
        N = self.bank.shape[0]
        rows = min(rows, N)
        if self._sample is None or self._sample[0].shape[0] != rows:
            idx = torch.arange(rows, device=self.bank.device) * (N // rows)
            self._sample = (self.bank.index_select(0, idx).contiguous(), self.norms.index_select(0, idx).contiguous())
        return self._sample


def standardise_(bank: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, out: torch.Tensor | None = None):
    """(x - mean) / (std + 1e-8) row-wise (utils/similarity.py:101-102); in place by default."""
    out = bank if out is None else out
    ops.standardise(bank, mean.contiguous(), std.contiguous(), out)
    return out


def standardise_to(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, dtype: torch.dtype):
    """(x - mean) / (std + 1e-8) of fp32 rows ``x`` [..., D], rounded ONCE to nearest-even into a new ``dtype`` tensor
    (torch.float16 or torch.bfloat16): ``standardise_``'s value, then the storage rounding of a half-precision bank (fp16:
    overflow -> +-inf, subnormals kept; NaN stays NaN).  Lets a 16-bit bank be built batch by batch."""
    if dtype not in ops.LP_DTYPES:
        raise ValueError(f"standardise_to: dtype {dtype} is not supported, expected torch.float16 or torch.bfloat16")
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=dtype)
    D = x.shape[-1]
    ops.standardise_lp(x.view(-1, D), mean.to(x.device, torch.float32).contiguous(), std.to(x.device, torch.float32).contiguous(),
                       out.view(-1, D))
    return out


def prepare_queries(queries: torch.Tensor, weights: torch.Tensor | None):
    Q, D = queries.shape
    tw = torch.empty(Q, D, device=queries.device)
    qn = torch.empty(Q, device=queries.device)
    ops.weighted_norms(queries.contiguous(), weights, qn, tw)
    return tw, qn


def _local_topk(tw, qn, bank, norms, k, eps, idx_offset, thr0=None):
    Q, D = tw.shape
    N = bank.shape[0]
    dev = tw.device
    nch = ops.cosine_topk_chunks(N, Q, D, k)
    ps = torch.empty(Q, nch, k, device=dev)
    pi = torch.empty(Q, nch, k, device=dev, dtype=torch.int64)
    ops.cosine_topk(tw, qn, bank, norms, k, eps, idx_offset, nch, ps, pi, thr0)
    out_s = torch.empty(Q, k, device=dev)
    out_i = torch.empty(Q, k, device=dev, dtype=torch.int64)
    ops.topk_merge(ps, pi, Q, nch, k, out_s, out_i, torch.empty(Q, device=dev, dtype=torch.int32))
    return out_s, out_i


def pruning_floor(tw, qn, pb: "PreparedBank", k: int, eps: float, sample_rows: int | None = None):
    """Per-query score floor for the main pass: the k-th best score over a row SAMPLE is a lower
    bound of the k-th best over the whole bank, so rows scoring below it can never enter the
    result.  Returned one ulp lower (the kernels keep rows STRICTLY above the floor, ties included
    this way).  None when the bank is too small for the extra pass to pay."""
    N = pb.bank.shape[0]
    if sample_rows is None:
        sample_rows = 256 * k
    if N < 8 * sample_rows:
        return None
    sb, sn = pb.sample(sample_rows)
    if ops.sample_floor_applicable(tw.shape[0], sb.shape[0], tw.shape[1], k, tw, sb):
        # Q <= 16: tile maxima of the sample scores + a one-wave selection (two short launches, no [Q, sample] matrix)
        floor = torch.empty(tw.shape[0], device=tw.device)
        ws = torch.empty(tw.shape[0] * ((sb.shape[0] + 15) // 16), device=tw.device)
        ops.cosine_sample_floor(tw, qn, sb, sn, k, eps, ws, floor)
        return floor
    sc = torch.empty(tw.shape[0], sb.shape[0], device=tw.device)
    ops.cosine_scores(tw, qn, sb, sn, eps, sc)          # [Q, sample] score matrix (small)
    floor = torch.empty(tw.shape[0], device=tw.device)
    ops.kth_largest_floor(sc, k, floor)                 # k-th best of the sample, one ulp lower (radix select, one launch)
    return floor


def _prefilter_enabled():
    import os
    return os.environ.get("SKYEMB_TOPK_PREFILTER", "1") != "0"


def _local_topk_prefiltered(tw, qn, pb: "PreparedBank", k, eps):
    """Two-stage exact top-k of this rank's shard (csrc/topk_prefilter.hip); queries the second stage could not certify
    (redo flags) go through the exact fp32 kernel."""
    Q = tw.shape[0]
    dev = tw.device
    bank16, rowp = pb.half_image()
    out_s = torch.empty(Q, k, device=dev)
    out_i = torch.empty(Q, k, device=dev, dtype=torch.int64)
    redo = torch.empty(Q, device=dev, dtype=torch.int32)
    ops.cosine_topk_prefiltered(tw, qn, pb.bank, pb.norms, bank16, rowp, k, eps, pb.idx_offset, out_s, out_i, redo)
    again = torch.nonzero(redo).squeeze(1)                 # host sync: a handful of bytes per search
    if again.numel():
        tw2, qn2 = tw.index_select(0, again).contiguous(), qn.index_select(0, again).contiguous()
        thr0 = pruning_floor(tw2, qn2, pb, k, eps)
        s2, i2 = _local_topk(tw2, qn2, pb.bank, pb.norms, k, eps, pb.idx_offset, thr0)
        out_s.index_copy_(0, again, s2)
        out_i.index_copy_(0, again, i2)
    return out_s, out_i, int(again.numel())


def cosine_topk(queries: torch.Tensor, bank, k: int, weights: torch.Tensor | None = None, eps: float = 1e-6,
                process_group=None, world_size: int = 1, prune: bool = True, stats: dict | None = None, select=None):
    """-> (scores f32 [Q,k], indices i64 [Q,k]).  ``bank`` is a [N,D] tensor or a PreparedBank
    (this rank's shard; ``idx_offset`` = first global row of the shard).  More than 16 queries take the two-stage
    path (fp16 matrix-core prefilter with a proven error bound, exact fp32 re-score of the survivors: same results bit
    for bit); SKYEMB_TOPK_PREFILTER=0 keeps every search on the exact fp32 kernels.

    A 2-D fp16 / bf16 tensor is a half-precision resident bank: it is served as a token bank with one token per row
    (``cosine_topk_tokens`` on ``bank.unsqueeze(1)``, ``stats['path'] == 'tokens'``) under that search's limits -- k <= 512,
    more than 16 queries in groups of 16 -- with the results of the fp32 search on the widened bank, bit for bit.  The
    many-query prefilter over a 16-bit flat bank is out of scope.  fp32 banks take exactly the paths described above.

    ``select`` (None: nothing above changes; a bool tensor [N] or a ``Selection``): only the rows marked True are eligible, with
    the result of the search over the compacted bank and indices mapped back (``cosine_topk_tokens``'s ``select``).  A flat
    [N,D] bank of any dtype is then served as a token bank with one token per row (``stats['path'] == 'tokens'``) under that
    search's limits: k <= 512, D % 64 == 0, D <= 1024, queries in groups of 16.  A PreparedBank with ``select`` is a ValueError:
    its many-query prefilter under a selection is out of scope.

    ``weights`` [Q, D] (one row per query; [D] or None: nothing above changes): a flat [N,D] bank is served the same way, as
    ``cosine_topk_tokens`` with per-query weights and one token per row (``stats['path'] == 'tokens'``); a PreparedBank is a
    ValueError."""
    if isinstance(weights, torch.Tensor) and weights.dim() == 2:      # per-query weights: the token search with one token per row
        if not (isinstance(bank, torch.Tensor) and bank.dim() == 2):
            raise ValueError("cosine_topk: per-query weights [Q, D] are served by the token search (cosine_topk_tokens with one "
                             "token per row); pass the flat [N, D] tensor, not a PreparedBank")
        return cosine_topk_tokens(queries, bank.unsqueeze(1), k, 'min', weights, eps, process_group, world_size, prune, stats,
                                  select=select)
    if select is not None:
        if isinstance(bank, PreparedBank):
            raise ValueError("cosine_topk: select is served by the token search (cosine_topk_tokens with one token per row); pass "
                             "the flat [N, D] tensor, not a PreparedBank -- the prefiltered many-query route takes no selection")
        if not (isinstance(bank, torch.Tensor) and bank.dim() == 2):
            raise ValueError("cosine_topk: select needs a flat [N, D] bank tensor")
        return cosine_topk_tokens(queries, bank.unsqueeze(1), k, 'min', weights, eps, process_group, world_size, prune, stats,
                                  select=select)
    if isinstance(bank, torch.Tensor) and bank.dim() == 2 and bank.dtype in ops.LP_DTYPES:
        return cosine_topk_tokens(queries, bank.unsqueeze(1), k, 'min', weights, eps, process_group, world_size, prune, stats)
    pb = bank if isinstance(bank, PreparedBank) else PreparedBank(bank, weights)
    q = queries.to(pb.bank.device, torch.float32).contiguous()
    Q, D = q.shape
    N = pb.bank.shape[0]
    assert D == pb.bank.shape[1]
    if k < 1:
        raise ValueError(f"cosine_topk: k = {k}")
    if world_size == 1 and k > N:
        raise ValueError(f"cosine_topk: k = {k} exceeds the {N} rows of the bank")
    if Q == 0:                                      # nothing to search for (an empty target list): empty result, no launch
        return (torch.empty(0, k, device=q.device), torch.empty(0, k, device=q.device, dtype=torch.int64))
    tw, qn = prepare_queries(q, pb.weights)
    if _prefilter_enabled() and ops.topk_prefilter_applicable(Q, N, D, k):
        out_s, out_i, n_redo = _local_topk_prefiltered(tw, qn, pb, k, eps)
        if stats is not None:
            stats.update(path="prefiltered", redone=n_redo)
    else:
        thr0 = pruning_floor(tw, qn, pb, k, eps) if prune else None
        out_s, out_i = _local_topk(tw, qn, pb.bank, pb.norms, k, eps, pb.idx_offset, thr0)
        if stats is not None:
            stats.update(path="exact", redone=0)
    if world_size > 1:
        from .distributed import gather_topk
        gs, gi = gather_topk(out_s, out_i, world_size, process_group)   # RCCL all-gather -> [Q, world, k]
        ops.topk_merge(gs, gi, Q, world_size, k, out_s, out_i)
    return out_s, out_i


def cosine_scores(queries: torch.Tensor, bank, weights: torch.Tensor | None = None, eps: float = 1e-6):
    """Plain [Q,N] score matrix (reference-shaped path with several patches per sample)."""
    pb = bank if isinstance(bank, PreparedBank) else PreparedBank(bank, weights)
    q = queries.to(pb.bank.device, torch.float32).contiguous()
    tw, qn = prepare_queries(q, pb.weights)
    out = torch.empty(q.shape[0], pb.bank.shape[0], device=q.device)
    ops.cosine_scores(tw, qn, pb.bank, pb.norms, eps, out)
    return out


# ------------------------------------------------------------------------------------------------
# patch-token banks: P tokens per image, scored token by token and combined per image (min | mean | max)
# ------------------------------------------------------------------------------------------------
class TokenBank:
    """Patch tokens [N, P, D] of N images + the weighted norms of the N * P rows (recomputed only when the weights change).

    ``bank`` is fp32, or fp16 / bf16 for a half-precision resident bank (``dtype``): such a bank IS the fp32 bank its elements
    widen to -- norms (fp32) and scores are those of the widened bank bit for bit, for half the memory and half the bytes per
    pass.  The only approximation is the rounding when the bank was stored (``standardise_to``)."""

    def __init__(self, bank: torch.Tensor, weights: torch.Tensor | None = None, idx_offset: int = 0):
        ops.bank_dtype_code(bank.dtype, "TokenBank")          # ValueError for anything but fp32 / fp16 / bf16
        assert bank.is_cuda and bank.is_contiguous() and bank.dim() == 3
        self.bank, self.idx_offset, self.dtype = bank, int(idx_offset), bank.dtype
        self.norms = torch.empty(bank.shape[0] * bank.shape[1], device=bank.device)
        self._sample = None
        self._version = 0                                  # counts set_weights calls: what depends on the norms checks it
        self.set_weights(weights)

    def set_weights(self, weights):
        self._version += 1
        self.weights = None if weights is None else weights.to(self.bank.device, torch.float32).contiguous()
        rows = self.bank.view(-1, self.bank.shape[2])
        if self.dtype == torch.float32:
            ops.weighted_norms(rows, self.weights, self.norms)
        else:
            ops.weighted_norms_lp(rows, self.weights, self.norms)
        self._sample = None

    def sample(self, images: int):
        """A strided sample of WHOLE images (tokens [S, P, D] in the bank's dtype + the norms of their S * P rows) used to
        derive the pruning floor of a search."""
        N, P, _ = self.bank.shape
        images = min(images, N)
        if self._sample is None or self._sample[0].shape[0] != images:
            idx = torch.arange(images, device=self.bank.device) * (N // images)
            self._sample = (self.bank.index_select(0, idx).contiguous(),
                            self.norms.view(N, P).index_select(0, idx).contiguous().view(-1))
        return self._sample


class Selection:
    """A selection of a bank's images: ``flags`` is a bool tensor [N] (host or device), True = eligible.  Holds the packed words
    the kernels read (``words`` i32 [ceil(N / 32)] on the device: bit i & 31 of word i >> 5 is image i, padding bits zero), ``N``
    and the selected ``count``; packed once (one short launch), reusable across searches and banks of N images.  A search with a
    selection returns what the same search returns over the compacted bank ``bank[flags]``, image indices mapped back."""

    def __init__(self, flags: torch.Tensor, device=None):
        if not isinstance(flags, torch.Tensor) or flags.dtype != torch.bool or flags.dim() != 1:
            what = f"{tuple(flags.shape)} {flags.dtype}" if isinstance(flags, torch.Tensor) else type(flags).__name__
            raise ValueError(f"Selection: flags must be a bool tensor with one dimension [N], got {what}")
        if not flags.is_cuda:                              # host flags: packed on ``device`` (default: the current GPU)
            flags = flags.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
        self.flags = flags.contiguous()
        self.N = int(flags.shape[0])
        self.words = torch.empty((self.N + 31) // 32, device=flags.device, dtype=torch.int32)
        if self.N:
            ops.pack_select(self.flags.view(torch.uint8), self.words)
        self.count = int(self.flags.sum())
        self._indices = None
        self._sample = None                                # bank -> (its weights version, images, the floor's sample)

    def sample(self, tb: "TokenBank", images: int):
        """A strided sample of ``images`` SELECTED whole images of ``tb`` (tokens + the norms of their rows) for the pruning floor.
        Kept here, with the selection it belongs to -- not in the bank -- until the bank, its weights or the size change, so
        that repeated searches under one Selection do not gather it again."""
        import weakref
        if self._sample is None:
            self._sample = weakref.WeakKeyDictionary()     # one entry per bank: a Selection may serve several (fp32 and fp16)
        got = self._sample.get(tb)
        if got is None or got[0] != tb._version or got[1] != images:
            N, P = tb.bank.shape[0], tb.bank.shape[1]
            idx = self.indices()[torch.arange(images, device=tb.bank.device) * (self.count // images)]
            got = (tb._version, images, tb.bank.index_select(0, idx), tb.norms.view(N, P).index_select(0, idx).view(-1))
            self._sample[tb] = got
        return got[2], got[3]

    def indices(self):
        """The selected images, ascending (i64 on the device): compacted position -> image."""
        if self._indices is None:
            self._indices = torch.nonzero(self.flags).squeeze(1)
        return self._indices


def _selection_arg(select, N, who, device=None):
    """``select`` (None | bool tensor [N] | Selection) -> None | Selection; ValueError unless it describes N images.  ``device``:
    the bank's, when it lives on a GPU -- flags are packed there, and a Selection packed on another device is a ValueError (its
    words would reach the kernel as a pointer into the wrong device's memory)."""
    if select is None:
        return None
    n = select.N if isinstance(select, Selection) else (select.shape[0] if isinstance(select, torch.Tensor) and select.dim() == 1 else None)
    if n is not None and n != N:
        raise ValueError(f"{who}: select describes {n} images, the bank has {N}")
    if device is not None and device.type != "cuda":
        device = None
    if not isinstance(select, Selection):
        if device is not None and isinstance(select, torch.Tensor) and select.is_cuda and select.device != device:
            raise ValueError(f"{who}: select is on {select.device}, the bank on {device}")
        return Selection(select, device)
    if device is not None and select.words.device != device:
        raise ValueError(f"{who}: the Selection was packed on {select.words.device}, the bank is on {device}: build it with "
                         f"Selection(flags, device=bank.device)")
    return select


def _combine_code(combine, who):
    if combine not in ops.COMBINE_CODES:
        raise ValueError(f"{who}: combine = {combine!r}, expected one of {sorted(ops.COMBINE_CODES)}")
    return ops.COMBINE_CODES[combine]


def _top_t_arg(top_t, P, who):
    """``top_t`` (None: all tokens) -> the library's argument (0: all tokens); ValueError outside 1 .. min(P, 16)."""
    if top_t is None:
        return 0
    if isinstance(top_t, bool) or int(top_t) != top_t or not 1 <= top_t <= min(P, 16):
        raise ValueError(f"{who}: top_t = {top_t!r}, expected None (all tokens) or an integer 1 .. min(P, 16) = {min(P, 16)} (P = {P})")
    return int(top_t)


def _weights_arg(weights, Q, D, who, ignored=False):
    """``weights`` (None | [D] | [Q, D]) -> None for shared weights (None or [D]: the calls as they ever were) or the [Q, D]
    tensor of per-query weights; ValueError naming both shapes for any other rank, leading dimension or D.  ``ignored``: the bank
    is a TokenBank, which carries its own weights -- the argument is then looked at only when it is [Q, D], and anything else is
    passed over unchecked, as it always was."""
    if weights is None:
        return None
    shape = tuple(weights.shape) if isinstance(weights, torch.Tensor) else None
    if ignored and shape != (Q, D):
        return None
    if shape not in ((D,), (Q, D)):
        raise ValueError(f"{who}: weights has shape {shape if shape is not None else type(weights).__name__}, expected ({D},) -- one "
                         f"vector for all queries -- or ({Q}, {D}) -- one row per query -- for queries of shape ({Q}, {D})")
    return weights if len(shape) == 2 else None


def _pq_group(who, P, D, k):
    """Queries per pass with per-query weights: the largest g <= 16 the library takes (two operand images in LDS:
    128 D + 32 g k <= 163840); ValueError with the library's text when not even one query fits."""
    for g in range(16, 0, -1):
        why = ops.cosine_token_pq_refusal(g, P, D, k)
        if why is None:
            return g
    raise ValueError(f"{who}: {why}")


def prepare_queries_pq(queries: torch.Tensor, weights: torch.Tensor):
    """``prepare_queries`` with one weight row per query: query q is prepared by the same call with its own row, so tw[q] and
    qn[q] are bit-equal to what the single-query search prepares."""
    Q, D = queries.shape
    tw = torch.empty(Q, D, device=queries.device)
    qn = torch.empty(Q, device=queries.device)
    for i in range(Q):
        ops.weighted_norms(queries[i:i + 1], weights[i], qn[i:i + 1], tw[i:i + 1])
    return tw, qn


def _token_scores(tw, qn, tokens, norms, code, eps, top_t=0, words=None):
    """[Q, N] combined scores of Q <= 16 prepared queries (words: a Selection's, deselected images score -inf)."""
    out = torch.empty(tw.shape[0], tokens.shape[0], device=tw.device)
    ops.cosine_token_scores(tw, qn, tokens, norms, code, eps, out, top_t, words)
    return out


def token_pruning_floor(tw, qn, tb, k: int, combine: str = 'min', eps: float = 1e-6, sample_images: int | None = None,
                        top_t: int | None = None, select=None, weights=None):
    """Per-query floor for the token search: the k-th best COMBINED score over a sample of whole images, one ulp lower
    (``pruning_floor``'s argument, with images for rows).  None under the same size rule: N < 8 x the sample.  ``top_t``: the
    search's own, so that the sample is scored as the search scores it and the floor stays a lower bound of its k-th best.
    ``select`` (None | bool tensor | Selection): the sample is drawn from the selected images only, strided over them, so the
    floor is a lower bound of the k-th best SELECTED score; the size rule applies to the selected count.  That sample changes
    with the selection, so it is not kept in the bank (``TokenBank._sample``): a ``Selection`` keeps its own (``Selection.sample``),
    a bool tensor is packed and sampled anew on every call.
    ``weights`` [Q, D] (per-query weights, rows for the Q <= 16 queries of ``tw``; None: the floor above, ``tb`` a TokenBank): the
    same sample -- ``tb`` may then be a plain [N,P,D] tensor, no norms are needed -- is scored by the kernel with per-query
    weights, as the search scores it."""
    tokens = tb.bank if isinstance(tb, TokenBank) else tb
    t = _top_t_arg(top_t, tokens.shape[1], "token_pruning_floor")
    N, P = tokens.shape[0], tokens.shape[1]
    W = _weights_arg(weights, tw.shape[0], tw.shape[1], "token_pruning_floor")
    sel = _selection_arg(select, N, "token_pruning_floor", tokens.device)
    if sample_images is None:
        sample_images = 256 * k
    if (N if sel is None else sel.count) < 8 * sample_images:
        return None
    if W is not None:
        W = W.to(tw.device, torch.float32).contiguous()
        st = _distance_sample(tb, sel, sample_images)
        sc = torch.empty(tw.shape[0], st.shape[0], device=tw.device)
        ops.cosine_token_scores_pq(tw, qn, st, W, _combine_code(combine, "token_pruning_floor"), eps, sc, t)
        floor = torch.empty(tw.shape[0], device=tw.device)
        ops.kth_largest_floor(sc, k, floor)
        return floor
    if sel is None:
        st, sn = tb.sample(sample_images)
    else:
        st, sn = sel.sample(tb, sample_images)
    sc = _token_scores(tw, qn, st, sn, _combine_code(combine, "token_pruning_floor"), eps, t)
    floor = torch.empty(tw.shape[0], device=tw.device)
    ops.kth_largest_floor(sc, k, floor)
    return floor


def _check_token_shape(who, Q, P, D, k):
    why = ops.cosine_token_refusal(max(1, min(Q, 16)), P, D, k)       # Q: queries per launch
    if why is not None:
        raise ValueError(f"{who}: {why}")


def cosine_topk_tokens(queries: torch.Tensor, bank, k: int, combine: str = 'min', weights: torch.Tensor | None = None,
                       eps: float = 1e-6, process_group=None, world_size: int = 1, prune: bool = True, stats: dict | None = None,
                       top_t: int | None = None, select=None):
    """-> (scores f32 [Q,k], image indices i64 [Q,k]): exact top-k images by the combined score of their P patch tokens
    (reference: compute_similarity with max_pool = False, utils/similarity.py:214-268, + update_best_scores), order
    (score desc, image asc).  ``bank`` is a [N,P,D] tensor (fp32, or fp16 / bf16: see TokenBank) or a TokenBank (this rank's
    shard of images; ``idx_offset`` = first global image of the shard).  One pass over the bank per group of at most 16 queries (Q > 16 runs ceil(Q / 16) passes: a
    many-query prefilter for token banks is out of scope).  Images whose combined score is -inf (a NaN token under min / mean)
    are never returned; missing entries are (-inf, -1).  ``weights`` is used only when ``bank`` is a plain tensor: a TokenBank
    carries its own (``TokenBank.set_weights``), and the argument is then ignored, as ``cosine_topk`` does with a PreparedBank.

    ``top_t`` (the reference's ``n_top_sims``; None: all tokens, the search above unchanged): an integer 1 .. min(P, 16); only
    the top_t best token scores of an image count.  With d[0] >= d[1] >= ... the image's scores in descending order (-inf, which
    a NaN score ranks as, last -- torch.topk would rank NaN largest): max is d[0] (unchanged), min is d[top_t-1], mean is
    (((0 + d[0]) + d[1]) + ... + d[top_t-1]) / float32(top_t), summed largest first.  ``top_t == P`` with 'min' is the plain min
    bit for bit; with 'mean' it is NOT the plain mean, which sums in token order.  An image with fewer than top_t scores above
    -inf scores -inf under min and mean and is never returned.  ValueError outside the range, before the first launch.

    ``select`` (None: every image, the search above unchanged; a bool tensor [N] or a ``Selection``): only the images marked
    True are eligible.  The result is exactly that of the same search over the compacted bank ``bank[select]`` -- scores bit for
    bit, order (score desc, image asc) -- with every index mapped back to this bank (then offset by ``idx_offset``).  The bank is
    not copied, deselected images cost no HBM bytes when P is a multiple of 16 (P < 16: a 16-row tile is passed over when all
    of its 16 / P images are deselected) and a NaN or inf in them changes nothing.  Fewer than k selected images: the tail is
    (-inf, -1).  One selection serves all queries; with ``world_size > 1`` it describes this rank's shard.  A length other than
    N is a ValueError before any launch; ``stats`` gains ``selected``.

    ``weights`` [Q, D] (per-query weights, one row per query -- the reference derives the weights from the target, so two targets
    never share them; [D] or None: the search above, same kernels, same bits): query q is scored under its own row, also when
    ``bank`` is a TokenBank, whose own weights and norms are then neither used nor touched.  Query preparation is the
    single-query one, row by row (tw[q], qn[q] bit-equal to a Q = 1 search with that row); the norm of a bank row under query q's
    weights is computed inside the pass as the fma chain acc = fma(w_q[d], x[d] * x[d], acc) over d = 0, 1, 2, ... (x * x
    rounded once), then one IEEE square root -- no norm pass over the bank, no norm array.  That is not ``TokenBank``'s order,
    so the search with one shared vector and this one with Q identical rows may differ in the last bits of a score; a 16-bit
    bank still gives the fp32 result on the widened bank bit for bit, and row q of the result is bit for bit the Q = 1 search
    with query q and its row.  An all-zero row scores every token 0; a negative sum under the root or a NaN weight gives -inf
    (never returned).  Queries run in groups of the largest g <= 16 with 128 D + 32 g k <= 163840 (two operand images in LDS;
    D = 768, k = 300: six per pass), weights sliced along; ValueError with the library's text when g = 1 does not fit, and, naming
    both shapes, for weights of any other rank, leading dimension or D.  ``stats['per_query_weights']`` is True and
    ``stats['group']`` is g."""
    who = "cosine_topk_tokens"
    tokens = bank.bank if isinstance(bank, TokenBank) else bank
    Q, D = queries.shape
    N, P = tokens.shape[0], tokens.shape[1]
    assert tokens.dim() == 3 and D == tokens.shape[2]
    code = _combine_code(combine, who)
    t = _top_t_arg(top_t, P, who)
    if k < 1:
        raise ValueError(f"{who}: k = {k}")
    if world_size == 1 and k > N:
        raise ValueError(f"{who}: k = {k} exceeds the {N} images of the bank")
    W = _weights_arg(weights, Q, D, who, isinstance(bank, TokenBank))
    if W is None:
        _check_token_shape(who, Q, P, D, k)                  # every refusal above and here: before the first launch
        step = 16
    else:
        ops.bank_dtype_code(tokens.dtype, who)
        step = _pq_group(who, P, D, k)
    sel = _selection_arg(select, N, who, tokens.device)
    words = None if sel is None else sel.words
    if W is None:
        tb = bank if isinstance(bank, TokenBank) else TokenBank(bank, weights)
        idx_offset = tb.idx_offset
    else:                                           # no TokenBank is built: its norm pass is what these weights make useless
        tb = bank
        idx_offset = bank.idx_offset if isinstance(bank, TokenBank) else 0
        W = W.to(tokens.device, torch.float32).contiguous()
    q = queries.to(tokens.device, torch.float32).contiguous()
    out_s = torch.empty(Q, k, device=q.device)
    out_i = torch.empty(Q, k, device=q.device, dtype=torch.int64)
    if Q == 0:                                      # nothing to search for: empty result, no launch
        return out_s, out_i
    tw_all, qn_all = prepare_queries(q, tb.weights) if W is None else prepare_queries_pq(q, W)
    pruned = False
    for lo in range(0, Q, step):
        tw, qn = tw_all[lo:lo + step], qn_all[lo:lo + step]
        Wg = None if W is None else W[lo:lo + step]
        Qg = tw.shape[0]
        thr0 = token_pruning_floor(tw, qn, tb, k, combine, eps, top_t=top_t, select=sel, weights=Wg) if prune else None
        pruned = pruned or thr0 is not None
        nl = ops.cosine_token_topk_chunks(N, P, Qg, D, k)
        ps = torch.empty(Qg, nl, k, device=q.device)
        pi = torch.empty(Qg, nl, k, device=q.device, dtype=torch.int64)
        if W is None:
            ops.cosine_token_topk(tw, qn, tb.bank, tb.norms, k, code, eps, idx_offset, nl, ps, pi, thr0, t, words)
        else:
            ops.cosine_token_topk_pq(tw, qn, tokens, Wg, k, code, eps, idx_offset, nl, ps, pi, thr0, t, words)
        ops.topk_merge(ps, pi, Qg, nl, k, out_s[lo:lo + step], out_i[lo:lo + step], torch.empty(Qg, device=q.device, dtype=torch.int32))
    if stats is not None:
        stats.update(path="tokens", groups=(Q + step - 1) // step, pruned=pruned)
        if W is not None:
            stats.update(per_query_weights=True, group=step)
        if top_t is not None:
            stats.update(top_t=t)
        if sel is not None:
            stats.update(selected=sel.count)
    if world_size > 1:
        from .distributed import gather_topk
        gs, gi = gather_topk(out_s, out_i, world_size, process_group)   # RCCL all-gather -> [Q, world, k]
        ops.topk_merge(gs, gi, Q, world_size, k, out_s, out_i)
    return out_s, out_i


def cosine_token_scores(queries: torch.Tensor, bank, combine: str = 'min', weights: torch.Tensor | None = None, eps: float = 1e-6,
                        top_t: int | None = None, select=None):
    """[Q, N] combined score of every image of a [N,P,D] token bank (fp32, fp16 or bf16; or a TokenBank), in groups of at most
    16 queries.
    ``weights`` is ignored when ``bank`` is a TokenBank (it carries its own).  ``top_t``: as for ``cosine_topk_tokens`` (None:
    all tokens; else only the top_t best token scores of an image count, mean summed largest first -- so 'mean' with
    ``top_t == P`` is not the plain mean).  ``select``: as for ``cosine_topk_tokens``; every [Q, N] slot is written, a deselected
    image gets -inf.  ``weights`` [Q, D]: per-query weights, as for ``cosine_topk_tokens`` (groups of g queries at k = 1)."""
    tokens = bank.bank if isinstance(bank, TokenBank) else bank
    Q, D = queries.shape
    assert tokens.dim() == 3 and D == tokens.shape[2]
    code = _combine_code(combine, "cosine_token_scores")
    t = _top_t_arg(top_t, tokens.shape[1], "cosine_token_scores")
    W = _weights_arg(weights, Q, D, "cosine_token_scores", isinstance(bank, TokenBank))
    if W is not None:
        ops.bank_dtype_code(tokens.dtype, "cosine_token_scores")
        step = _pq_group("cosine_token_scores", tokens.shape[1], D, 1)
        sel = _selection_arg(select, tokens.shape[0], "cosine_token_scores", tokens.device)
        q = queries.to(tokens.device, torch.float32).contiguous()
        W = W.to(tokens.device, torch.float32).contiguous()
        out = torch.empty(Q, tokens.shape[0], device=q.device)
        if Q == 0:
            return out
        tw, qn = prepare_queries_pq(q, W)
        for lo in range(0, Q, step):
            ops.cosine_token_scores_pq(tw[lo:lo + step], qn[lo:lo + step], tokens, W[lo:lo + step], code, eps, out[lo:lo + step], t,
                                       None if sel is None else sel.words)
        return out
    _check_token_shape("cosine_token_scores", Q, tokens.shape[1], D, 1)
    sel = _selection_arg(select, tokens.shape[0], "cosine_token_scores", tokens.device)
    words = None if sel is None else sel.words
    tb = bank if isinstance(bank, TokenBank) else TokenBank(bank, weights)
    q = queries.to(tb.bank.device, torch.float32).contiguous()
    out = torch.empty(Q, tb.bank.shape[0], device=q.device)
    if Q == 0:
        return out
    tw, qn = prepare_queries(q, tb.weights)
    for lo in range(0, Q, 16):
        out[lo:lo + 16] = _token_scores(tw[lo:lo + 16], qn[lo:lo + 16], tb.bank, tb.norms, code, eps, t, words)
    return out


# ------------------------------------------------------------------------------------------------
# the distance metrics (weighted MSE / MAE, utils/similarity.py:174-212) over the same token banks: smaller is better
# ------------------------------------------------------------------------------------------------
def _metric_code(metric, who):
    if metric not in ops.METRIC_CODES:
        raise ValueError(f"{who}: metric = {metric!r}, expected one of {sorted(ops.METRIC_CODES)} (the cosine metric is "
                         f"cosine_topk_tokens / cosine_token_scores)")
    return ops.METRIC_CODES[metric]


def prepare_distance_weights(weights, D, device):
    """c = fp32(w / sum(w)) [D] on the device, by torch: the feature weights as the distance kernels take them (None: w = 1).
    ``weights`` [Q, D] (per-query weights): c [Q, D], every row prepared on its own by the [D] rule, so row q is bit-equal to
    what the single-query search prepares from it."""
    if weights is not None and weights.dim() == 2:
        return torch.stack([prepare_distance_weights(row, D, device) for row in weights]).contiguous()
    w = torch.ones(D, device=device) if weights is None else weights.to(device, torch.float32).reshape(D)
    return (w / w.sum()).contiguous()


def _distance_scores(c, t, tokens, mcode, ccode, top_t=0, words=None):
    """[Q, N] combined distances of Q <= 16 queries; c [D], or [Q, D] with one row per query."""
    out = torch.empty(t.shape[0], tokens.shape[0], device=t.device)
    (ops.distance_token_scores if c.dim() == 1 else ops.distance_token_scores_pq)(c, t, tokens, mcode, ccode, out, top_t, words)
    return out


def _distance_sample(bank, sel, images):
    """The floor's strided sample of ``images`` whole images [S, P, D]: a TokenBank's own (``TokenBank.sample``) or, under a
    selection, the one that Selection keeps for it; a plain tensor is gathered anew (no norms are computed for it)."""
    if isinstance(bank, TokenBank):
        return bank.sample(images)[0] if sel is None else sel.sample(bank, images)[0]
    n = bank.shape[0] if sel is None else sel.count
    idx = torch.arange(images, device=bank.device) * (n // images)
    return bank.index_select(0, idx if sel is None else sel.indices()[idx])


def distance_pruning_floor(c, t, bank, k: int, metric: str = 'MAE', combine: str = 'mean', sample_images: int | None = None,
                           top_t: int | None = None, select=None):
    """``token_pruning_floor`` for the distance metrics, in KEY space (key = -distance): the same sample of whole images (the
    selection's own under ``select``) is scored by the distance kernel, negated, and its k-th largest key, one ulp lower, is a
    floor of the k-th best key of the search.  None under the same size rule (fewer than 8 x the sample's images).  ``c``:
    ``prepare_distance_weights`` ([D], or [Q, D] with one row per query of ``t``); ``t`` [Q <= 16, D]; ``bank``: a [N,P,D] tensor or
    a TokenBank."""
    tokens = bank.bank if isinstance(bank, TokenBank) else bank
    N, P = tokens.shape[0], tokens.shape[1]
    tt = _top_t_arg(top_t, P, "distance_pruning_floor")
    if tuple(c.shape) not in ((t.shape[1],), tuple(t.shape)):
        raise ValueError(f"distance_pruning_floor: c has shape {tuple(c.shape)}, expected ({t.shape[1]},) or {tuple(t.shape)} for "
                         f"queries of shape {tuple(t.shape)}")
    mcode, ccode = _metric_code(metric, "distance_pruning_floor"), _combine_code(combine, "distance_pruning_floor")
    sel = _selection_arg(select, N, "distance_pruning_floor", tokens.device)
    if sample_images is None:
        sample_images = 256 * k
    if (N if sel is None else sel.count) < 8 * sample_images:
        return None
    keys = _distance_scores(c, t, _distance_sample(bank, sel, sample_images), mcode, ccode, tt).neg_()
    floor = torch.empty(t.shape[0], device=t.device)
    ops.kth_largest_floor(keys, k, floor)
    return floor


def distance_topk_tokens(queries: torch.Tensor, bank, k: int, metric: str = 'MAE', combine: str = 'mean',
                         weights: torch.Tensor | None = None, prune: bool = True, stats: dict | None = None, top_t: int | None = None,
                         select=None, process_group=None, world_size: int = 1):
    """-> (distances f32 [Q,k] ascending, image indices i64 [Q,k]): exact top-k images by the combined weighted MSE / MAE distance
    of their P patch tokens to each query (reference: compute_similarity with metric 'MSE' | 'MAE', utils/similarity.py:174-268,
    + update_best_scores), order (distance asc, image asc).  ``bank``: a [N,P,D] tensor (fp32, fp16 or bf16) or a TokenBank (its
    norms go unused; its weights are the feature weights, ``weights`` is then ignored); one pass per group of at most 16
    queries.  The arithmetic and its fixed summation order are the contract in include/skyemb.h: a 16-bit bank gives the fp32
    result on the widened bank bit for bit.

    Combine, with a[0] <= a[1] <= ... the ``top_t`` smallest token distances of an image (``top_t`` None: all P): 'min' is a[0];
    'max' the largest of those used (a[top_t-1], or the plain max); 'mean' (((0 + a[0]) + a[1]) + ...) / float32(top_t), smallest
    first (``top_t`` None: token order, divided by P -- so top_t == P is not the plain mean).  A NaN token distance ranks as +inf
    (torch would propagate the NaN): 'min' ignores it, 'max' and 'mean' become +inf, as they do for an image with fewer than top_t
    finite token distances; an image whose combined distance is +inf is never returned.  Missing entries are (+inf, -1).

    ``select``, ``prune``, ``stats``, ``world_size``: as for ``cosine_topk_tokens`` (the floor and the merges work on
    key = -distance).  Every ValueError -- an unknown metric or combine, top_t outside 1 .. min(P, 16), k, a selection of
    another length, a shape the kernels do not take -- is raised before the first launch.

    ``weights`` [Q, D] (per-query weights, one row per query, also over a TokenBank's own; [D] or None: the search above, same
    kernels, same bits): query q takes c_q = fp32(w_q / sum(w_q)), prepared row by row, and the contract is untouched, so row q of
    the result is bit for bit the Q = 1 search with query q and ``weights=w_q``.  c [Q, D] sits in LDS beside the queries, so
    the queries run in groups of the largest g <= 16 with 128 D + 32 g k <= 163840, as for ``cosine_topk_tokens``;
    ``stats['per_query_weights']`` is True and ``stats['group']`` is g."""
    who = "distance_topk_tokens"
    tokens = bank.bank if isinstance(bank, TokenBank) else bank
    Q, D = queries.shape
    N, P = tokens.shape[0], tokens.shape[1]
    assert tokens.dim() == 3 and D == tokens.shape[2]
    mcode, ccode = _metric_code(metric, who), _combine_code(combine, who)
    tt = _top_t_arg(top_t, P, who)
    if k < 1:
        raise ValueError(f"{who}: k = {k}")
    if world_size == 1 and k > N:
        raise ValueError(f"{who}: k = {k} exceeds the {N} images of the bank")
    ops.bank_dtype_code(tokens.dtype, who)
    W = _weights_arg(weights, Q, D, who, isinstance(bank, TokenBank))
    if W is None:
        _check_token_shape(who, Q, P, D, k)
        step = 16
    else:
        step = _pq_group(who, P, D, k)
    sel = _selection_arg(select, N, who, tokens.device)
    words = None if sel is None else sel.words
    dev = tokens.device
    idx_offset = bank.idx_offset if isinstance(bank, TokenBank) else 0
    if isinstance(bank, TokenBank) and W is None:
        weights = bank.weights
    q = queries.to(dev, torch.float32).contiguous()
    out_s = torch.empty(Q, k, device=dev)
    out_i = torch.empty(Q, k, device=dev, dtype=torch.int64)
    if Q == 0:
        return out_s, out_i
    c_all = prepare_distance_weights(weights, D, dev)
    pruned = False
    for lo in range(0, Q, step):
        t = q[lo:lo + step]
        c = c_all if W is None else c_all[lo:lo + step]
        Qg = t.shape[0]
        thr0 = distance_pruning_floor(c, t, bank, k, metric, combine, top_t=top_t, select=sel) if prune else None
        pruned = pruned or thr0 is not None
        nl = ops.cosine_token_topk_chunks(N, P, Qg, D, k)
        ps = torch.empty(Qg, nl, k, device=dev)
        pi = torch.empty(Qg, nl, k, device=dev, dtype=torch.int64)
        (ops.distance_token_topk if W is None else ops.distance_token_topk_pq)(c, t, tokens, mcode, ccode, k, idx_offset, nl, ps, pi,
                                                                               thr0, tt, words)
        ops.topk_merge(ps, pi, Qg, nl, k, out_s[lo:lo + step], out_i[lo:lo + step], torch.empty(Qg, device=dev, dtype=torch.int32))
    if stats is not None:
        stats.update(path="tokens", metric=metric, groups=(Q + step - 1) // step, pruned=pruned)
        if W is not None:
            stats.update(per_query_weights=True, group=step)
        if top_t is not None:
            stats.update(top_t=tt)
        if sel is not None:
            stats.update(selected=sel.count)
    if world_size > 1:
        from .distributed import gather_topk
        gs, gi = gather_topk(out_s, out_i, world_size, process_group)   # keys: [Q, world, k]
        ops.topk_merge(gs, gi, Q, world_size, k, out_s, out_i)
    return out_s.neg_(), out_i                                          # keys -> distances: (-inf, -1) becomes (+inf, -1)


def distance_token_scores(queries: torch.Tensor, bank, metric: str = 'MAE', combine: str = 'mean', weights: torch.Tensor | None = None,
                          top_t: int | None = None, select=None):
    """[Q, N] combined weighted MSE / MAE distance of every image of a [N,P,D] token bank (fp32, fp16 or bf16; or a TokenBank, whose
    weights then replace ``weights``), in groups of at most 16 queries; ``metric``, ``combine``, ``top_t`` and the NaN rule as for
    ``distance_topk_tokens``.  ``select``: every [Q, N] slot is written, a deselected image gets +inf.  ``weights`` [Q, D]:
    per-query weights, as for ``distance_topk_tokens`` (groups of g queries at k = 1)."""
    who = "distance_token_scores"
    tokens = bank.bank if isinstance(bank, TokenBank) else bank
    Q, D = queries.shape
    assert tokens.dim() == 3 and D == tokens.shape[2]
    mcode, ccode = _metric_code(metric, who), _combine_code(combine, who)
    tt = _top_t_arg(top_t, tokens.shape[1], who)
    ops.bank_dtype_code(tokens.dtype, who)
    W = _weights_arg(weights, Q, D, who, isinstance(bank, TokenBank))
    if W is None:
        _check_token_shape(who, Q, tokens.shape[1], D, 1)
        step = 16
    else:
        step = _pq_group(who, tokens.shape[1], D, 1)
    sel = _selection_arg(select, tokens.shape[0], who, tokens.device)
    words = None if sel is None else sel.words
    if isinstance(bank, TokenBank) and W is None:
        weights = bank.weights
    q = queries.to(tokens.device, torch.float32).contiguous()
    out = torch.empty(Q, tokens.shape[0], device=tokens.device)
    if Q == 0:
        return out
    c = prepare_distance_weights(weights, D, tokens.device)
    for lo in range(0, Q, step):
        out[lo:lo + step] = _distance_scores(c if W is None else c[lo:lo + step], q[lo:lo + step], tokens, mcode, ccode, tt, words)
    return out
