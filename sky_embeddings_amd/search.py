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

import bisect
import dataclasses
import weakref

import torch

from . import ops


_AN_LP = {torch.float16: "an fp16", torch.bfloat16: "an bf16"}     # a 16-bit bank as the alignment refusals name it


def _sample_index(images: int, n: int, device):
    """The strided sample every pruning floor draws: ``images`` of n rows / images / selected images, n // images apart."""
    return torch.arange(images, device=device) * (n // images)


def _kth_floor(scores: torch.Tensor, k: int):
    """[Q] the k-th largest of every row of ``scores`` [Q, S], one ulp lower (radix select, one launch): a pruning floor."""
    floor = torch.empty(scores.shape[0], device=scores.device)
    ops.kth_largest_floor(scores, k, floor)
    return floor


class PreparedBank:
    """Bank rows + their weighted norms (recomputed only when the weights change).

    ``bank`` is fp32, or fp16 / bf16 for a half-precision resident bank (``dtype``): such a bank IS the fp32 bank its elements
    widen to -- norms, scores and every search result are those of the widened bank bit for bit -- and nothing here ever holds
    an fp32 copy or a second image of it.  It must start 16-byte aligned (ValueError; a fresh tensor does).  A resident 16-bit
    bank of either format is made by ``PreparedBank.resident(bank)``; the plain constructor takes fp32 and fp16 and refuses bf16
    (ValueError naming ``resident``), as it always has.  The many-query search multiplies a bf16 bank's rows as bf16 matrix
    operands (v_mfma_f32_16x16x32_bf16) -- no conversion, which fp16 operands could not hold exactly."""

    def __init__(self, bank: torch.Tensor, weights: torch.Tensor | None = None, idx_offset: int = 0):
        if isinstance(bank, torch.Tensor) and bank.dtype == torch.bfloat16:
            raise ValueError("PreparedBank: the plain constructor does not take a bfloat16 bank (fp16 matrix operands cannot hold bf16 "
                             "values exactly); build it with PreparedBank.resident(bank, weights, idx_offset), whose many-query search "
                             "multiplies the rows as bf16 matrix operands -- or pass the flat [N, D] tensor itself to cosine_topk, "
                             "which serves it by the token search with one token per row (cosine_topk_tokens)")
        self._init(bank, weights, idx_offset)

    @classmethod
    def resident(cls, bank: torch.Tensor, weights: torch.Tensor | None = None, idx_offset: int = 0):
        """A PreparedBank over a resident 16-bit bank [N, D], fp16 or bf16 (ValueError for anything else).  fp16: exactly
        ``PreparedBank(bank, weights, idx_offset)``.  bf16: the same object over ``TokenBank(bank.unsqueeze(1))``, which computes
        the norms -- ``half_image()`` returns ``(bank, rowp)``, ``tail_tile`` holds the last N % 256 rows; no fp32 copy and no
        second image exist."""
        if not isinstance(bank, torch.Tensor) or bank.dtype not in ops.LP_DTYPES:
            what = bank.dtype if isinstance(bank, torch.Tensor) else type(bank).__name__
            raise ValueError(f"PreparedBank.resident: a resident bank is torch.float16 or torch.bfloat16, got {what}; an fp32 bank "
                             f"takes PreparedBank(bank)")
        if bank.dtype == torch.float16:
            return cls(bank, weights, idx_offset)
        self = cls.__new__(cls)
        self._init(bank, weights, idx_offset)
        return self

    def _init(self, bank, weights, idx_offset):
        if bank.dtype in ops.LP_DTYPES:
            ops._check_aligned16(bank, "PreparedBank", _AN_LP[bank.dtype])
        assert bank.is_cuda and bank.dtype in ops.BANK_DTYPES and bank.is_contiguous() and bank.dim() == 2
        self.bank, self.idx_offset, self.dtype = bank, int(idx_offset), bank.dtype
        self._sample = None
        self._half = None
        self.tail_tile = None
        self._version = 0                                  # counts set_weights calls: what depends on norms or row constants checks it
        self._row_tokens = None
        if self.dtype == torch.float32:
            self._tokens = None
            self.norms = torch.empty(bank.shape[0], device=bank.device)
            self.set_weights(weights)
        else:
            # the same rows as a token bank with one token per row: the route of the searches the two-stage path does not take
            # (and of its uncertified queries).  It computes the norms (ops.weighted_norms_lp); they are shared, not computed twice.
            self._tokens = TokenBank(bank.unsqueeze(1), weights, idx_offset)
            self.norms, self.weights = self._tokens.norms, self._tokens.weights

    def set_weights(self, weights):
        if self._tokens is not None:
            self._tokens.set_weights(weights)
            self.weights = self._tokens.weights
        else:
            self.weights = None if weights is None else weights.to(self.bank.device, torch.float32).contiguous()
            ops.weighted_norms(self.bank, self.weights, self.norms)
        self._version += 1
        self._row_tokens = None
        self._sample = None
        self._half = None

    def row_tokens(self):
        """The same rows as a TokenBank with one token per row: the route of a search under a selection that the two-stage path
        does not take, and of its uncertified queries.  A 16-bit bank has it from the start (it shares the norms); an fp32 bank
        builds it on first use -- one norm pass, 4 bytes per row, no copy of the rows -- and keeps it until the weights change."""
        if self._tokens is not None:
            return self._tokens
        if self._row_tokens is None:
            self._row_tokens = TokenBank(self.bank.unsqueeze(1), self.weights, self.idx_offset)
        return self._row_tokens

    def half_image(self):
        """(bank16, rowp): the fp16 rows + per-row constants the prefiltered many-query search runs on; built on first use and
        kept until the weights change.  fp32 bank: bank16 is a scaled fp16 image of it (one pass over the bank, +50 % bank
        memory).  fp16 / bf16 bank: bank16 is the bank itself; only ``rowp`` (16 bytes per row) and ``tail_tile`` -- a zero-padded copy
        of the last N % 256 rows, one tile [256, D], or None -- are allocated."""
        if self._half is None:
            if self.dtype == torch.float32:
                self._half = ops.bank16_prepare(self.bank, self.norms)
                self.tail_tile = None
            elif self.dtype == torch.float16:
                self.tail_tile, rowp = ops.bank16_rowp_lp(self.bank, self.norms)
                self._half = (self.bank, rowp)
            else:
                self.tail_tile, rowp = ops.resident_rowp(self.bank, self.norms)
                self._half = (self.bank, rowp)
        return self._half

    def two_stage(self, tw, qn, k, eps, out_s, out_i, redo, prepared=None):
        """Launch the two-stage search (csrc/topk_prefilter.hip) of this bank's dtype into (out_s, out_i, redo) -- under a selection
        when ``prepared`` is ``Selection.prefilter`` of this bank.  With ``half_image`` the one place that tells the three banks
        apart on that path."""
        bank16, rowp = self.half_image()
        if prepared is not None:
            ops.cosine_topk_prefiltered_sel(tw, qn, self.bank if self.dtype == torch.float32 else None, self.norms, bank16, self.tail_tile,
                                            prepared, k, eps, self.idx_offset, out_s, out_i, redo)
        elif self.dtype == torch.float32:
            ops.cosine_topk_prefiltered(tw, qn, self.bank, self.norms, bank16, rowp, k, eps, self.idx_offset, out_s, out_i, redo)
        else:
            op = ops.cosine_topk_prefiltered_lp if self.dtype == torch.float16 else ops.cosine_topk_prefiltered_resident
            op(tw, qn, bank16, self.norms, self.tail_tile, rowp, k, eps, self.idx_offset, out_s, out_i, redo)

    def whole_live_tiles(self, prepared):
        """The live whole 256-row tiles of a prepared selection: a 16-bit bank's partial last tile, read from ``tail_tile``, is not
        one (what SELECT_MIN_LIVE_TILES is compared with)."""
        n_live, last_live = prepared[2], prepared[3]
        return n_live - (1 if self.dtype != torch.float32 and self.bank.shape[0] % 256 and last_live else 0)

    def sample(self, rows: int):
        """A strided row sample (bank rows + norms) used to derive the pruning floor of a search."""
        N = self.bank.shape[0]
        rows = min(rows, N)
        if self._sample is None or self._sample[0].shape[0] != rows:
            idx = _sample_index(rows, N, self.bank.device)
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
    return _kth_floor(sc, k)


def _prefilter_enabled():
    import os
    return os.environ.get("SKYEMB_TOPK_PREFILTER", "1") != "0"


def _two_stage(Q, k, device, launch, rerun):
    """The two-stage driver every route shares: allocate the result and the redo flags, ``launch(out_s, out_i, redo)`` stages 1 + 2,
    read the flags once, have ``rerun(again)`` -> (scores, indices) search the flagged queries ``again`` (i64, ascending) exactly,
    copy those rows back.  -> (out_s, out_i, number of queries re-run)."""
    out_s = torch.empty(Q, k, device=device)
    out_i = torch.empty(Q, k, device=device, dtype=torch.int64)
    redo = torch.empty(Q, device=device, dtype=torch.int32)
    launch(out_s, out_i, redo)
    again = torch.nonzero(redo).squeeze(1)                 # host sync: a handful of bytes per search
    if again.numel():
        s2, i2 = rerun(again)
        out_s.index_copy_(0, again, s2)
        out_i.index_copy_(0, again, i2)
    return out_s, out_i, int(again.numel())


def _gather_merge(out_s, out_i, Q, k, world_size, process_group):
    """Every rank's [Q, k] lists all-gathered over RCCL -> [Q, world, k] and merged into (out_s, out_i); one rank: as they are."""
    if world_size > 1:
        from .distributed import gather_topk
        gs, gi = gather_topk(out_s, out_i, world_size, process_group)
        ops.topk_merge(gs, gi, Q, world_size, k, out_s, out_i)
    return out_s, out_i


SELECT_MIN_LIVE_TILES = 8      # fewer live whole 256-row tiles than this: a PreparedBank search under a selection takes the token route


@dataclasses.dataclass(frozen=True)
class RowRequest:
    """One ``cosine_topk`` call as it stands before the first launch: everything ``_row_request`` decides."""
    route: str                          # 'empty' | 'tokens' | 'exact' | 'prefiltered'
    Q: int
    N: int
    D: int
    k: int
    bank: object                        # 'tokens': what cosine_topk_tokens searches; else the PreparedBank (or the flat fp32 tensor)
    weights: torch.Tensor | None        # 'tokens' over a flat tensor: the caller's; else None (a PreparedBank carries its own)
    select: object                      # 'tokens': the caller's, as given; else None | the Selection
    rerun: str | None                   # 'prefiltered': what searches its uncertified queries, 'exact' | 'tokens'


def _row_request(who, queries, bank, k, weights, select, world_size=1) -> RowRequest:
    """Validate a ``cosine_topk`` call and decide its route.  No device work, except that a bool-tensor ``select`` over a PreparedBank
    is packed into a Selection (one short launch).  Every ValueError of ``cosine_topk`` that is not ``cosine_topk_tokens``'s own is
    raised here, in this order: [Q, D] weights over anything but a flat tensor; ``select`` over neither a flat tensor nor a
    PreparedBank.  Then a flat tensor with [Q, D] weights, with ``select`` or of a 16-bit dtype is route 'tokens' (one token per
    row; ``cosine_topk_tokens`` validates it).  A PreparedBank under ``select``: the two-stage path does not apply (Q <= 16 -- Q = 0
    and k < 1 included --, the shape, the switch); k > N; the token search's shape rule; the selection.  Any other bank: k < 1;
    k > N; then Q = 0 is route 'empty', a 16-bit bank off the two-stage path route 'tokens' (its one-token TokenBank), and on it the
    token search's shape rule (its uncertified queries go there: ``rerun``; an fp32 bank without a selection re-runs them by the
    exact kernel).  One decision waits for ``Selection.prefilter``'s read-back: the fall of a 'prefiltered' request under a
    selection to the token route below SELECT_MIN_LIVE_TILES (``cosine_topk``)."""
    pb = bank if isinstance(bank, PreparedBank) else None
    flat = isinstance(bank, torch.Tensor) and bank.dim() == 2
    per_query = isinstance(weights, torch.Tensor) and weights.dim() == 2
    Q, D = queries.shape
    if per_query and not flat:
        raise ValueError(f"{who}: per-query weights [Q, D] are served by the token search (cosine_topk_tokens with one "
                         "token per row); pass the flat [N, D] tensor, not a PreparedBank")
    if select is not None and pb is None and not flat:
        raise ValueError(f"{who}: select needs a flat [N, D] bank tensor")
    if flat and (per_query or select is not None or bank.dtype in ops.LP_DTYPES):
        return RowRequest('tokens', Q, bank.shape[0], D, k, bank.unsqueeze(1), weights, select, None)
    # where the two-stage route does not apply a selection is refused as it ever was, before anything else is looked at (16 queries
    # or fewer never take it, whatever the bank)
    if select is not None and (Q <= 16 or not (_prefilter_enabled() and ops.topk_prefilter_applicable(Q, pb.bank.shape[0], D, k))):
        raise ValueError(f"{who}: select is served by the token search (cosine_topk_tokens with one token per row); pass "
                         "the flat [N, D] tensor, not a PreparedBank -- the prefiltered many-query route takes no selection")
    rows = bank if pb is None else pb.bank
    N = rows.shape[0]
    assert D == rows.shape[1]
    if select is None and k < 1:
        raise ValueError(f"{who}: k = {k}")
    if world_size == 1 and k > N:
        raise ValueError(f"{who}: k = {k} exceeds the {N} rows of the bank")
    lp = rows.dtype != torch.float32
    if select is not None:
        _check_token_shape(who, Q, 1, D, k)                # the limits of the route the uncertified queries and small selections take
        return RowRequest('prefiltered', Q, N, D, k, bank, None, _selection_arg(select, N, who, rows.device), 'tokens')
    if Q == 0:                                             # nothing to search for (an empty target list): empty result, no launch
        return RowRequest('empty', Q, N, D, k, bank, None, None, None)
    if not (_prefilter_enabled() and ops.topk_prefilter_applicable(Q, N, D, k)):
        return RowRequest('tokens', Q, N, D, k, pb._tokens, None, None, None) if lp else RowRequest('exact', Q, N, D, k, bank, None, None, None)
    if lp:
        _check_token_shape(who, Q, 1, D, k)                # the limits of the route its uncertified queries take
    return RowRequest('prefiltered', Q, N, D, k, bank, None, None, 'tokens' if lp else 'exact')


def cosine_topk(queries: torch.Tensor, bank, k: int, weights: torch.Tensor | None = None, eps: float = 1e-6,
                process_group=None, world_size: int = 1, prune: bool = True, stats: dict | None = None, select=None):
    """-> (scores f32 [Q,k], indices i64 [Q,k]).  ``bank`` is a [N,D] tensor or a PreparedBank
    (this rank's shard; ``idx_offset`` = first global row of the shard).  More than 16 queries take the two-stage
    path (fp16 matrix-core prefilter with a proven error bound, exact fp32 re-score of the survivors: same results bit
    for bit); SKYEMB_TOPK_PREFILTER=0 keeps every search on the exact fp32 kernels.

    A 2-D fp16 / bf16 tensor is a half-precision resident bank: it is served as a token bank with one token per row
    (``cosine_topk_tokens`` on ``bank.unsqueeze(1)``, ``stats['path'] == 'tokens'``) under that search's limits -- k <= 512,
    more than 16 queries in groups of 16 -- with the results of the fp32 search on the widened bank, bit for bit.  The
    many-query prefilter over a 16-bit bank is reached through ``PreparedBank.resident(bank)`` (fp16 or bf16; fp16 also through
    ``PreparedBank(bank_fp16)``): where the two-stage path applies
    (more than 16 queries, k <= 192, N >= 2048) it reads the resident 16-bit rows directly -- no fp32 copy, no second image: 16 bytes
    of constants per row and one 256-row tile -- with the results of the fp32 search on the widened bank, bit for bit
    (``stats['path'] == 'prefiltered'``; uncertified queries are re-run by the token search, ``stats['redone']``); everywhere
    else, and under SKYEMB_TOPK_PREFILTER=0, it is served as the bare tensor is (``stats['path'] == 'tokens'``), within that
    search's limits in both cases.  A bf16 bank's rows are multiplied as bf16 matrix operands against a bf16 split of the query
    (one pass by default, SKYEMB_PREFILTER_LO=1: two); a row with an inf / NaN element, a nonzero element outside [2^-60, 2^120) or
    an overflowed weighted norm cannot be bounded in stage 1 and is a candidate of every query, decided by the exact stage, and a
    query whose largest weighted component lies outside [2^-50, 2^79) is re-run by the token search.  fp32 banks take exactly the
    paths described above.

    ``select`` (None: nothing above changes; a bool tensor [N] or a ``Selection``): only the rows marked True are eligible, with
    the result of the search over the compacted bank and indices mapped back (``cosine_topk_tokens``'s ``select``).  A flat
    [N,D] bank of any dtype is then served as a token bank with one token per row (``stats['path'] == 'tokens'``) under that
    search's limits: k <= 512, D % 64 == 0, D <= 1024, queries in groups of 16.

    A PreparedBank (fp32 or resident fp16 / bf16) with ``select`` takes the two-stage path under the selection wherever that path
    applies to the whole bank (more than 16 queries, k <= 192, N >= 2048, SKYEMB_TOPK_PREFILTER not 0): the result is exactly that
    of ``cosine_topk(queries, PreparedBank(bank[select], weights), k)`` -- scores bit for bit, order (score desc, index asc), ties
    to the lower bank row -- with every index mapped back to this bank, then offset by ``idx_offset``.  Nothing is gathered: stage 1
    walks the live 256-row tiles (those with a selected row) and deselected rows fail its test through a masked copy of the row
    constants (16 bytes per row, built by two short launches and kept with a ``Selection`` per bank until the bank's weights
    change; a bool tensor is prepared on every call).  So a NaN, inf or all-zero row that is deselected changes nothing, and only
    selections that empty whole tiles save bank bytes -- the fp16 image is not compacted.  Fewer than k selected rows: a
    (-inf, -1) tail (k may exceed the selected count, not N), and a selected row that scores -inf (a NaN in it) is then not
    returned, as in ``cosine_topk_tokens``; none selected: all (-inf, -1), no launch.  Uncertified queries
    (``stats['redone']``) are re-run under the same selection by the token search with one token per row, for both bank dtypes
    (the exact fp32 kernel takes no selection), so D must be a multiple of 64 and at most 1024 (ValueError before any launch).  A
    selection with fewer than 8 live whole tiles (``SELECT_MIN_LIVE_TILES``: the phase schedule's own minimum, N >= 8 tiles, applied
    to the live-tile count) is served whole by that token search (``stats['path'] == 'tokens'``), never refused.  ``stats`` gains
    ``selected`` and ``tiles`` = (live bank tiles, all bank tiles).  Where the two-stage path does not apply (Q <= 16, k > 192,
    N < 2048, the switch off) the call is a ValueError as before: pass the flat tensor.  One selection serves all queries
    (per-query selections are out of scope); with ``world_size > 1`` it describes this rank's shard.

    ``weights`` [Q, D] (one row per query; [D] or None: nothing above changes): a flat [N,D] bank is served the same way, as
    ``cosine_topk_tokens`` with per-query weights and one token per row (``stats['path'] == 'tokens'``); a PreparedBank is a
    ValueError (per-query weights on the two-stage path are out of scope), with or without ``select``."""
    if not isinstance(bank, PreparedBank) and select is None and not (isinstance(weights, torch.Tensor) and weights.dim() == 2) \
            and not (isinstance(bank, torch.Tensor) and bank.dim() == 2 and bank.dtype in ops.LP_DTYPES):
        # an fp32 tensor searched on its own is a PreparedBank from here on.  Built before the request is validated, as it ever
        # was: the norm pass precedes even a refusal of k
        bank = PreparedBank(bank, weights)
    rq = _row_request("cosine_topk", queries, bank, k, weights, select, world_size)
    if rq.route == 'tokens':                               # served by the token search, one token per row
        return cosine_topk_tokens(queries, rq.bank, k, 'min', rq.weights, eps, process_group, world_size, prune, stats, select=rq.select)
    pb, sel, Q, dev, prepared = rq.bank, rq.select, rq.Q, rq.bank.bank.device, None
    if rq.route == 'empty':
        return torch.empty(0, k, device=dev), torch.empty(0, k, device=dev, dtype=torch.int64)
    q = queries.to(dev, torch.float32).contiguous()
    if sel is not None:
        tiles_all = (rq.N + 255) // 256
        if sel.count == 0:                                 # nothing is eligible: no stage-1 launch
            if stats is not None:
                stats.update(path="prefiltered", redone=0, selected=0, tiles=(0, tiles_all))
            return _gather_merge(torch.full((Q, k), float("-inf"), device=dev), torch.full((Q, k), -1, device=dev, dtype=torch.int64), Q, k,
                                 world_size, process_group)
        prepared = sel.prefilter(pb)
        if pb.whole_live_tiles(prepared) < SELECT_MIN_LIVE_TILES:      # the token search serves the whole call, gather included
            st = {}
            out = cosine_topk_tokens(q, pb.row_tokens(), k, 'min', None, eps, process_group, world_size, prune, st, select=sel)
            if stats is not None:
                stats.update(st, selected=sel.count, tiles=(prepared[2], tiles_all))
            return out
    tw, qn = prepare_queries(q, pb.weights)
    if rq.route == 'exact':
        thr0 = pruning_floor(tw, qn, pb, k, eps) if prune else None
        out_s, out_i = _local_topk(tw, qn, pb.bank, pb.norms, k, eps, pb.idx_offset, thr0)
        n_redo = 0
    else:
        def rerun_exact(again):                            # the exact fp32 kernel, under a floor of its own whatever ``prune`` says
            tw2, qn2 = tw.index_select(0, again).contiguous(), qn.index_select(0, again).contiguous()
            return _local_topk(tw2, qn2, pb.bank, pb.norms, k, eps, pb.idx_offset, pruning_floor(tw2, qn2, pb, k, eps))

        def rerun_tokens(again):                           # the token search with one token per row, under the same selection
            return cosine_topk_tokens(q.index_select(0, again), pb.row_tokens(), k, 'min', None, eps, prune=prune, select=sel)

        out_s, out_i, n_redo = _two_stage(Q, k, dev, lambda *out: pb.two_stage(tw, qn, k, eps, *out, prepared),
                                          rerun_exact if rq.rerun == 'exact' else rerun_tokens)
    if stats is not None:
        stats.update(path=rq.route, redone=n_redo)
        if sel is not None:
            stats.update(selected=sel.count, tiles=(prepared[2], tiles_all))
    return _gather_merge(out_s, out_i, Q, k, world_size, process_group)


def cosine_scores(queries: torch.Tensor, bank, weights: torch.Tensor | None = None, eps: float = 1e-6):
    """Plain [Q,N] score matrix (reference-shaped path with several patches per sample)."""
    pb = bank if isinstance(bank, PreparedBank) else PreparedBank(bank, weights)
    if pb.dtype != torch.float32:
        raise ValueError("cosine_scores: an fp16 bank is scored by cosine_token_scores (one token per row: bank.unsqueeze(1))")
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
    pass.  The only approximation is the rounding when the bank was stored (``standardise_to``).

    ``TokenBank.resident(bank)`` (fp16 / bf16 only) is the same object in every respect -- same norms, ``set_weights``, ``sample`` --
    that also opens the two-stage many-query route of ``cosine_topk_tokens`` (see there): it carries, built on first use and
    dropped when the weights change, the stage-1 row constants of its N * P rows (``stage1()``: 16 bytes per row and one
    zero-padded 256-row tail tile).  No fp32 copy and no second image of the bank exist.  The plain constructor never takes that
    route."""

    def __init__(self, bank: torch.Tensor, weights: torch.Tensor | None = None, idx_offset: int = 0):
        ops.bank_dtype_code(bank.dtype, "TokenBank")          # ValueError for anything but fp32 / fp16 / bf16
        assert bank.is_cuda and bank.is_contiguous() and bank.dim() == 3
        self.bank, self.idx_offset, self.dtype = bank, int(idx_offset), bank.dtype
        self.norms = torch.empty(bank.shape[0] * bank.shape[1], device=bank.device)
        self._resident = False                             # True: made by TokenBank.resident
        self._stage1 = None                                # (tail tile, rowp) of the two-stage route
        self._stage1_mean = None                           # (pooled image, its tail tile, rowp) of the route under combine 'mean'
        self._stage1_mse = None                            # (c, tail tile, rowp) of the weighted-MSE route, for the last c seen
        self._mse_top_t = False                            # True: asked to take that route under top_t too (prepare_mse_top_t)
        self._mse_pq = None                                # (image [x ; x o x], rowp) of that route with per-query weights (prepare_mse_per_query)
        self._mse_mean = None                              # (pooled image, its tail tile, aux) of that route under combine 'mean' (prepare_mse_mean)
        self._stage1_mse_mean = None                       # (c, rowp) of it, for the last c seen
        self._version = 0                                  # counts set_weights calls: what depends on the norms checks it
        self.set_weights(weights)

    @classmethod
    def resident(cls, bank: torch.Tensor, weights: torch.Tensor | None = None, idx_offset: int = 0):
        """A TokenBank over a resident 16-bit token bank: a contiguous, 16-byte aligned [N, P, D] tensor of fp16 or bf16 (ValueError
        for anything else), whose many-query min / max / mean searches may take the two-stage route (``cosine_topk_tokens``)."""
        if not isinstance(bank, torch.Tensor) or bank.dtype not in ops.LP_DTYPES:
            what = bank.dtype if isinstance(bank, torch.Tensor) else type(bank).__name__
            raise ValueError(f"TokenBank.resident: a resident token bank is torch.float16 or torch.bfloat16, got {what}; an fp32 bank "
                             f"takes TokenBank(bank)")
        if bank.dim() != 3 or not bank.is_contiguous():
            raise ValueError(f"TokenBank.resident: the bank must be a contiguous [N, P, D] tensor, got shape {tuple(bank.shape)}, "
                             f"strides {tuple(bank.stride())}")
        ops._check_aligned16(bank, "TokenBank.resident", _AN_LP[bank.dtype])
        self = cls(bank, weights, idx_offset)
        self._resident = True
        return self

    def stage1(self):
        """(tail, rowp) of ``ops.resident_rowp`` over the flat [N * P, D] rows: what stage 1 of the two-stage route reads besides the
        bank itself.  Built on first use, kept until the weights change."""
        if self._stage1 is None:
            N, P, D = self.bank.shape
            self._stage1 = ops.resident_rowp(self.bank.view(N * P, D), self.norms)
        return self._stage1

    def stage1_mean(self):
        """(pooled, tail, rowp) of ``ops.token_mean_pool``: what stage 1 of the two-stage route reads under combine 'mean' -- the
        16-bit image [N, D] of the images' pooled unit tokens, its 256-row tail tile and the row constants of the mean bound
        (2 D + 16 bytes per image and one tail tile).  Built on first use, kept until the weights change."""
        if self._stage1_mean is None:
            self._stage1_mean = ops.token_mean_pool(self.bank, self.norms)
        return self._stage1_mean

    def stage1_mse(self, c):
        """(tail, rowp) of ``ops.token_mse_rowp`` under the distance weights ``c`` [D]: what stage 1 of the two-stage weighted-MSE
        route (``distance_topk_tokens``) reads besides the bank itself -- 16 bytes per token row and one 256-row tail tile.  Kept
        for the last ``c`` seen: the cache is keyed by the vector itself (compared element by element -- one small device-to-host
        read per search, next to the redo flags' --, so ``set_weights`` need not clear it); a different vector rebuilds them, one
        launch over the bank."""
        held = self._stage1_mse
        if held is None or not torch.equal(held[0], c):
            held = self._stage1_mse = (c.clone(), *ops.token_mse_rowp(self.bank, c))
        return held[1], held[2]

    def prepare_mse_top_t(self):
        """Ask this resident bank to take the two-stage weighted-MSE route of ``distance_topk_tokens`` under ``top_t`` as well
        (distance 'max' with 1 <= top_t < P: stage 1 counts the rows that pass, stage 2 sorts the token distances).  Nothing is built
        here -- the route reads ``stage1_mse`` as the plain one does --; a bank never asked answers ``top_t`` by the grouped route,
        as it always has.  Returns ``self``: ``TokenBank.resident(bank).prepare_mse_top_t()``."""
        if not self._resident:
            raise ValueError("TokenBank.prepare_mse_top_t: the bank must be made by TokenBank.resident")
        self._mse_top_t = True
        return self

    def prepare_mse_per_query(self):
        """Ask this resident bank to take the two-stage weighted-MSE route of ``distance_topk_tokens`` with per-query weights
        ([Q, D] ``weights``), and build what that route reads: a second 16-bit image [N P padded to whole 256-row tiles, 2 D] of the
        bank, rows [x ; x o x] with the squares rounded once to the bank's dtype, and its row constants (``ops.token_mse_pq_image``:
        one pass over the bank, 4 N P D + 16 N P bytes beside the bank's 2 N P D).  Neither depends on the weights -- per-query weights
        arrive with the search --, so ``set_weights`` keeps them.  A bank never asked answers per-query weights by the grouped route,
        as it always has.  Cosine with per-query weights keeps the grouped route either way: its row norm sits under a square root
        in the denominator, which no single dot product holds.  Returns ``self``:
        ``TokenBank.resident(bank).prepare_mse_per_query()``."""
        if not self._resident:
            raise ValueError("TokenBank.prepare_mse_per_query: the bank must be made by TokenBank.resident")
        N, P, D = self.bank.shape
        if D % 32 or not 128 <= D <= 2048:
            raise ValueError(f"TokenBank.prepare_mse_per_query: the image holds rows of 2 D: D % 32 == 0 and 128 <= D <= 2048 (D = {D})")
        if self._mse_pq is None:
            self._mse_pq = ops.token_mse_pq_image(self.bank)
        return self

    def prepare_mse_mean(self):
        """Ask this resident bank to take the two-stage weighted-MSE route of ``distance_topk_tokens`` under ``combine='mean'``, and
        build what that route reads: the pooled 16-bit image [N, D] of the bank -- each image's tokens summed in fp32 in token order,
        scaled exactly by 1 / P and by the image's own power of two, rounded once to the bank's dtype --, its 256-row tail tile and
        the bank's share of the row constants (``ops.token_mse_mean_pool``: one pass over the bank, 2 N D + 8 N bytes beside the
        bank's 2 N P D).  None of it depends on the weights, so ``set_weights`` keeps it; the weights' share (``stage1_mse_mean``) is
        one more pass per weight vector.  A bank never asked answers 'mean' by the grouped route, as it always has.  Returns
        ``self``: ``TokenBank.resident(bank).prepare_mse_mean()``."""
        if not self._resident:
            raise ValueError("TokenBank.prepare_mse_mean: the bank must be made by TokenBank.resident")
        if self._mse_mean is None:
            self._mse_mean = ops.token_mse_mean_pool(self.bank)
        return self

    def stage1_mse_mean(self, c):
        """(pooled, tail, rowp) of the two-stage weighted-MSE route under combine 'mean' and the distance weights ``c`` [D]: the
        pooled image and tail tile of ``prepare_mse_mean`` and the row constants of ``ops.token_mse_mean_rowp``, kept for the last
        ``c`` seen as ``stage1_mse`` keeps its own (keyed by the vector itself)."""
        if self._mse_mean is None:
            raise ValueError("TokenBank.stage1_mse_mean: the bank was not asked (TokenBank.prepare_mse_mean)")
        pooled, tail, aux = self._mse_mean
        held = self._stage1_mse_mean
        if held is None or not torch.equal(held[0], c):
            held = self._stage1_mse_mean = (c.clone(), ops.token_mse_mean_rowp(self.bank, c, aux))
        return pooled, tail, held[1]

    def set_weights(self, weights):
        self._version += 1
        self.weights = None if weights is None else weights.to(self.bank.device, torch.float32).contiguous()
        rows = self.bank.view(-1, self.bank.shape[2])
        if self.dtype == torch.float32:
            ops.weighted_norms(rows, self.weights, self.norms)
        else:
            ops.weighted_norms_lp(rows, self.weights, self.norms)
        self._sample = None                                # user -> its sample (see ``sample``)
        self._stage1 = self._stage1_mean = None

    def sample(self, images: int, user: str = "floor"):
        """A strided sample of WHOLE images (tokens [S, P, D] in the bank's dtype + the norms of their S * P rows) used to
        derive the pruning floor of a search.  One sample is kept per ``user`` -- the grouped route's floor and the two-stage
        route's bootstrap floor ask for different sizes, and a re-run alternates between them -- until the size or the weights change."""
        N, P, _ = self.bank.shape
        images = min(images, N)
        if self._sample is None:
            self._sample = {}
        got = self._sample.get(user)
        if got is None or got[0].shape[0] != images:
            idx = _sample_index(images, N, self.bank.device)
            got = self._sample[user] = (self.bank.index_select(0, idx).contiguous(),
                                        self.norms.view(N, P).index_select(0, idx).contiguous().view(-1))
        return got


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
        self._prefilter = None                             # PreparedBank -> (its version, its row constants, what stage 1 needs)
        self._token_prefilter = None                       # resident TokenBank -> the same
        self._mean = None                                  # resident TokenBank -> (its version, its pooled image, the compacted one)
        self._mse = None                                   # resident TokenBank -> None (asked, not built) | (its MSE rowp, what stage 1 needs)

    def prefilter(self, pb: "PreparedBank"):
        """What the two-stage many-query search needs of this selection over ``pb`` (``ops.prefilter_select_prepare``: the masked row
        constants, the live tiles, their number, whether the last tile is live).  Kept here per bank, like ``sample``, until the
        bank's weights -- and with them its row constants -- change: repeated searches under one Selection do not rebuild it."""
        if self._prefilter is None:
            self._prefilter = weakref.WeakKeyDictionary()
        rowp = pb.half_image()[1]
        got = self._prefilter.get(pb)
        if got is None or got[0] != pb._version or got[1] is not rowp:
            got = (pb._version, rowp, ops.prefilter_select_prepare(self.words, self.N, rowp))
            self._prefilter[pb] = got
        return got[2]

    def token_prefilter(self, tb: "TokenBank"):
        """What the two-stage token search needs of this selection over the resident ``tb`` (``ops.token_prefilter_select_prepare``: the
        masked row constants, the live tiles, their number, whether the last tile is live, and -- a host list, read back once here,
        never per search -- the selected images up to and including each live tile).  Kept per bank like ``prefilter``, rebuilt when
        the bank's weights version or its stage-1 constants change."""
        if self._token_prefilter is None:
            self._token_prefilter = weakref.WeakKeyDictionary()
        rowp = tb.stage1()[1]
        got = self._token_prefilter.get(tb)
        if got is None or got[0] != tb._version or got[1] is not rowp:
            got = (tb._version, rowp, ops.token_prefilter_select_prepare(self.words, tb.bank.shape[0], tb.bank.shape[1], rowp))
            self._token_prefilter[tb] = got
        return got[2]

    def prepare_mean(self, tb: "TokenBank"):
        """Ask this selection to hold, for the resident ``tb``, what the two-stage search under combine 'mean' reads in stage 1: the
        selected images' rows of ``tb.stage1_mean()`` compacted into an image [count, D] with its tail tile, row constants and the
        map compacted position -> image (``ops.token_mean_select_gather``: one short launch, 2 D + 20 bytes per selected image and
        one 256-row tail tile).  Only a Selection asked so takes that route (``cosine_topk_tokens``): the compaction pays when
        searches repeat under one Selection.  Kept per bank like ``token_prefilter``; once asked for a bank, an entry made stale by
        ``set_weights`` is rebuilt by the next search, not dropped.  Returns ``self``: ``Selection(flags).prepare_mean(tb)``."""
        if not isinstance(tb, TokenBank) or not tb._resident:
            raise ValueError("Selection.prepare_mean: the bank must be made by TokenBank.resident")
        if tb.bank.shape[0] != self.N:
            raise ValueError(f"Selection.prepare_mean: the selection describes {self.N} images, the bank has {tb.bank.shape[0]}")
        if self.words.device != tb.bank.device:
            raise ValueError(f"Selection.prepare_mean: the Selection was packed on {self.words.device}, the bank is on {tb.bank.device}")
        if self.count == 0:
            return self                                    # nothing to compact: the grouped route answers (-inf, -1)
        if self._mean is None:
            self._mean = weakref.WeakKeyDictionary()
        self._mean.setdefault(tb, None)
        self.mean_prefilter(tb)
        return self

    def mean_prefilter(self, tb: "TokenBank"):
        """(pooled_sel, tail_sel, rowp_sel, map) of ``prepare_mean`` for ``tb``, rebuilt when the bank's weights version or its pooled
        image changed since."""
        pooled = tb.stage1_mean()
        got = self._mean.get(tb)
        if got is None or got[0] != tb._version or got[1] is not pooled:
            got = (tb._version, pooled, ops.token_mean_select_gather(pooled[0], pooled[2], self.indices()))
            self._mean[tb] = got
        return got[2]

    def prepare_mse(self, tb: "TokenBank"):
        """Ask this selection to take the two-stage weighted-MSE route of ``distance_topk_tokens`` over the resident ``tb``.  Only a
        Selection asked so takes it; a bool tensor or a Selection never asked keeps the grouped route.  What stage 1 reads -- the
        masked copy of ``tb.stage1_mse(c)``'s row constants, the live tiles and their counts (``ops.token_prefilter_select_prepare``:
        two short launches, one read-back, 16 bytes per token row) -- depends on the distance weights ``c``, which only a search knows,
        so it is built by the first search per (bank, c) and kept until ``c`` or the bank's constants change (``mse_prefilter``).
        Returns ``self``: ``Selection(flags).prepare_mse(tb)``."""
        if not isinstance(tb, TokenBank) or not tb._resident:
            raise ValueError("Selection.prepare_mse: the bank must be made by TokenBank.resident")
        if tb.bank.shape[0] != self.N:
            raise ValueError(f"Selection.prepare_mse: the selection describes {self.N} images, the bank has {tb.bank.shape[0]}")
        if self.words.device != tb.bank.device:
            raise ValueError(f"Selection.prepare_mse: the Selection was packed on {self.words.device}, the bank is on {tb.bank.device}")
        if self._mse is None:
            self._mse = weakref.WeakKeyDictionary()
        self._mse.setdefault(tb, None)
        return self

    def mse_prefilter(self, tb: "TokenBank", c):
        """``token_prefilter`` for the weighted-MSE route under the distance weights ``c``: ``ops.token_prefilter_select_prepare`` over
        the row constants of ``tb.stage1_mse(c)``.  Keyed by those constants themselves: ``stage1_mse`` returns a new tensor exactly
        when ``c`` differs from the last one seen, and then this is rebuilt."""
        rowp = tb.stage1_mse(c)[1]
        got = self._mse.get(tb)
        if got is None or got[0] is not rowp:
            got = (rowp, ops.token_prefilter_select_prepare(self.words, tb.bank.shape[0], tb.bank.shape[1], rowp))
            self._mse[tb] = got
        return got[1]

    def sample(self, tb: "TokenBank", images: int):
        """A strided sample of ``images`` SELECTED whole images of ``tb`` (tokens + the norms of their rows) for the pruning floor.
        Kept here, with the selection it belongs to -- not in the bank -- until the bank, its weights or the size change, so
        that repeated searches under one Selection do not gather it again."""
        if self._sample is None:
            self._sample = weakref.WeakKeyDictionary()     # one entry per bank: a Selection may serve several (fp32 and fp16)
        got = self._sample.get(tb)
        if got is None or got[0] != tb._version or got[1] != images:
            N, P = tb.bank.shape[0], tb.bank.shape[1]
            idx = self.indices()[_sample_index(images, self.count, tb.bank.device)]
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


def _check_token_shape(who, Q, P, D, k):
    why = ops.cosine_token_refusal(max(1, min(Q, 16)), P, D, k)       # Q: queries per launch
    if why is not None:
        raise ValueError(f"{who}: {why}")


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


_COSINE = object()                      # ``metric`` of the two cosine functions: not a name a caller can pass


@dataclasses.dataclass(frozen=True)
class TokenRequest:
    """One patch-token request as it stands before the first launch: everything ``_token_request`` decides."""
    who: str                            # the public function, for error texts
    Q: int
    N: int
    P: int
    D: int
    k: int                              # the scores calls: 1
    combine: int                        # ops.COMBINE_CODES
    metric: int | None                  # ops.METRIC_CODES (``metric_name``: its key, for stats); None: cosine
    metric_name: str | None
    top_t: int                          # the library's argument: 0 = all tokens
    per_query: bool                     # weights are [Q, D]
    step: int                           # queries per pass
    idx_offset: int
    tokens: torch.Tensor                # [N, P, D], unwrapped
    bank: "TokenBank | None"            # the TokenBank the caller gave, if any
    weights: torch.Tensor | None        # the weights that count (see _token_request)
    select: "Selection | None"

    @property
    def groups(self):
        return (self.Q + self.step - 1) // self.step


def _token_request(who, queries, bank, k, combine, metric, weights, top_t, select, world_size=1) -> TokenRequest:
    """Validate a request of one of the four public token functions and decide what is decided before the first launch.  No
    device work, except that a bool-tensor ``select`` is packed into a Selection (one short launch).  ``k`` None: a scores call
    (planned at k = 1); ``metric`` _COSINE: no distance metric.  Every ValueError of those functions is raised here, in this
    order -- cosine: combine, top_t, k, weights shape, shape rule, selection; distance: metric, combine, top_t, k, bank dtype,
    weights shape, shape rule, selection.

    ``weights``: a TokenBank's own replace a [D] or None argument (which is then not even looked at); a [Q, D] argument
    overrides them.  ``step``: 16 with shared weights; with per-query weights the largest g <= 16 the library takes
    (``_pq_group``)."""
    tb, tokens = _unwrap(bank)
    (Q, D), (N, P) = queries.shape, tokens.shape[:2]
    assert tokens.dim() == 3 and D == tokens.shape[2]
    mcode = None if metric is _COSINE else _metric_code(metric, who)
    code = _combine_code(combine, who)
    t = _top_t_arg(top_t, P, who)
    if k is not None and k < 1:
        raise ValueError(f"{who}: k = {k}")
    if k is not None and world_size == 1 and k > N:
        raise ValueError(f"{who}: k = {k} exceeds the {N} images of the bank")
    k = 1 if k is None else k
    if mcode is not None:
        ops.bank_dtype_code(tokens.dtype, who)
    W = _weights_arg(weights, Q, D, who, tb is not None)
    if W is None:
        _check_token_shape(who, Q, P, D, k)
        step = 16
    else:
        if mcode is None:                    # cosine with shared weights leaves the dtype to the TokenBank it runs on
            ops.bank_dtype_code(tokens.dtype, who)
        step = _pq_group(who, P, D, k)
    sel = _selection_arg(select, N, who, tokens.device)
    return TokenRequest(who=who, Q=Q, N=N, P=P, D=D, k=k, combine=code, metric=mcode, metric_name=None if mcode is None else metric,
                        top_t=t, per_query=W is not None, step=step, idx_offset=0 if tb is None else tb.idx_offset, tokens=tokens,
                        bank=tb, weights=W if W is not None else (weights if tb is None else tb.weights), select=sel)


def _unwrap(bank):
    """``bank`` (TokenBank | [N, P, D] tensor) -> (the TokenBank or None, the token tensor): the one place that tells them apart."""
    return (bank, bank.bank) if isinstance(bank, TokenBank) else (None, bank)


def _floor_sample(tb, tokens, sel, images):
    """The floor's strided sample of ``images`` whole images: (tokens [S, P, D], norms of their S * P rows or None).  A TokenBank's
    own (``TokenBank.sample``) or, under a selection, the one that Selection keeps for it; a plain tensor is gathered anew, and no
    norms are computed for it."""
    if tb is not None:
        return tb.sample(images) if sel is None else sel.sample(tb, images)
    idx = _sample_index(images, tokens.shape[0] if sel is None else sel.count, tokens.device)
    return tokens.index_select(0, idx if sel is None else sel.indices()[idx]), None


class _CosineScorer:
    """What is cosine about a token search: how a group of queries -- (tw, qn, w): prepared queries and their [g, D] weight rows,
    w None for shared weights -- is scored against ``tokens`` or the floor's sample of them.  Shared weights (``W`` None) run on the
    TokenBank ``tb``, whose norms are an operand; per-query weights ``W`` [Q, D] need none (the kernel computes them), and ``tb`` is
    then only where the sample comes from, or None."""
    negate = False                                   # keys are the scores

    def __init__(self, tokens, tb, sel, combine, top_t, eps, W=None):
        self.tokens, self.tb, self.sel, self.combine, self.top_t, self.eps, self.W = tokens, tb, sel, combine, top_t, eps, W
        self.norms = tb.norms if W is None else None

    @classmethod
    def of(cls, rq: TokenRequest, eps):
        """The scorer of a search.  Shared weights over a plain tensor build a TokenBank here, which costs a norm pass; per-query
        weights never do: that pass is what they make useless."""
        if rq.per_query:
            return cls(rq.tokens, rq.bank, rq.select, rq.combine, rq.top_t, eps, rq.weights.to(rq.tokens.device, torch.float32).contiguous())
        return cls(rq.tokens, rq.bank if rq.bank is not None else TokenBank(rq.tokens, rq.weights), rq.select, rq.combine, rq.top_t, eps)

    def prepare(self, q):
        self.tw, self.qn = prepare_queries(q, self.tb.weights) if self.W is None else prepare_queries_pq(q, self.W)

    def group(self, lo, hi):
        return self.tw[lo:hi], self.qn[lo:hi], None if self.W is None else self.W[lo:hi]

    def sample(self, images):
        if self.W is None:                           # tokens and norms: of a TokenBank, as this call ever needed
            return self.tb.sample(images) if self.sel is None else self.sel.sample(self.tb, images)
        return _floor_sample(self.tb, self.tokens, self.sel, images)[0], None

    def scores(self, group, tokens, norms, out, words=None):
        tw, qn, w = group
        if w is None:
            ops.cosine_token_scores(tw, qn, tokens, norms, self.combine, self.eps, out, self.top_t, words)
        else:
            ops.cosine_token_scores_pq(tw, qn, tokens, w, self.combine, self.eps, out, self.top_t, words)

    def lists(self, group, k, idx_offset, nl, ps, pi, thr0, words):
        tw, qn, w = group
        if w is None:
            ops.cosine_token_topk(tw, qn, self.tokens, self.norms, k, self.combine, self.eps, idx_offset, nl, ps, pi, thr0, self.top_t,
                                  words)
        else:
            ops.cosine_token_topk_pq(tw, qn, self.tokens, w, k, self.combine, self.eps, idx_offset, nl, ps, pi, thr0, self.top_t, words)


class _DistanceScorer:
    """What is distance about a token search.  A group is (t, c): the raw queries and ``prepare_distance_weights`` of ``weights``
    ([D] shared, or the group's [g, D] rows).  No TokenBank is ever built (there are no norms; ``tb`` is only where the sample comes
    from, or None); keys are negated distances."""
    negate = True
    norms = None

    def __init__(self, tokens, tb, sel, metric, combine, top_t, weights=None):
        self.tokens, self.tb, self.sel, self.metric, self.combine, self.top_t, self.weights = tokens, tb, sel, metric, combine, top_t, weights

    @classmethod
    def of(cls, rq: TokenRequest):
        return cls(rq.tokens, rq.bank, rq.select, rq.metric, rq.combine, rq.top_t, rq.weights)

    def prepare(self, q):
        self.q, self.c = q, prepare_distance_weights(self.weights, q.shape[1], self.tokens.device)

    def group(self, lo, hi):
        return self.q[lo:hi], self.c[lo:hi] if self.c.dim() == 2 else self.c

    def sample(self, images):
        return _floor_sample(self.tb, self.tokens, self.sel, images)[0], None

    def scores(self, group, tokens, norms, out, words=None):
        t, c = group
        op = ops.distance_token_scores if c.dim() == 1 else ops.distance_token_scores_pq
        op(c, t, tokens, self.metric, self.combine, out, self.top_t, words)

    def lists(self, group, k, idx_offset, nl, ps, pi, thr0, words):
        t, c = group
        op = ops.distance_token_topk if c.dim() == 1 else ops.distance_token_topk_pq
        op(c, t, self.tokens, self.metric, self.combine, k, idx_offset, nl, ps, pi, thr0, self.top_t, words)


def _floor_images(N, sel, k, sample_images):
    """The size rule of the token floors: the sample's images (default 256 k), or None when the bank -- under a selection: the
    selected images -- holds fewer than 8 x that and the extra pass would not pay."""
    images = 256 * k if sample_images is None else sample_images
    return None if (N if sel is None else sel.count) < 8 * images else images


def _token_floor(sc, group, k, sample_images=None):
    """[g] floor of the k-th best key of one group (whose first member is its [g, D] queries), or None (``_floor_images``).  The
    sample is scored as the search scores it -- without selection words: it holds selected images only -- and the k-th largest
    key is taken one ulp lower."""
    images = _floor_images(sc.tokens.shape[0], sc.sel, k, sample_images)
    if images is None:
        return None
    st, sn = sc.sample(images)
    keys = torch.empty(group[0].shape[0], st.shape[0], device=group[0].device)
    sc.scores(group, st, sn, keys)
    return _kth_floor(keys.neg_() if sc.negate else keys, k)


def _topk_tokens(rq: TokenRequest, sc, queries, prune, stats, process_group, world_size):
    """The top-k driver: per group of ``step`` queries one floor, one pass over the bank into per-wave lists, one merge; then the
    all-gather and merge across ranks.  Everything runs in key space; the scorer says whether keys are negated on the way out."""
    Q, k, step, dev = rq.Q, rq.k, rq.step, rq.tokens.device
    words = None if rq.select is None else rq.select.words
    q = queries.to(dev, torch.float32).contiguous()
    out_s = torch.empty(Q, k, device=dev)
    out_i = torch.empty(Q, k, device=dev, dtype=torch.int64)
    if Q == 0:                                      # nothing to search for: empty result, no launch
        return out_s, out_i
    sc.prepare(q)
    pruned = False
    for lo in range(0, Q, step):
        group = sc.group(lo, lo + step)
        Qg = min(step, Q - lo)
        thr0 = _token_floor(sc, group, k) if prune else None
        pruned = pruned or thr0 is not None
        nl = ops.cosine_token_topk_chunks(rq.N, rq.P, Qg, rq.D, k)
        ps = torch.empty(Qg, nl, k, device=dev)
        pi = torch.empty(Qg, nl, k, device=dev, dtype=torch.int64)
        sc.lists(group, k, rq.idx_offset, nl, ps, pi, thr0, words)
        ops.topk_merge(ps, pi, Qg, nl, k, out_s[lo:lo + step], out_i[lo:lo + step], torch.empty(Qg, device=dev, dtype=torch.int32))
    if stats is not None:
        stats.update(path="tokens", groups=rq.groups, pruned=pruned)
        if rq.metric is not None:
            stats.update(metric=rq.metric_name)
        if rq.per_query:
            stats.update(per_query_weights=True, group=step)
        if rq.top_t != 0:
            stats.update(top_t=rq.top_t)
        if rq.select is not None:
            stats.update(selected=rq.select.count)
    _gather_merge(out_s, out_i, Q, k, world_size, process_group)        # (of keys)
    return (out_s.neg_() if sc.negate else out_s), out_i                # distances: (-inf, -1) becomes (+inf, -1)


TOKEN_PREFILTER_MIN_Q = 256    # fewest queries sent through the two-stage token route (measured: DESIGN.md section 6, item 17)
TOKEN_MEAN_PREFILTER_MIN_Q = 256   # ... under combine 'mean': the smallest measured Q that beats the grouped route
# ... under combine 'mean' with a Selection that holds the compacted pooled image (Selection.prepare_mean).  NOT MEASURED yet: the
# unselected constant stands in until tools/bench_token_mean_select.py has run
TOKEN_MEAN_SELECT_PREFILTER_MIN_Q = TOKEN_MEAN_PREFILTER_MIN_Q
# ... under 'min' with 1 <= top_t < P: the smallest measured Q that beats the grouped route on every
# leg, measured on banks of 3.07e9 elements (250 000 x 16 x 768 and 62 500 x 64 x 768).  About 4.3 ms of a two-stage call shrink
# neither with Q nor with the bank while a grouped pass shrinks with the bank (at 0.77e9 elements the plain search lost at 64, item
# 19), so a bank below the measured size waits for the Q from which the plain search was measured to win
TOKEN_TOPT_PREFILTER_MIN_Q = 64
TOKEN_TOPT_PREFILTER_MIN_ELEMENTS = 62500 * 64 * 768      # N P D of the smallest bank the constant above was measured on
TOKEN_TOPT_PREFILTER_MIN_Q_SMALL = 256                     # smaller banks


# fewest queries sent through the two-stage weighted-MSE route: the smallest Q of tools/mse_prefilter_crossover.py's grid at which it
# is at least 10 % faster than the grouped route, row-constants launch included (profiles/mse_prefilter_crossover.json; DESIGN.md
# section 6, item 22): 2.0x at 64 (1.05x - 1.07x at 32), measured on a bank of 15 625 x 64 x 768 = 0.77e9 elements.  A two-stage call
# costs about 10 ms there whatever Q is, and that does not shrink with the bank, while a grouped pass does: a bank below the measured
# size has NOT been measured and waits for the grid's largest Q
TOKEN_MSE_PREFILTER_MIN_Q = 64
TOKEN_MSE_PREFILTER_MIN_ELEMENTS = 15625 * 64 * 768       # N P D of the bank the constant above was measured on
TOKEN_MSE_PREFILTER_MIN_Q_SMALL = 1024                    # smaller banks
# ... by opt-in (TokenBank.prepare_mse_top_t, Selection.prepare_mse): distance 'max' under 1 <= top_t < P, a selection of images, and
# both together.  tools/bench_mse_select_topt.py measures them against the grouped route on the bank above (its legs: top_t = 4, a
# 10 % selection scattered and in runs of 4096 rows, both); each constant is the smallest Q of its grid at which the route is at least
# 10 % faster on every leg that exercises it, both dtypes, preparation launches included (profiles/mse_select_topt_crossover.json and
# its repeat).  Measured: 32, the grid's smallest point, for all three -- 1.12x under top_t (in both runs
# and both dtypes, 1 % above the margin), 1.30x - 1.41x under the scattered selection, 1.88x - 2.09x under the runs.  Smaller banks are
# NOT MEASURED: TOKEN_MSE_PREFILTER_MIN_Q_SMALL, as above
TOKEN_MSE_TOPT_PREFILTER_MIN_Q = 32
TOKEN_MSE_SELECT_PREFILTER_MIN_Q = 32
TOKEN_MSE_SELECT_TOPT_PREFILTER_MIN_Q = 32
# ... with per-query weights [Q, D], by opt-in (TokenBank.prepare_mse_per_query): stage 1 multiplies a second image of the bank with
# rows of 2 D, twice the k-steps of the shared-weight route, against a grouped route that takes at most 16 queries per bank pass.
# tools/bench_mse_per_query.py measures it against the grouped per-query route on the bank above (Q in 16 .. 1024, 'min' and 'max',
# both dtypes, query preparation and the first-threshold sample included, the one-off image build -- about 1 ms -- apart); the
# constant is the smallest Q of its grid from which the route is at least 10 % faster in both of two runs
# (profiles/mse_per_query_crossover.json and its repeat).  Measured: 128, decided by bf16 -- 1.51x - 1.52x
# there (fp16: 2.36x - 2.39x), 2.28x - 2.30x at 256 (3.3x - 3.5x), 1.76x - 1.80x at 1024 (2.9x - 3.0x); at 64 fp16 wins by 1.53x -
# 1.58x but bf16, whose bound is the wider one (unit roundoff 2^-8), loses (0.89x - 0.91x), and one constant serves both dtypes.
# Smaller banks are NOT MEASURED: TOKEN_MSE_PREFILTER_MIN_Q_SMALL, as above
TOKEN_MSE_PQ_PREFILTER_MIN_Q = 128
# ... under combine 'mean', by opt-in (TokenBank.prepare_mse_mean): stage 1 walks a pooled image of N rows, not N P.
# tools/bench_mse_mean.py measures it against the grouped route on two banks of the size above, [15625, 64, 768] and [250000, 4, 768]
# (Q in 16 .. 1024, k = 100, both dtypes, query preparation, the first-threshold sample and the row-constants launch included, the
# one-off pooling pass -- 0.8 - 1.1 ms -- apart); the constant is the smallest Q of its grid from which the route is at least 10 %
# faster in both of two runs, on every bank and dtype (profiles/mse_mean_crossover.json and its repeat).
# Measured: 64, decided by the P = 64 bank -- 1.94x - 2.02x there (1.01x - 1.05x at 32, 0.58x - 0.59x at 16), 5.2x - 5.5x at 256,
# 4.6x - 4.9x at 1024; the P = 4 bank wins from the grid's smallest point (2.5x at 16, 6.5x at 64, 12.6x - 12.9x at 1024): a call costs
# about 2 ms there against about 9.5 ms on the P = 64 bank, whose candidates cost 64 token rows each.  Smaller banks are NOT MEASURED:
# TOKEN_MSE_PREFILTER_MIN_Q_SMALL, as above
TOKEN_MSE_MEAN_PREFILTER_MIN_Q = 64


def _token_mse_prefilter_refusal(rq: TokenRequest):
    """``_token_prefilter_refusal`` for a distance request over a resident 16-bit bank: None when ``distance_topk_tokens`` serves it
    by the two-stage route (metric MSE, combine min | max, shared weights -- per-query weights only over a bank asked by
    ``TokenBank.prepare_mse_per_query``, without ``top_t`` and ``select`` --, P a divisor of 64, the library's shape rule, the switch
    on, enough queries; ``top_t`` only over a bank asked by ``TokenBank.prepare_mse_top_t``, ``select`` only as a Selection asked by
    ``Selection.prepare_mse`` for this bank), else the first reason why the grouped route serves it."""
    name = next((n for n, code in ops.METRIC_CODES.items() if code == rq.metric), rq.metric_name)
    tb, sel = rq.bank, rq.select
    held = getattr(sel, "_mse", None)                      # (getattr: a Selection may be built without __init__, a bank too)
    asked = isinstance(sel, Selection) and held is not None and tb in held
    why = token_mse_route_refusal(rq.Q, rq.N, rq.P, rq.D, rq.k, name, rq.combine, rq.top_t, sel is not None, rq.per_query,
                                  top_t_prepared=bool(getattr(tb, "_mse_top_t", False)), select_prepared=asked,
                                  selected=sel.count if asked else None, per_query_prepared=getattr(tb, "_mse_pq", None) is not None,
                                  mean_prepared=getattr(tb, "_mse_mean", None) is not None)
    if why == "select under a distance metric" and isinstance(sel, Selection):
        why += " without the masked row constants of this bank (opt in once per Selection and bank: Selection.prepare_mse)"
    return why


def token_mse_route_refusal(Q, N, P, D, k, metric, combine, top_t=0, select=False, per_query=False, *, top_t_prepared=False,
                            select_prepared=False, selected=None, per_query_prepared=False, mean_prepared=False):
    """The same decision from the request's plain facts, for a caller that has not wrapped its bank yet (``similarity_search.py``
    builds a ``TokenBank.resident`` -- a norm pass over the bank -- only when this returns None): ``metric`` a name, ``combine`` a
    name or an ``ops.COMBINE_CODES`` code, ``top_t`` None / 0 for all tokens, ``select`` whether there is a selection.  The bank is
    taken to be a 16-byte aligned fp16 / bf16 tensor.  No device work.

    ``top_t_prepared`` / ``select_prepared`` (keyword only; False: the answers as they ever were): the caller will opt in by
    ``TokenBank.prepare_mse_top_t`` / ``Selection.prepare_mse``, and the request is then decided under ``top_t`` / the selection:
    the library's range for ``top_t``, the smallest Q of the route the request takes, and with ``selected`` (the number of selected
    images; None: not looked at) the rule that the selected images are themselves a bank the route takes.

    ``per_query_prepared`` (keyword only; False: the answers as they ever were): the caller will opt in by
    ``TokenBank.prepare_mse_per_query``, and a request with per-query weights is then decided by that route's rule -- no ``top_t`` and
    no ``select`` (with either the answer stays "per-query weights"), D % 32 == 0 and 128 <= D <= 2048 (stage 1 multiplies rows of
    2 D), and ``TOKEN_MSE_PQ_PREFILTER_MIN_Q`` as the smallest Q.

    ``mean_prepared`` (keyword only; False: the answers as they ever were): the caller will opt in by
    ``TokenBank.prepare_mse_mean``, and ``combine='mean'`` is then decided by that route's rule -- no ``top_t``, no ``select`` and no
    per-query weights (with any of them the answer stays "combine 'mean' under a distance metric"), P a divisor of 64, the switch on,
    the library's shape rule with N >= 2048 IMAGES (stage 1 walks the pooled image), and ``TOKEN_MSE_MEAN_PREFILTER_MIN_Q`` as the
    smallest Q."""
    combine = ops.COMBINE_CODES.get(combine, combine)
    if metric != 'MSE':
        return f"metric {metric} (a distance that is no dot product)"
    if combine == ops.COMBINE_CODES['mean']:
        if not mean_prepared or top_t or select or per_query:
            return "combine 'mean' under a distance metric"
        if P < 1 or 64 % P:
            return f"P = {P} does not divide 64"
        if not _prefilter_enabled():
            return "SKYEMB_TOPK_PREFILTER=0"
        why = ops.token_mse_mean_prefilter_refusal(Q, N, P, D, k)         # the library's shape rule first, then the smallest Q
        if why is not None:
            return why
        if N * P * D >= TOKEN_MSE_PREFILTER_MIN_ELEMENTS:
            if Q < TOKEN_MSE_MEAN_PREFILTER_MIN_Q:
                return f"Q = {Q} < TOKEN_MSE_MEAN_PREFILTER_MIN_Q = {TOKEN_MSE_MEAN_PREFILTER_MIN_Q}"
        elif Q < TOKEN_MSE_PREFILTER_MIN_Q_SMALL:
            return (f"Q = {Q} < TOKEN_MSE_PREFILTER_MIN_Q_SMALL = {TOKEN_MSE_PREFILTER_MIN_Q_SMALL} (a bank of fewer than "
                    f"TOKEN_MSE_PREFILTER_MIN_ELEMENTS = {TOKEN_MSE_PREFILTER_MIN_ELEMENTS} elements)")
        return None
    if top_t and not top_t_prepared:
        return "top_t under a distance metric"
    if select and not select_prepared:
        return "select under a distance metric"
    if per_query and (not per_query_prepared or top_t or select):
        return "per-query weights"
    if P < 1 or 64 % P:
        return f"P = {P} does not divide 64"
    if not _prefilter_enabled():
        return "SKYEMB_TOPK_PREFILTER=0"
    if per_query:                                          # its own smallest Q and its own shape rule (rows of 2 D)
        if N * P * D >= TOKEN_MSE_PREFILTER_MIN_ELEMENTS:
            if Q < TOKEN_MSE_PQ_PREFILTER_MIN_Q:
                return f"Q = {Q} < TOKEN_MSE_PQ_PREFILTER_MIN_Q = {TOKEN_MSE_PQ_PREFILTER_MIN_Q}"
        elif Q < TOKEN_MSE_PREFILTER_MIN_Q_SMALL:
            return (f"Q = {Q} < TOKEN_MSE_PREFILTER_MIN_Q_SMALL = {TOKEN_MSE_PREFILTER_MIN_Q_SMALL} (a bank of fewer than "
                    f"TOKEN_MSE_PREFILTER_MIN_ELEMENTS = {TOKEN_MSE_PREFILTER_MIN_ELEMENTS} elements)")
        return ops.token_mse_pq_prefilter_refusal(Q, N, P, D, k)
    if top_t:
        why = ops.token_mse_topt_prefilter_refusal(Q, N, P, D, k, combine, top_t)
        if why is not None:
            return why
    # distance 'min' under any top_t and 'max' under top_t == P ARE the plain search (ops.token_mse_topt_folds): its smallest Q
    top = bool(top_t) and ops.token_mse_topt_folds(P, combine, top_t)[1] == 'top'
    name = "TOKEN_MSE" + ("_SELECT" if select else "") + ("_TOPT" if top else "") + "_PREFILTER_MIN_Q"
    if N * P * D >= TOKEN_MSE_PREFILTER_MIN_ELEMENTS:
        if Q < globals()[name]:
            return f"Q = {Q} < {name} = {globals()[name]}"
    elif Q < TOKEN_MSE_PREFILTER_MIN_Q_SMALL:
        return (f"Q = {Q} < TOKEN_MSE_PREFILTER_MIN_Q_SMALL = {TOKEN_MSE_PREFILTER_MIN_Q_SMALL} (a bank of fewer than "
                f"TOKEN_MSE_PREFILTER_MIN_ELEMENTS = {TOKEN_MSE_PREFILTER_MIN_ELEMENTS} elements)")
    why = ops.token_mse_prefilter_refusal(Q, N, P, D, k)
    if why is None and select and selected is not None:
        # the selection must itself be a bank the route takes (k <= selected images, selected images x P >= 2048 rows): then the
        # bootstrap sample exists, and the grouped route is cheap in exactly the cases refused here
        why = ops.token_mse_prefilter_refusal(Q, selected, P, D, k)
        why = why if why is None else "the selected images alone: " + why
    return why


def _token_prefilter_refusal(rq: TokenRequest):
    """None when ``cosine_topk_tokens`` (a distance request: ``distance_topk_tokens``) serves the request by the two-stage route,
    else the first reason why the grouped route serves it.  A pure function of the request (and the bank it names): no device work."""
    tb = rq.bank
    if tb is not None and getattr(tb, "dtype", None) == torch.float32:
        return "an fp32 token bank"
    if tb is None or not getattr(tb, "_resident", False):
        return "the bank was not made by TokenBank.resident"
    if rq.metric is not None:
        return _token_mse_prefilter_refusal(rq)
    mean = rq.combine == ops.COMBINE_CODES['mean']
    if rq.top_t != 0 and mean:
        return "top_t under combine 'mean'"
    if mean and rq.select is not None:
        held = getattr(rq.select, "_mean", None)           # (getattr: a Selection may be built without __init__)
        if not isinstance(rq.select, Selection) or held is None or tb not in held:
            return ("select under combine 'mean' without the compacted pooled image of this bank (opt in once per Selection and bank: "
                    "Selection.prepare_mean)")
    if rq.select is not None and not isinstance(rq.select, Selection):
        return "select is not a Selection"
    if rq.per_query:
        return "per-query weights"
    if rq.P < 1 or 64 % rq.P:
        return f"P = {rq.P} does not divide 64"
    if not _prefilter_enabled():
        return "SKYEMB_TOPK_PREFILTER=0"
    if mean and rq.select is not None:                     # stage 1 walks the selected images' compacted pooled rows
        if rq.Q < TOKEN_MEAN_SELECT_PREFILTER_MIN_Q:
            return f"Q = {rq.Q} < TOKEN_MEAN_SELECT_PREFILTER_MIN_Q = {TOKEN_MEAN_SELECT_PREFILTER_MIN_Q}"
        why = ops.token_mean_prefilter_refusal(rq.Q, rq.N, rq.P, rq.D, rq.k)
        if why is None:
            why = ops.token_mean_select_prefilter_refusal(rq.Q, rq.select.count, rq.P, rq.D, rq.k)
            why = why if why is None else "the selected images alone: " + why
        return why
    if mean:                                               # its own size and shape rule: stage 1 walks images, not token rows
        if rq.Q < TOKEN_MEAN_PREFILTER_MIN_Q:
            return f"Q = {rq.Q} < TOKEN_MEAN_PREFILTER_MIN_Q = {TOKEN_MEAN_PREFILTER_MIN_Q}"
        return ops.token_mean_prefilter_refusal(rq.Q, rq.N, rq.P, rq.D, rq.k)
    if rq.top_t != 0:
        why = ops.token_topt_prefilter_refusal(rq.Q, rq.N, rq.P, rq.D, rq.k, rq.combine, rq.top_t)
        if why is not None:
            return why
    # 'max' under any top_t and 'min' under top_t == P ARE the plain search (ops.token_topt_folds): its threshold; the top-t folds
    # have their own
    if rq.top_t != 0 and ops.token_topt_folds(rq.P, rq.combine, rq.top_t)[1] == 'top':
        if rq.N * rq.P * rq.D >= TOKEN_TOPT_PREFILTER_MIN_ELEMENTS:
            if rq.Q < TOKEN_TOPT_PREFILTER_MIN_Q:
                return f"Q = {rq.Q} < TOKEN_TOPT_PREFILTER_MIN_Q = {TOKEN_TOPT_PREFILTER_MIN_Q}"
        elif rq.Q < TOKEN_TOPT_PREFILTER_MIN_Q_SMALL:
            return (f"Q = {rq.Q} < TOKEN_TOPT_PREFILTER_MIN_Q_SMALL = {TOKEN_TOPT_PREFILTER_MIN_Q_SMALL} (a bank of fewer than "
                    f"TOKEN_TOPT_PREFILTER_MIN_ELEMENTS = {TOKEN_TOPT_PREFILTER_MIN_ELEMENTS} elements)")
    elif rq.Q < TOKEN_PREFILTER_MIN_Q:
        return f"Q = {rq.Q} < TOKEN_PREFILTER_MIN_Q = {TOKEN_PREFILTER_MIN_Q}"
    why = ops.token_prefilter_refusal(rq.Q, rq.N, rq.P, rq.D, rq.k)
    if why is None and rq.select is not None:
        # the selection must itself be a bank the route takes (k <= selected images, selected images x P >= 2048 rows): then the
        # bootstrap sample exists, and the grouped route is cheap in exactly the cases refused here
        why = ops.token_prefilter_refusal(rq.Q, rq.select.count, rq.P, rq.D, rq.k)
        why = why if why is None else "the selected images alone: " + why
    return why


def _bootstrap_floor(rq: TokenRequest, tw, qn, eps):
    """[Q] the k-th best combined score of every query over a strided sample of min(N, max(16 k, 256)) whole images, scored by
    the grouped kernels, one ulp lower: the two-stage route's first threshold, a lower bound of the k-th best over the bank.  Under
    a selection the sample is min(count, max(16 k, 256)) SELECTED images (``Selection.sample``, kept there per bank and weights
    version): a lower bound of the k-th best selected score.  The sample is scored under the request's ``top_t``: d[top_t-1] of
    a sample is a lower bound of the k-th best d[top_t-1] over the bank, and -- d[top_t-1] >= the plain min -- a higher floor than the
    plain min's, which would be valid too but admit every image whose top_t-th token, not its worst, reaches the sample's k-th worst."""
    tb, k = rq.bank, rq.k
    if rq.select is not None:
        S = min(rq.select.count, max(16 * k, 256))
        st, sn = rq.select.sample(tb, S)
    else:
        S = min(rq.N, max(16 * k, 256))
        st, sn = tb.sample(S, "bootstrap")
    floor = torch.empty(rq.Q, device=tw.device)
    keys = torch.empty(16, S, device=tw.device)
    for lo in range(0, rq.Q, 16):
        g = min(16, rq.Q - lo)
        ops.cosine_token_scores(tw[lo:lo + g], qn[lo:lo + g], st, sn, rq.combine, eps, keys[:g], rq.top_t, None)
        ops.kth_largest_floor(keys[:g], k, floor[lo:lo + g])
    return floor


def _topk_tokens_prefiltered(rq: TokenRequest, eps, queries, prune, stats, process_group, world_size):
    """The two-stage driver (csrc/topk_prefilter.hip, "Patch-token banks"): one bootstrap floor, one stage-1 pass with exact
    re-scoring after every slice; flagged queries go through the grouped route, those queries only.  Under a selection stage 1
    walks the live tiles of ``Selection.token_prefilter``; its first slice ends at the first live-tile position whose count of
    selected images reaches 96 k (never less than n_live / 128 positions, never less than 1), and the re-run keeps the selection.
    Under 'mean' a selection is served by compaction instead (``Selection.mean_prefilter``): stage 1 is the unselected mean pass over
    the selected images' pooled rows, stage 2 follows the map back to the bank."""
    tb, Q, k, dev, sel = rq.bank, rq.Q, rq.k, rq.tokens.device, rq.select
    mean = rq.combine == ops.COMBINE_CODES['mean']
    q = queries.to(dev, torch.float32).contiguous()
    tw, qn = prepare_queries(q, tb.weights)
    thr0 = _bootstrap_floor(rq, tw, qn, eps)
    prepared = None if sel is None or mean else sel.token_prefilter(tb)
    head, eps_off = (tw, qn, tb.bank, tb.norms), (eps, rq.idx_offset)

    def launch(*out):                                      # ``top_t`` follows ``combine`` in the calls that take it
        if mean and sel is not None:                       # stage 1 over the selected images' compacted pooled rows
            return ops.cosine_topk_tokens_mean_prefiltered_sel(*head, *sel.mean_prefilter(tb), k, *eps_off, *out, thr0)
        if mean:                                           # stage 1 over the pooled image
            return ops.cosine_topk_tokens_mean_prefiltered(*head, *tb.stage1_mean(), k, *eps_off, *out, thr0)
        tail, rowp = tb.stage1()
        fold = (rq.combine,) if rq.top_t == 0 else (rq.combine, rq.top_t)
        if sel is None:
            op = ops.cosine_topk_tokens_prefiltered if rq.top_t == 0 else ops.cosine_topk_tokens_prefiltered_top
            return op(*head, tail, rowp, k, *fold, *eps_off, *out, thr0)
        n_live, cum = prepared[2], prepared[4]
        direct_end = min(max(bisect.bisect_left(cum, 96 * k) + 1, n_live // 128, 1), n_live)
        op = ops.cosine_topk_tokens_prefiltered_sel if rq.top_t == 0 else ops.cosine_topk_tokens_prefiltered_top_sel
        op(*head, tail, prepared, direct_end, k, *fold, *eps_off, *out, thr0)

    def rerun(again):                                      # the grouped route; every other field, top_t and select among them, is carried over
        rq2 = dataclasses.replace(rq, Q=int(again.numel()))
        return _topk_tokens(rq2, _CosineScorer.of(rq2, eps), q.index_select(0, again), prune, None, None, 1)

    out_s, out_i, n_redo = _two_stage(Q, k, dev, launch, rerun)
    if stats is not None:
        stats.update(path="prefiltered", redone=n_redo, combine=next(name for name, code in ops.COMBINE_CODES.items() if code == rq.combine))
        if rq.top_t != 0:
            stats.update(top_t=rq.top_t)
        if sel is not None and mean:
            stats.update(selected=sel.count, compacted=(sel.count, rq.N))
        elif sel is not None:
            stats.update(selected=sel.count, tiles=(prepared[2], (rq.N * rq.P + 255) // 256))
    return _gather_merge(out_s, out_i, Q, k, world_size, process_group)


def _score_tokens(rq: TokenRequest, sc, queries):
    """The scores driver: [Q, N], one pass over the bank per group of ``step`` queries, written straight into its rows."""
    words = None if rq.select is None else rq.select.words
    q = queries.to(rq.tokens.device, torch.float32).contiguous()
    out = torch.empty(rq.Q, rq.N, device=rq.tokens.device)
    if rq.Q == 0:
        return out
    sc.prepare(q)
    for lo in range(0, rq.Q, rq.step):
        sc.scores(sc.group(lo, lo + rq.step), rq.tokens, sc.norms, out[lo:lo + rq.step], words)
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
    who = "token_pruning_floor"
    bank, tokens = _unwrap(tb)
    t = _top_t_arg(top_t, tokens.shape[1], who)
    W = _weights_arg(weights, tw.shape[0], tw.shape[1], who)
    sel = _selection_arg(select, tokens.shape[0], who, tokens.device)
    if _floor_images(tokens.shape[0], sel, k, sample_images) is None:     # before ``combine`` is read, as it ever was
        return None
    if W is not None:
        W = W.to(tw.device, torch.float32).contiguous()
    # shared weights take the sample from ``tb`` itself: a TokenBank, and anything else fails there, as it ever did
    sc = _CosineScorer(tokens, tb if W is None else bank, sel, _combine_code(combine, who), t, eps, W)
    return _token_floor(sc, (tw, qn, W), k, sample_images)


def cosine_topk_tokens(queries: torch.Tensor, bank, k: int, combine: str = 'min', weights: torch.Tensor | None = None,
                       eps: float = 1e-6, process_group=None, world_size: int = 1, prune: bool = True, stats: dict | None = None,
                       top_t: int | None = None, select=None):
    """-> (scores f32 [Q,k], image indices i64 [Q,k]): exact top-k images by the combined score of their P patch tokens
    (reference: compute_similarity with max_pool = False, utils/similarity.py:214-268, + update_best_scores), order
    (score desc, image asc).  ``bank`` is a [N,P,D] tensor (fp32, or fp16 / bf16: see TokenBank) or a TokenBank (this rank's
    shard of images; ``idx_offset`` = first global image of the shard).  One pass over the bank per group of at most 16 queries
    (Q > 16 runs ceil(Q / 16) passes) -- the grouped route, ``stats['path'] == 'tokens'``.

    Two-stage route (``stats['path'] == 'prefiltered'``): a ``TokenBank.resident(bank)`` (fp16 / bf16) with ``combine`` 'min' or
    'max', shared weights, P a divisor of 64, at least ``TOKEN_PREFILTER_MIN_Q`` queries, a shape the
    library takes (D % 32 == 0, 128 <= D <= 4096, 2048 <= N P < 2^31, k <= 256, k <= N) and SKYEMB_TOPK_PREFILTER not 0 is searched
    in ONE pass for all queries: the bank's rows are multiplied on the 16-bit matrix cores with a proven error bound, an image is
    a candidate when every ('min') / some ('max') token of it can still reach the query's threshold, and every candidate is
    re-scored exactly after each slice of the bank, which also makes the threshold exact.  Scores and indices are bit for bit
    those of the grouped route over the same bank in a plain ``TokenBank``.  ``stats`` gains ``redone`` (queries whose candidate
    list was full, re-run by the grouped route) and ``combine``.  With ``select`` the route is taken when the selected images are
    themselves a bank it takes (k <= selected images, selected images x P >= 2048 rows): stage 1 then reads only the 256-row tiles
    that hold a selected image, every row of a deselected image fails its test whatever it holds, the first threshold comes from
    a sample of selected images, and a re-run keeps the selection; ``stats`` gains ``selected`` and ``tiles`` = (live tiles, all
    tiles).  What the selection needs is kept in the ``Selection`` per bank (``Selection.token_prefilter``): pass the same object to
    repeated searches.  ``combine`` 'mean' takes the route by a stage 1 of its own: the mean of an image's token cosines is, up to
    ``eps`` and rounding, one dot product with the image's pooled unit tokens, so the matrix cores multiply a derived 16-bit image
    [N, D] of them (``TokenBank.stage1_mean``, one launch per bank and weights version) under a proven bound U >= mean, and every
    candidate image's P tokens are re-scored exactly, folded in token order with the one division -- bit for bit the grouped
    route.  Its rule: no ``top_t``, shared weights, P a divisor of 64, at least ``TOKEN_MEAN_PREFILTER_MIN_Q``
    queries, D % 32 == 0, 128 <= D <= 4096, N >= 2048 images, N P < 2^31, k <= 256, k <= N.  ``select`` under 'mean' takes the route
    by opt-in only: a ``Selection`` that was asked to hold the compacted pooled image of this bank
    (``Selection(flags).prepare_mean(bank)``: the selected images' pooled rows and constants gathered into an image [count, D] by one
    short launch, 2 D + 20 bytes per selected image and one 256-row tail tile, kept per bank and rebuilt when its weights change).
    Stage 1 is then the unselected mean pass over ``count`` rows, not N -- its work falls with the selection however the images are
    scattered --, a deselected image appears nowhere, stage 2 follows the map back to the bank; ``stats`` gains ``selected`` and
    ``compacted`` = (count, N).  Its rule: the rule above on the bank, the same rule with ``count`` for N (count >= 2048, k <= count)
    and at least ``TOKEN_MEAN_SELECT_PREFILTER_MIN_Q`` queries.  A bool tensor or a Selection never asked keeps the grouped route:
    the gather costs memory and a launch that only repeated searches under one Selection amortise.  Everything else is served by the grouped
    route as ever, never refused.  ``top_t`` under 'min' and 'max', alone and with ``select``, takes the route too: 'max' with any
    ``top_t`` and 'min' with ``top_t == P`` are the plain search; 'min' with 1 <= top_t < P scores d[top_t-1], which reaches a
    threshold only when at least top_t tokens do, so an image is a candidate when the COUNT of its rows that pass the row test is
    >= top_t, and stage 2 sorts its exact token scores with the grouped kernels' own network -- bit for bit the grouped route; the
    first threshold comes from a sample scored under the same ``top_t``, a re-run keeps it, ``stats`` gains ``top_t``, and the
    smallest Q is ``TOKEN_TOPT_PREFILTER_MIN_Q`` (a bank of fewer than ``TOKEN_TOPT_PREFILTER_MIN_ELEMENTS`` elements:
    ``TOKEN_TOPT_PREFILTER_MIN_Q_SMALL``).  Out of scope for the two-stage route: ``top_t`` under 'mean' (the mean of the
    top_t best is not bounded by a count), per-query weights (the row norm sum w_qd x_d^2 sits under a square root in the
    denominator, so no single dot product bounds the score; ``distance_topk_tokens`` with 'MSE' does take them, by opt-in), fp32
    token banks, P not dividing 64, and
    ``select`` under 'mean' without ``Selection.prepare_mean``.

    Images whose combined score is -inf (a NaN token under min / mean)
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
    rq = _token_request("cosine_topk_tokens", queries, bank, k, combine, _COSINE, weights, top_t, select, world_size)
    if _token_prefilter_refusal(rq) is None:
        return _topk_tokens_prefiltered(rq, eps, queries, prune, stats, process_group, world_size)
    return _topk_tokens(rq, _CosineScorer.of(rq, eps), queries, prune, stats, process_group, world_size)


def cosine_token_scores(queries: torch.Tensor, bank, combine: str = 'min', weights: torch.Tensor | None = None, eps: float = 1e-6,
                        top_t: int | None = None, select=None):
    """[Q, N] combined score of every image of a [N,P,D] token bank (fp32, fp16 or bf16; or a TokenBank), in groups of at most
    16 queries.
    ``weights`` is ignored when ``bank`` is a TokenBank (it carries its own).  ``top_t``: as for ``cosine_topk_tokens`` (None:
    all tokens; else only the top_t best token scores of an image count, mean summed largest first -- so 'mean' with
    ``top_t == P`` is not the plain mean).  ``select``: as for ``cosine_topk_tokens``; every [Q, N] slot is written, a deselected
    image gets -inf.  ``weights`` [Q, D]: per-query weights, as for ``cosine_topk_tokens`` (groups of g queries at k = 1)."""
    rq = _token_request("cosine_token_scores", queries, bank, None, combine, _COSINE, weights, top_t, select)
    return _score_tokens(rq, _CosineScorer.of(rq, eps), queries)


# ------------------------------------------------------------------------------------------------
# the distance metrics (weighted MSE / MAE, utils/similarity.py:174-212) over the same token banks: smaller is better
# ------------------------------------------------------------------------------------------------
def distance_pruning_floor(c, t, bank, k: int, metric: str = 'MAE', combine: str = 'mean', sample_images: int | None = None,
                           top_t: int | None = None, select=None):
    """``token_pruning_floor`` for the distance metrics, in KEY space (key = -distance): the same sample of whole images (the
    selection's own under ``select``) is scored by the distance kernel, negated, and its k-th largest key, one ulp lower, is a
    floor of the k-th best key of the search.  None under the same size rule (fewer than 8 x the sample's images).  ``c``:
    ``prepare_distance_weights`` ([D], or [Q, D] with one row per query of ``t``); ``t`` [Q <= 16, D]; ``bank``: a [N,P,D] tensor or
    a TokenBank."""
    who = "distance_pruning_floor"
    tb, tokens = _unwrap(bank)
    tt = _top_t_arg(top_t, tokens.shape[1], who)
    if tuple(c.shape) not in ((t.shape[1],), tuple(t.shape)):
        raise ValueError(f"distance_pruning_floor: c has shape {tuple(c.shape)}, expected ({t.shape[1]},) or {tuple(t.shape)} for "
                         f"queries of shape {tuple(t.shape)}")
    mcode, ccode = _metric_code(metric, who), _combine_code(combine, who)
    sel = _selection_arg(select, tokens.shape[0], who, tokens.device)
    return _token_floor(_DistanceScorer(tokens, tb, sel, mcode, ccode, tt), (t, c), k, sample_images)


def _topk_tokens_mse_prefiltered(rq: TokenRequest, queries, prune, stats, process_group, world_size):
    """The two-stage driver of ``distance_topk_tokens`` (csrc/topk_prefilter.hip, "Weighted MSE"): the first threshold is
    ``distance_pruning_floor``'s -- the k-th best key of a strided sample of min(N, max(16 k, 256)) whole images, scored by the
    grouped kernel in groups of 16 queries, one ulp lower --, then one stage-1 pass for all queries with exact re-scoring after
    every slice; flagged queries go through the grouped route, those queries only.  Everything runs in key space (key = -distance)
    until the result is negated on the way out.  Under ``top_t`` the sample is scored under it; under a selection the sample is of
    SELECTED images, stage 1 walks the live tiles of ``Selection.mse_prefilter`` and its first slice ends where ``cum`` says the
    cosine driver's would (``_topk_tokens_prefiltered``); the re-run keeps both.  Under ``combine='mean'`` (a bank asked by
    ``TokenBank.prepare_mse_mean``; "Weighted MSE under combine 'mean'" there) stage 1 walks the pooled image of
    ``TokenBank.stage1_mse_mean``; the sample is scored under 'mean' and the re-run keeps it."""
    tb, Q, k, dev, sel = rq.bank, rq.Q, rq.k, rq.tokens.device, rq.select
    q = queries.to(dev, torch.float32).contiguous()
    c = prepare_distance_weights(rq.weights, rq.D, dev)
    mean = rq.combine == ops.COMBINE_CODES['mean']         # (no top_t and no selection reach here with it: token_mse_route_refusal)
    if mean:
        pooled, tail, rowp = tb.stage1_mse_mean(c)
    else:
        tail, rowp = tb.stage1_mse(c)
    # (a selection that reaches this driver holds at least 2048 token rows -- the route's shape rule on the selected images alone --,
    # and 7 whole 256-row tiles and a tail tile hold 2047 at most: it has SELECT_MIN_LIVE_TILES live whole tiles, nothing to check)
    prepared = None if sel is None else sel.mse_prefilter(tb, c)
    # the floor: the sample of SELECTED images under a selection, scored under the request's top_t (a[top_t-1] of a sample bounds the
    # k-th best a[top_t-1] of the search)
    S = min(rq.N if sel is None else sel.count, max(16 * k, 256))
    st = tb.sample(S, "bootstrap")[0] if sel is None else sel.sample(tb, S)[0]
    thr0 = torch.empty(Q, device=dev)
    keys = torch.empty(16, S, device=dev)
    for lo in range(0, Q, 16):
        g = min(16, Q - lo)
        ops.distance_token_scores(c, q[lo:lo + g], st, rq.metric, rq.combine, keys[:g], rq.top_t)
        ops.kth_largest_floor(keys[:g].neg_(), k, thr0[lo:lo + g])

    def launch(*out):                                      # ``top_t`` follows ``combine`` in the calls that take it
        if mean:
            return ops.distance_topk_tokens_mean_prefiltered(c, q, tb.bank, pooled, tail, rowp, k, rq.idx_offset, *out, thr0)
        if sel is None and rq.top_t == 0:
            return ops.distance_topk_tokens_prefiltered(c, q, tb.bank, tail, rowp, k, rq.combine, rq.idx_offset, *out, thr0)
        if sel is None:
            return ops.distance_topk_tokens_prefiltered_top(c, q, tb.bank, tail, rowp, k, rq.combine, rq.top_t, rq.idx_offset, *out, thr0)
        n_live, cum = prepared[2], prepared[4]
        direct_end = min(max(bisect.bisect_left(cum, 96 * k) + 1, n_live // 128, 1), n_live)
        return ops.distance_topk_tokens_prefiltered_top_sel(c, q, tb.bank, tail, prepared, direct_end, k, rq.combine, rq.top_t,
                                                            rq.idx_offset, *out, thr0)

    def rerun(again):                                      # the grouped route, in key space like ``launch``'s result
        rq2 = dataclasses.replace(rq, Q=int(again.numel()))
        s2, i2 = _topk_tokens(rq2, _DistanceScorer.of(rq2), q.index_select(0, again), prune, None, None, 1)
        return s2.neg_(), i2

    out_s, out_i, n_redo = _two_stage(Q, k, dev, launch, rerun)
    if stats is not None:
        stats.update(path="prefiltered", redone=n_redo, metric=rq.metric_name,
                     combine=next(name for name, code in ops.COMBINE_CODES.items() if code == rq.combine))
        if rq.top_t != 0:
            stats.update(top_t=rq.top_t)
        if sel is not None:
            stats.update(selected=sel.count, tiles=(prepared[2], (rq.N * rq.P + 255) // 256))
    _gather_merge(out_s, out_i, Q, k, world_size, process_group)        # (of keys)
    return out_s.neg_(), out_i                                          # (-inf, -1) becomes (+inf, -1)


def _topk_tokens_mse_pq_prefiltered(rq: TokenRequest, queries, prune, stats, process_group, world_size):
    """``_topk_tokens_mse_prefiltered`` with per-query weights (csrc/topk_prefilter.hip, "Weighted MSE with PER-QUERY weights"):
    stage 1 multiplies the bank's second image [x ; x o x] (``TokenBank.prepare_mse_per_query``) by query images built from
    [c_q o t_q ; -c_q / 2], stage 2 re-scores candidates under row q of c.  The first threshold comes from the same strided sample
    of min(N, max(16 k, 256)) whole images, scored by the grouped per-query kernel in groups of ``rq.step`` (``_pq_group``) queries;
    flagged queries are re-run by the grouped per-query route, those queries only, each with its own weight row."""
    tb, Q, k, dev = rq.bank, rq.Q, rq.k, rq.tokens.device
    q = queries.to(dev, torch.float32).contiguous()
    W = rq.weights.to(dev, torch.float32).contiguous()
    c = prepare_distance_weights(W, rq.D, dev)
    image, rowp = tb._mse_pq
    S = min(rq.N, max(16 * k, 256))
    st = tb.sample(S, "bootstrap")[0]
    thr0 = torch.empty(Q, device=dev)
    keys = torch.empty(rq.step, S, device=dev)
    for lo in range(0, Q, rq.step):
        g = min(rq.step, Q - lo)
        ops.distance_token_scores_pq(c[lo:lo + g], q[lo:lo + g], st, rq.metric, rq.combine, keys[:g], 0, None)
        ops.kth_largest_floor(keys[:g].neg_(), k, thr0[lo:lo + g])

    def launch(*out):
        return ops.distance_topk_tokens_prefiltered_pq(c, q, tb.bank, image, rowp, k, rq.combine, rq.idx_offset, *out, thr0)

    def rerun(again):                                      # the grouped per-query route, in key space like ``launch``'s result
        rq2 = dataclasses.replace(rq, Q=int(again.numel()), weights=W.index_select(0, again))
        s2, i2 = _topk_tokens(rq2, _DistanceScorer.of(rq2), q.index_select(0, again), prune, None, None, 1)
        return s2.neg_(), i2

    out_s, out_i, n_redo = _two_stage(Q, k, dev, launch, rerun)
    if stats is not None:
        stats.update(path="prefiltered", per_query_weights=True, redone=n_redo, metric=rq.metric_name,
                     combine=next(name for name, code in ops.COMBINE_CODES.items() if code == rq.combine))
    _gather_merge(out_s, out_i, Q, k, world_size, process_group)        # (of keys)
    return out_s.neg_(), out_i                                          # (-inf, -1) becomes (+inf, -1)


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

    Two-stage route (``stats['path'] == 'prefiltered'``): metric 'MSE' with ``combine`` 'min' or 'max' over a
    ``TokenBank.resident(bank)`` (fp16 / bf16), shared weights, no ``top_t``, no ``select``, P a divisor of 64, at least
    ``TOKEN_MSE_PREFILTER_MIN_Q`` queries (a bank of fewer than ``TOKEN_MSE_PREFILTER_MIN_ELEMENTS`` elements:
    ``TOKEN_MSE_PREFILTER_MIN_Q_SMALL``), a shape the library takes (D % 32 == 0, 128 <= D <= 4096, 2048 <= N P < 2^31, k <= 256,
    k <= N) and SKYEMB_TOPK_PREFILTER not 0 is searched in ONE pass for all queries: D dist = A_q + B_r - 2 (c o t) . x is one dot
    product per token, multiplied on the 16-bit matrix cores with a proven error bound next to a per-query and a per-row constant
    (the row constants: ``TokenBank.stage1_mse``, one launch per bank and weight vector); an image is a candidate when some ('min')
    / every ('max') token of it can still reach the query's threshold, and every candidate is re-scored by the contract's own
    chain after each slice of the bank.  Distances and indices are bit for bit those of the grouped route.  ``stats`` gains
    ``redone`` (queries re-run by the grouped route: a full candidate list, a zero or out-of-range query, a negative or NaN
    weight) and ``combine``.  ``top_t`` and ``select`` take the route BY OPT-IN only; a caller that has not asked gets the grouped
    route, as ever.  ``TokenBank.resident(bank).prepare_mse_top_t()`` opens it for ``top_t``: 'min' under any ``top_t`` and 'max'
    under ``top_t == P`` are the plain search; 'max' under 1 <= top_t < P scores a[top_t-1], which reaches a threshold only when at
    least top_t token distances do, so an image is a candidate when the COUNT of its rows that pass the row test is >= top_t, and
    stage 2 sorts the image's exact token distances with the grouped kernel's own network; the first threshold comes from a sample
    scored under the same ``top_t``, a re-run keeps it, ``stats`` gains ``top_t``.  ``Selection(flags).prepare_mse(bank)`` opens it
    for ``select``: stage 1 reads only the 256-row tiles that hold a selected image, every row of a deselected image fails its test
    whatever it holds (a masked copy of the row constants, built with the live tiles by the first search per bank and weight vector
    and kept in the Selection), the first threshold comes from a sample of selected images, a re-run keeps the selection, ``stats``
    gains ``selected`` and ``tiles`` = (live tiles, all tiles).  The selected images must themselves be a bank the route takes
    (selected x P >= 2048 rows -- hence 8 live whole tiles --, k <= selected): a smaller selection is served whole by the grouped
    route, never refused, and fewer than k selected images leave a (+inf, -1) tail.  Smallest Q on a bank of at least
    ``TOKEN_MSE_PREFILTER_MIN_ELEMENTS`` elements: ``TOKEN_MSE_TOPT_PREFILTER_MIN_Q`` (the top-t fold),
    ``TOKEN_MSE_SELECT_PREFILTER_MIN_Q`` (a selection), ``TOKEN_MSE_SELECT_TOPT_PREFILTER_MIN_Q`` (both); smaller banks:
    ``TOKEN_MSE_PREFILTER_MIN_Q_SMALL``.  Per-query weights ([Q, D], below) take the route BY OPT-IN too:
    ``TokenBank.resident(bank).prepare_mse_per_query()`` builds a second 16-bit image of the bank, rows [x ; x o x] of length 2 D with
    the squares rounded once to the bank's dtype (4 N P D bytes beside the bank's 2 N P D, one pass, independent of the weights and
    kept across ``set_weights``); then D dist = A_q - 2 [c_q o t_q ; -c_q / 2] . [x ; x o x] is still one dot product per token, the row
    constant B_r having moved into it, and stage 2 re-scores candidates under row q of c -- bit for bit the grouped per-query route.
    Its rule: metric 'MSE', 'min' or 'max', no ``top_t`` and no ``select`` (with either the request keeps the grouped route), P a
    divisor of 64, D % 32 == 0 and 128 <= D <= 2048, the shape rule above on (N, P, 2 D, k), at least
    ``TOKEN_MSE_PQ_PREFILTER_MIN_Q`` queries (smaller banks: ``TOKEN_MSE_PREFILTER_MIN_Q_SMALL``); ``stats`` gains
    ``per_query_weights``.  A negative, NaN or above-2^10 weight sends back only the queries whose own row holds it; a query with
    c_q o t_q = 0 is re-run as well.  ``combine`` 'mean' takes the route BY OPT-IN as well:
    ``TokenBank.resident(bank).prepare_mse_mean()`` builds a pooled 16-bit image [N, D] of the bank -- each image's tokens summed in
    fp32 in token order, scaled exactly by 1 / P and by the image's own power of two, rounded once (2 N D + 8 N bytes, one pass,
    independent of the weights and kept across ``set_weights``) --; D mean_p dist = A_q + Bbar_i - 2 (c o t) . m_i is exactly linear
    in the tokens, so stage 1 walks N rows instead of N P (its row constants: ``TokenBank.stage1_mse_mean``, one more pass per bank
    and weight vector) and stage 2 re-scores every candidate image's tokens and folds them in token order -- bit for bit the grouped
    route.  Its rule: metric 'MSE', 'mean', shared weights, no ``top_t`` and no ``select`` (with either the request keeps the grouped
    route), P a divisor of 64, D % 32 == 0, 128 <= D <= 4096, N >= 2048 images, k <= 256, at least
    ``TOKEN_MSE_MEAN_PREFILTER_MIN_Q`` queries (smaller banks: ``TOKEN_MSE_PREFILTER_MIN_Q_SMALL``); the first threshold comes from
    the same sample scored under 'mean', a re-run keeps it.  Out of scope for the two-stage route, served by the grouped route as
    ever: metric 'MAE' (no dot product), ``combine`` 'mean' over a bank never asked or together with ``top_t``, ``select`` or
    per-query weights, per-query weights over a bank never asked or together with ``top_t`` or ``select``, fp32 banks, P not dividing
    64, a bool-tensor ``select``.  (Cosine with per-query weights, ``cosine_topk_tokens``, stays on the grouped route as
    well: its row norm sum w_qd x_d^2 sits under a square root in the denominator, so stage 1's candidate test is no longer one
    linear instruction.)

    ``select``, ``prune``, ``stats``, ``world_size``: as for ``cosine_topk_tokens`` (the floor and the merges work on
    key = -distance).  Every ValueError -- an unknown metric or combine, top_t outside 1 .. min(P, 16), k, a selection of
    another length, a shape the kernels do not take -- is raised before the first launch.

    ``weights`` [Q, D] (per-query weights, one row per query, also over a TokenBank's own; [D] or None: the search above, same
    kernels, same bits): query q takes c_q = fp32(w_q / sum(w_q)), prepared row by row, and the contract is untouched, so row q of
    the result is bit for bit the Q = 1 search with query q and ``weights=w_q``.  c [Q, D] sits in LDS beside the queries, so
    the queries run in groups of the largest g <= 16 with 128 D + 32 g k <= 163840, as for ``cosine_topk_tokens``;
    ``stats['per_query_weights']`` is True and ``stats['group']`` is g."""
    rq = _token_request("distance_topk_tokens", queries, bank, k, combine, metric, weights, top_t, select, world_size)
    if _token_prefilter_refusal(rq) is None:
        driver = _topk_tokens_mse_pq_prefiltered if rq.per_query else _topk_tokens_mse_prefiltered
        return driver(rq, queries, prune, stats, process_group, world_size)
    return _topk_tokens(rq, _DistanceScorer.of(rq), queries, prune, stats, process_group, world_size)


def distance_token_scores(queries: torch.Tensor, bank, metric: str = 'MAE', combine: str = 'mean', weights: torch.Tensor | None = None,
                          top_t: int | None = None, select=None):
    """[Q, N] combined weighted MSE / MAE distance of every image of a [N,P,D] token bank (fp32, fp16 or bf16; or a TokenBank, whose
    weights then replace ``weights``), in groups of at most 16 queries; ``metric``, ``combine``, ``top_t`` and the NaN rule as for
    ``distance_topk_tokens``.  ``select``: every [Q, N] slot is written, a deselected image gets +inf.  ``weights`` [Q, D]:
    per-query weights, as for ``distance_topk_tokens`` (groups of g queries at k = 1)."""
    rq = _token_request("distance_token_scores", queries, bank, None, combine, metric, weights, top_t, select)
    return _score_tokens(rq, _DistanceScorer.of(rq), queries)
