"""What the per-pair (tests/test_prefilter_stage1_gpu.py) and per-candidate (tests/test_prefilter_stage2_gpu.py) GPU tests of the
two-stage many-query search share: guarded device buffers, the preparation call, and one search call through the C ABI whose
workspace is read back through skyemb_topk_prefilter_ws_layout; TokenSearch is the same for the patch-token route
(tests/test_token_prefilter_stage_gpu.py), MseTokenSearch for its weighted-MSE forms (tests/test_token_mse_stage_gpu.py).  No test
lives here."""
import numpy as np
import torch

from tests.prefilter_stage1_reference import EPS

DEV = "cuda"
PAD, FILL, GUARD = 256, 0xA5, 0xEE
FILL32 = np.frombuffer(bytes([FILL] * 4), dtype=np.int32)[0]
TORCH16 = {"fp16": torch.float16, "bf16": torch.bfloat16}


class Guarded:
    """nbytes of device memory pre-filled with FILL between two guard zones; .t(dtype, *shape) views it."""
    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * PAD,), FILL, dtype=torch.uint8, device=DEV)
        self.buf[:PAD] = GUARD
        self.buf[PAD + self.n:] = GUARD
        self.mem = self.buf[PAD:PAD + self.n]

    def ptr(self):
        return self.mem.data_ptr()

    def t(self, dtype, *shape):
        return self.mem.view(dtype).view(*shape)

    def np(self, dtype, *shape):
        return self.mem.cpu().numpy().view(dtype).reshape(*shape)

    def intact(self):
        return bool((self.buf[:PAD] == GUARD).all()) and bool((self.buf[PAD + self.n:] == GUARD).all())

    def untouched(self):
        return self.intact() and bool((self.mem == FILL).all())


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bank_tensor(x, fmt):
    """The device bank of `fmt` holding the float32 values x (each one a number of the format)."""
    t = dev(np.asarray(x, dtype=np.float32))
    return t if fmt == "fp32" else t.to(TORCH16[fmt])


def patterns16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def prepare(ops, fmt, x, xn):
    """Run the preparation kernel of `fmt` into guarded buffers: -> (bank tensor, rowp Guarded, image or tail Guarded or None)."""
    N, D = x.shape
    L = ops.lib()
    rows = L.skyemb_bank16_rowp_rows(N)
    bank = bank_tensor(x, fmt)
    xn_d = dev(xn)
    rowp = Guarded(rows * 16)
    if fmt == "fp32":
        assert L.skyemb_bank16_bytes(N, D) == rows * D * 2
        side = Guarded(rows * D * 2)
        rc = L.skyemb_bank16_prepare(ptr(bank), ptr(xn_d), N, D, side.ptr(), rowp.ptr(), stream())
    else:
        side = Guarded(256 * D * 2) if N % 256 else None
        rc = L.skyemb_resident_rowp(ptr(bank), ops.dtype_code(TORCH16[fmt]), ptr(xn_d), N, D, rowp.ptr(), side.ptr() if side else None, stream())
    torch.cuda.synchronize()
    assert rc == 0, L.skyemb_last_error()
    assert rowp.intact() and (side is None or side.intact())
    return bank, xn_d, rowp, side


def ws_arrays(raw, lay, Q, D):
    """The workspace's arrays (numpy views of the bytes `raw`) at the offsets of skyemb_topk_prefilter_ws_layout."""
    Qp, cap = -(-Q // 256) * 256, lay["cap"]
    shapes = dict(qh=(np.uint16, Qp, D), ql=(np.uint16, Qp, D), qbase=(np.float32, Q, 4), qpar=(np.float32, Qp, 4), tau=(np.float32, Q),
                  bound=(np.float32, Q), cnt=(np.int32, Q), overflow=(np.int32, Q), nsel=(np.int32, Q), sel_i=(np.int32, Q, 256),
                  cand_i=(np.int32, Q, cap), cand_d=(np.float32, Q, cap))
    out = {}
    for f, (dt, *shape) in shapes.items():
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[f] = raw[lay[f]:lay[f] + n].view(dt).reshape(*shape)
    return out


class Search:
    """One call of the two-stage search of `fmt` through the C ABI with guarded outputs and workspace; .ws holds the workspace's
    arrays (numpy) as the call left them.  flags (a boolean per row): the search runs under that selection."""
    def __init__(self, ops, fmt, tw, qn, x, xn, k, thr0=None, flags=None, idx_offset=0):
        L = ops.lib()
        Q, D = tw.shape
        N = x.shape[0]
        self.Q, self.N, self.D, self.k = Q, N, D, k
        bank, xn_d, rowp, side = prepare(ops, fmt, x, xn)
        self.rowp = rowp.np(np.float32, -1, 4)
        lay = ops.topk_prefilter_ws_layout(Q, D, k)
        nbytes = L.skyemb_topk_prefilter_ws_bytes(Q, D, k)
        ws = Guarded(nbytes)
        out_s, out_i, redo = Guarded(Q * k * 4), Guarded(Q * k * 8), Guarded(Q * 4)
        tw_d, qn_d, thr_d = dev(tw), dev(qn), dev(thr0)
        tail = ptr(side.mem) if side is not None and fmt != "fp32" else None
        self.tiles = None
        if flags is not None:
            assert thr0 is None
            bits = np.zeros(-(-N // 32) * 32, dtype=np.uint8)
            bits[:N] = flags
            words = dev(np.packbits(bits, bitorder="little").view(np.uint32).view(np.int32))
            rowp_sel, tiles, n_live, last_live = ops.prefilter_select_prepare(words, N, rowp.t(torch.float32, -1, 4))
            self.tiles = tiles.cpu().numpy()[:n_live]
            self.rowp = rowp_sel.cpu().numpy()
            if fmt == "fp32":
                rc = L.skyemb_cosine_topk_prefiltered_sel(ptr(tw_d), ptr(qn_d), Q, ptr(bank), ptr(xn_d), side.ptr(), ptr(rowp_sel), ptr(tiles), n_live,
                                                          last_live, N, D, k, EPS, idx_offset, ws.ptr(), nbytes, out_s.ptr(), out_i.ptr(), redo.ptr(),
                                                          stream())
            elif fmt == "fp16":
                rc = L.skyemb_cosine_topk_prefiltered_lp_sel(ptr(tw_d), ptr(qn_d), Q, ptr(bank), ptr(xn_d), tail, ptr(rowp_sel), ptr(tiles), n_live,
                                                             last_live, N, D, k, EPS, idx_offset, ws.ptr(), nbytes, out_s.ptr(), out_i.ptr(), redo.ptr(),
                                                             stream())
            else:
                rc = L.skyemb_cosine_topk_prefiltered_resident_sel(ptr(tw_d), ptr(qn_d), Q, ptr(bank), ops.dtype_code(TORCH16[fmt]), ptr(xn_d), tail,
                                                                   ptr(rowp_sel), ptr(tiles), n_live, last_live, N, D, k, EPS, idx_offset, ws.ptr(),
                                                                   nbytes, out_s.ptr(), out_i.ptr(), redo.ptr(), stream())
        elif fmt == "fp32":
            rc = L.skyemb_cosine_topk_prefiltered(ptr(tw_d), ptr(qn_d), Q, ptr(bank), ptr(xn_d), side.ptr(), rowp.ptr(), N, D, k, EPS, idx_offset,
                                                  ptr(thr_d), ws.ptr(), nbytes, out_s.ptr(), out_i.ptr(), redo.ptr(), stream())
        else:
            rc = L.skyemb_cosine_topk_prefiltered_resident(ptr(tw_d), ptr(qn_d), Q, ptr(bank), ops.dtype_code(TORCH16[fmt]), ptr(xn_d), tail,
                                                           rowp.ptr(), N, D, k, EPS, idx_offset, ptr(thr_d), ws.ptr(), nbytes, out_s.ptr(),
                                                           out_i.ptr(), redo.ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0, L.skyemb_last_error()
        self.guards_ok = all(g.intact() for g in (ws, out_s, out_i, redo, rowp) + ((side,) if side is not None else ()))
        self.cap = lay["cap"]
        self.ws = ws_arrays(ws.mem.cpu().numpy(), lay, Q, D)
        self.out_s, self.out_i, self.redo = out_s.np(np.float32, Q, k), out_i.np(np.int64, Q, k), redo.np(np.int32, Q)

    def lists(self):
        """Per query the rows of its list (cnt clipped to cap)."""
        return [self.ws["cand_i"][q, :min(int(self.ws["cnt"][q]), self.cap)] for q in range(self.Q)]

    def dense_dots(self, n):
        """dot^ [Q, N] of lists that hold every row once in their first n slots (NaN where a row is missing)."""
        d = np.full((self.Q, self.N), np.nan, dtype=np.float32)
        np.put_along_axis(d, self.ws["cand_i"][:, :n].astype(np.int64), self.ws["cand_d"][:, :n], axis=1)
        return d


def set_lo(monkeypatch, lo):
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", "1" if lo else "0")


TOK_KMAX = 256


class TokenSearch:
    """One call of the two-stage TOKEN search (skyemb_cosine_topk_tokens_prefiltered, or _sel under `flags`, a boolean per image)
    through the C ABI over the bank xw [N, P, D] (float32 values of `fmt`), with guarded outputs and a guarded workspace pre-filled
    with FILL.  .ws: the workspace's arrays at ops.token_prefilter_ws_layout's offsets as the call left them; .rn the lengths of the
    running lists (the `nsel` field), .list [Q, TOK_KMAX] their 64-bit keys.
    token_rescore_body zeroes cnt after every slice, so the candidates are read from cand_i itself: the workspace was filled with
    FILL32, a negative number no image equals, and every later slice wrote its candidates from slot 0 on.  An entry that is not
    FILL32 is a candidate some slice appended; those whose image lies in the LAST slice's range are that slice's complete set,
    the others are what is left of an earlier slice's."""
    def __init__(self, ops, fmt, tw, qn, xw, xn, k, combine, thr0=None, flags=None, idx_offset=0):
        from tests import token_prefilter_select_reference as tps
        L = ops.lib()
        Q, D = tw.shape
        N, P = xw.shape[:2]
        self.Q, self.N, self.P, self.D, self.k = Q, N, P, D, k
        bank, xn_d, rowp, side = prepare(ops, fmt, xw.reshape(N * P, D), xn)
        lay = ops.token_prefilter_ws_layout(Q, D, k)
        nbytes = L.skyemb_token_prefilter_ws_bytes(Q, D, k)
        assert lay["list"] == L.skyemb_topk_prefilter_ws_bytes(Q, D, k)
        assert nbytes == lay["list"] + -(-Q * TOK_KMAX * 8 // 256) * 256
        ws = Guarded(nbytes)
        out_s, out_i, redo = Guarded(Q * k * 4), Guarded(Q * k * 8), Guarded(Q * 4)
        tw_d, qn_d, thr_d = dev(tw), dev(qn), dev(thr0)
        code, comb, tail = ops.dtype_code(TORCH16[fmt]), ops.COMBINE_CODES[combine], side.ptr() if side is not None else None
        self.tiles = self.cum = None
        if flags is None:
            rc = L.skyemb_cosine_topk_tokens_prefiltered(ptr(tw_d), ptr(qn_d), Q, ptr(bank), code, ptr(xn_d), tail, rowp.ptr(), N, P, D, k, comb,
                                                         EPS, idx_offset, ptr(thr_d), ws.ptr(), nbytes, out_s.ptr(), out_i.ptr(), redo.ptr(),
                                                         stream())
        else:
            bits = np.zeros(-(-N // 32) * 32, dtype=np.uint8)
            bits[:N] = flags
            words = dev(np.packbits(bits, bitorder="little").view(np.uint32).view(np.int32))
            rowp_sel, tiles, n_live, last_live, cum = ops.token_prefilter_select_prepare(words, N, P, rowp.t(torch.float32, -1, 4))
            self.tiles, self.cum, self.last_live = tiles.cpu().numpy()[:n_live], cum, last_live
            self.direct_end = tps.direct_end(cum, n_live, k)            # search.py's rule
            rc = L.skyemb_cosine_topk_tokens_prefiltered_sel(ptr(tw_d), ptr(qn_d), Q, ptr(bank), code, ptr(xn_d), tail, ptr(rowp_sel),
                                                             ptr(tiles), n_live, last_live, self.direct_end, N, P, D, k, comb, EPS, idx_offset,
                                                             ptr(thr_d), ws.ptr(), nbytes, out_s.ptr(), out_i.ptr(), redo.ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0, L.skyemb_last_error()
        self.guards_ok = all(g.intact() for g in (ws, out_s, out_i, redo, rowp) + ((side,) if side is not None else ()))
        self.cap = lay["cap"]
        raw = ws.mem.cpu().numpy()
        self.ws = ws_arrays(raw, lay, Q, D)
        self.rn = self.ws["nsel"]
        self.list = raw[lay["list"]:lay["list"] + Q * TOK_KMAX * 8].view(np.uint64).reshape(Q, TOK_KMAX)
        self.out_s, self.out_i, self.redo = out_s.np(np.float32, Q, k), out_i.np(np.int64, Q, k), redo.np(np.int32, Q)

    def candidates(self, q, images=None):
        """The images left in query q's candidate row (all of them, or those inside the boolean mask `images`), duplicates kept."""
        row = self.ws["cand_i"][q]
        row = row[row != FILL32].astype(np.int64)
        if images is None:
            return row
        inside = (row >= 0) & (row < self.N)
        return row[inside][images[row[inside]]]


def select_words(flags, N):
    """The packed selection words (one bit per image, little-endian) of a boolean mask [N], on the device."""
    bits = np.zeros(-(-N // 32) * 32, dtype=np.uint8)
    bits[:N] = flags
    return dev(np.packbits(bits, bitorder="little").view(np.uint32).view(np.int32))


class MseTokenSearch(TokenSearch):
    """TokenSearch's twin for the weighted-MSE search: one call of skyemb_distance_topk_tokens_prefiltered, or of its _top (top_t),
    _sel (flags, a boolean per image), _top_sel or _pq (c of shape [Q, D]: per-query weights) form, over the bank xw [N, P, D]
    (float32 values of `fmt`), raw queries t [Q, D] and prepared weights c.  combine is the DISTANCE combine; thr0 a floor per query
    in KEY space (key = -distance).  skyemb_token_mse_rowp / skyemb_token_mse_pq_image write into guarded buffers (.rowp, .image:
    16-bit patterns [rows, 2 D]); the workspace is read back at ops.token_prefilter_ws_layout(Q, D or 2 D, k).  .ws, .rn, .list,
    .candidates, .out_s (KEYS), .out_i, .redo, .guards_ok as in TokenSearch, and the FILL32 convention with them."""
    def __init__(self, ops, fmt, c, t, xw, k, combine, top_t=None, flags=None, thr0=None, idx_offset=0):
        from tests import token_prefilter_select_reference as tps
        L = ops.lib()
        fmt = {"f16": "fp16"}.get(fmt, fmt)
        Q, D = t.shape
        N, P = xw.shape[:2]
        R = N * P
        self.pq = np.ndim(c) == 2
        Ds = 2 * D if self.pq else D                                   # the row length stage 1 multiplies
        self.Q, self.N, self.P, self.D, self.Ds, self.k = Q, N, P, D, Ds, k
        assert not self.pq or (top_t is None and flags is None)
        bank = bank_tensor(np.ascontiguousarray(xw.reshape(R, D)), fmt)
        code, comb = ops.dtype_code(TORCH16[fmt]), ops.COMBINE_CODES[combine]
        c_d, t_d, thr_d = dev(np.asarray(c, np.float32)), dev(np.asarray(t, np.float32)), dev(thr0)
        rows = L.skyemb_bank16_rowp_rows(R)
        rowp, side = Guarded(rows * 16), None
        if self.pq:
            side = Guarded(rows * Ds * 2)
            rc = L.skyemb_token_mse_pq_image(ptr(bank), code, R, D, side.ptr(), rowp.ptr(), stream())
        else:
            side = Guarded(256 * D * 2) if R % 256 else None
            rc = L.skyemb_token_mse_rowp(ptr(bank), code, ptr(c_d), R, D, rowp.ptr(), side.ptr() if side else None, stream())
        torch.cuda.synchronize()
        assert rc == 0, L.skyemb_last_error()
        assert rowp.intact() and (side is None or side.intact())
        self.rowp = rowp.np(np.float32, -1, 4)
        self.image = side.np(np.uint16, rows, Ds) if self.pq else None
        lay = ops.token_prefilter_ws_layout(Q, Ds, k)
        nbytes = L.skyemb_token_prefilter_ws_bytes(Q, Ds, k)
        assert lay["list"] == L.skyemb_topk_prefilter_ws_bytes(Q, Ds, k)
        assert nbytes == lay["list"] + -(-Q * TOK_KMAX * 8 // 256) * 256
        ws = Guarded(nbytes)
        out_s, out_i, redo = Guarded(Q * k * 4), Guarded(Q * k * 8), Guarded(Q * 4)
        tail = side.ptr() if side is not None else None
        back = (idx_offset, ptr(thr_d), ws.ptr(), nbytes, out_s.ptr(), out_i.ptr(), redo.ptr(), stream())
        self.tiles = self.cum = None
        if self.pq:
            rc = L.skyemb_distance_topk_tokens_prefiltered_pq(ptr(c_d), ptr(t_d), Q, ptr(bank), code, side.ptr(), rowp.ptr(), N, P, D, k, comb,
                                                              *back)
        elif flags is None and top_t is None:
            rc = L.skyemb_distance_topk_tokens_prefiltered(ptr(c_d), ptr(t_d), Q, ptr(bank), code, rowp.ptr(), tail, N, P, D, k, comb, *back)
        elif flags is None:
            rc = L.skyemb_distance_topk_tokens_prefiltered_top(ptr(c_d), ptr(t_d), Q, ptr(bank), code, rowp.ptr(), tail, N, P, D, k, comb, top_t,
                                                               *back)
        else:
            rowp_sel, tiles, n_live, last_live, cum = ops.token_prefilter_select_prepare(select_words(flags, N), N, P, rowp.t(torch.float32, -1, 4))
            self.tiles, self.cum, self.last_live = tiles.cpu().numpy()[:n_live], cum, last_live
            self.direct_end = tps.direct_end(cum, n_live, k)            # search.py's rule
            self.rowp = rowp_sel.cpu().numpy()
            lead = (ptr(c_d), ptr(t_d), Q, ptr(bank), code, ptr(rowp_sel), tail, ptr(tiles), n_live, last_live, self.direct_end, N, P, D, k, comb)
            if top_t is None:
                rc = L.skyemb_distance_topk_tokens_prefiltered_sel(*lead, *back)
            else:
                rc = L.skyemb_distance_topk_tokens_prefiltered_top_sel(*lead, top_t, *back)
        torch.cuda.synchronize()
        assert rc == 0, L.skyemb_last_error()
        self.guards_ok = all(g.intact() for g in (ws, out_s, out_i, redo, rowp) + ((side,) if side is not None else ()))
        self.cap = lay["cap"]
        raw = ws.mem.cpu().numpy()
        self.ws = ws_arrays(raw, lay, Q, Ds)
        self.rn = self.ws["nsel"]
        self.list = raw[lay["list"]:lay["list"] + Q * TOK_KMAX * 8].view(np.uint64).reshape(Q, TOK_KMAX)
        self.out_s, self.out_i, self.redo = out_s.np(np.float32, Q, k), out_i.np(np.int64, Q, k), redo.np(np.int32, Q)

    def dots(self):
        """P = 1, a single direct slice: dot^ [Q, R] from cand_i / cand_d (NaN where a row is not listed), and per query the number
        of slots written -- anything in a list's row that is not the FILL pattern counts, in either array."""
        assert self.P == 1
        ci, cd = self.ws["cand_i"], self.ws["cand_d"]
        used = ci != FILL32
        d = np.full((self.Q, self.N), np.nan, dtype=np.float32)
        ok = used & (ci >= 0) & (ci < self.N)
        qq = np.nonzero(ok)[0]
        d[qq, ci[ok]] = cd[ok]
        written = used | (cd.view(np.int32) != FILL32)
        return d, written.sum(axis=1)
