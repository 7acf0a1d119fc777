"""Thin torch-tensor front end of the C ABI (pointers + sizes in, nothing allocated inside).

PyTorch is used only for device memory and streams; every op below runs a hand-written gfx950
kernel from libskyemb.so on torch's current stream and raises if the library is missing.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_DGELU, ACT_GELU, ACT_NONE, BF16, COMBINE_MAX, COMBINE_MEAN, COMBINE_MIN, F16, F32, KC, METRIC_MAE, METRIC_MSE, RC,
                   AdamwDesc, GemmArgs, GemmGroupInfo, LnBwdSide, check, lib)

TORCH_DTYPE = {BF16: torch.bfloat16, F32: torch.float32, F16: torch.float16}
LP_DTYPES = (torch.bfloat16, torch.float16)     # the two 16-bit operand formats of the MFMA kernels (SKYEMB_BF16 / SKYEMB_F16)


def dtype_code(t: torch.dtype) -> int:
    if t == torch.bfloat16:
        return BF16
    if t == torch.float32:
        return F32
    if t == torch.float16:
        return F16
    raise TypeError(f"unsupported activation dtype {t}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    if t is None:
        return None
    assert t.is_cuda, "libskyemb ops need device tensors (there is no CPU fallback)"
    return t.data_ptr()


# SKYEMB_PREFETCH=0: no prefetch hints in the launches' arguments (read whenever an argument struct is built -- once per launch of a
# captured step -- so that bench.py can A/B the hint inside one process)
def _prefetch_on():
    import os
    return os.environ.get("SKYEMB_PREFETCH", "1") != "0"


def gemm_args(A, B, *, M, N, K, a_layout=KC, b_layout=KC, lda=None, ldb=None, alpha=1.0, bias=None, table=None,
              tab_row=None, ldt=0, dst_row=None, resid=None, ldr=0, aux=None, ldaux=0, act=ACT_NONE, out_f32=None, ldo32=0,
              out=None, ldo=0, out2=None, ldo2=0, tile=0, colsum_a=None, ws=None, split_k=0, prefetch=None):
    """skyemb_gemm_args for C[M,N] = alpha * A[M,K] B[N,K]^T with fused epilogue (see include/skyemb.h).  prefetch: a tensor a LATER
    launch reads (the next layer's weights): touched by this launch so that it is in the memory-side cache by then (a hint)."""
    g = GemmArgs()
    g.A, g.B = _p(A), _p(B)
    g.lda = lda if lda is not None else (K if a_layout == KC else M)
    g.ldb = ldb if ldb is not None else (K if b_layout == KC else N)
    g.a_layout, g.b_layout = a_layout, b_layout
    g.M, g.N, g.K = M, N, K
    g.dtype = dtype_code(A.dtype)
    assert B.dtype == A.dtype
    g.alpha = alpha
    g.bias, g.table, g.tab_row, g.ldt, g.dst_row = _p(bias), _p(table), _p(tab_row), ldt, _p(dst_row)
    g.resid, g.ldr, g.aux, g.ldaux, g.act = _p(resid), ldr, _p(aux), ldaux, act
    g.out_f32, g.ldo32, g.out, g.ldo, g.out2, g.ldo2 = _p(out_f32), ldo32 or N, _p(out), ldo or N, _p(out2), ldo2 or N
    g.tile = tile
    g.colsum_a = _p(colsum_a)
    g.ws, g.ws_bytes, g.split_k = _p(ws), (ws.numel() * ws.element_size() if ws is not None else 0), split_k
    if prefetch is not None and _prefetch_on():
        g.prefetch, g.prefetch_bytes = _p(prefetch), prefetch.numel() * prefetch.element_size() // 4 * 4
    return g


def gemm(A, B, **kw):
    """C[M,N] = alpha * A[M,K] B[N,K]^T with fused epilogue (see include/skyemb.h)."""
    g = gemm_args(A, B, **kw)
    check(lib().skyemb_gemm(ctypes.byref(g), _stream()), "skyemb_gemm")


class GemmGroup:
    """Several independent GEMMs as ONE launch (skyemb_gemm_group_*): one tile shape (``tile`` = 0 lets the plan choose),
    data-gradient (KC.RC) and weight-gradient (RC.RC) problems may share a launch.  Built once from gemm_args(...)
    structs -- the device blob holds the raw pointers, so the operand buffers must stay allocated -- and replayed with
    launch().  `ok` is False when a problem is outside the grouped subset (launch them singly)."""

    def __init__(self, args, device, tile=0, adamw=None, side=None, ln_bwd=None):
        """adamw: an _lib.AdamwDesc -- the optimiser step fused into the launch's epilogue (weight-gradient groups of a
        single-process run: skyemb_gemm_group_plan_adamw).  side = (own_step, lo, hi, blocks) with adamw: the step of the flat
        slice [lo, hi) rides in the launch as a side job of `blocks` extra workgroups (skyemb_gemm_group_plan_side_adamw);
        own_step: the launch's own tiles are stepped in their epilogue too, else stored as gradients.  ln_bwd = dict(dy, x, gamma,
        mean, rstd, g_in, g_out, g_lp, part, M, D): a LayerNorm backward that does not depend on the launch's tiles (a block's
        norm1) rides in it as a side job instead of a launch of its own (skyemb_gemm_group_attach_ln_bwd); `ln_side` says whether
        the plan took it (else the caller launches ops.layernorm_bwd as before)."""
        n = len(args)
        arr = (GemmArgs * n)(*args)
        nbytes = lib().skyemb_gemm_group_blob_bytes(n)
        host = torch.zeros(nbytes, dtype=torch.uint8)
        self.info = GemmGroupInfo()
        if side is not None:
            own, lo, hi, blocks = side
            rc = lib().skyemb_gemm_group_plan_side_adamw(arr, n, tile, ctypes.byref(adamw), int(bool(own)), int(lo), int(hi), int(blocks),
                                                         host.data_ptr(), nbytes, ctypes.byref(self.info))
        elif adamw is not None:
            rc = lib().skyemb_gemm_group_plan_adamw(arr, n, tile, ctypes.byref(adamw), host.data_ptr(), nbytes, ctypes.byref(self.info))
        else:
            rc = lib().skyemb_gemm_group_plan(arr, n, tile, host.data_ptr(), nbytes, ctypes.byref(self.info))
        self.ok = rc == 0
        if rc > 0:
            check(rc, "skyemb_gemm_group_plan")
        # workgroups that compute TILES (the grid also holds the side jobs' workgroups)
        self.tile_blocks = self.info.total_blocks - (int(side[3]) if side is not None else 0)
        self.ln_side = False
        if self.ok and ln_bwd is not None and ln_bwd["dy"].dtype in LP_DTYPES:
            rec = LnBwdSide()
            for k in ("dy", "x", "gamma", "mean", "rstd", "g_in", "g_out", "g_lp", "part"):
                setattr(rec, k, _p(ln_bwd[k]))
            rec.M, rec.D = ln_bwd["M"], ln_bwd["D"]
            rc2 = lib().skyemb_gemm_group_attach_ln_bwd(host.data_ptr(), nbytes, ctypes.byref(self.info), ctypes.byref(rec))
            if rc2 > 0:
                check(rc2, "skyemb_gemm_group_attach_ln_bwd")
            self.ln_side = rc2 == 0
        self.total_blocks = self.info.total_blocks
        self.blob = host.to(device) if self.ok else None

    def launch(self):
        check(lib().skyemb_gemm_group_launch(self.blob.data_ptr(), ctypes.byref(self.info), _stream()), "skyemb_gemm_group_launch")


GEMM_COUNT_NAMES = ("fallback", "pipe", "tile256", "group", "group256", "splitk")


def gemm_launch_counts(reset=False):
    """{family: launches so far in this process} (include/skyemb.h, SKYEMB_GEMM_COUNT_*): a diagnostic the parity tests read."""
    buf = (ctypes.c_longlong * 8)()
    check(lib().skyemb_gemm_launch_counts(ctypes.cast(buf, ctypes.c_void_p), 8, int(reset)), "skyemb_gemm_launch_counts")
    return dict(zip(GEMM_COUNT_NAMES, list(buf)))


def colsum(X, M, N, out, ldx=None):
    code = dtype_code(X.dtype)
    check(lib().skyemb_colsum(_p(X), code, ldx if ldx is not None else N, M, N, _p(out), _stream()), "skyemb_colsum")


def random_mask_from_noise(noise, keep, ids_restore, mask, ids_keep, dec_dst=None, dec_tab=None, n_extra=1):
    B, L = noise.shape
    check(lib().skyemb_random_mask_from_noise(_p(noise), B, L, keep, _p(ids_restore), _p(mask), _p(ids_keep),
                                              _p(dec_dst), _p(dec_tab), n_extra, _stream()), "skyemb_random_mask_from_noise")


def augment(imgs, out, params, nan_mask, noise, A):
    B, C, S, _ = imgs.shape
    check(lib().skyemb_augment(_p(imgs), _p(out), _p(params), _p(nan_mask), _p(noise), B, C, S, A, _stream()), "skyemb_augment")


def tile_cutouts(tile, big_endian, h0, w0, S, out, lo=None, hi=None):
    """out [n, C, S, S] = windows of the HBM-resident survey tile [C, H, W] (4-byte words; big_endian [C] int32 marks planes
    still in FITS byte order), clipped at lo / hi (NaN kept)."""
    C, H, W = tile.shape
    check(lib().skyemb_tile_cutouts(_p(tile), _p(big_endian), C, H, W, _p(h0), _p(w0), h0.numel(), S,
                                    0.0 if lo is None else float(lo), 0.0 if hi is None else float(hi), int(lo is not None),
                                    int(hi is not None), _p(out), _stream()), "skyemb_tile_cutouts")


def attnpool_q(latent, Wq, bq, q):
    """q [D] = Wq latent + bq: the sample-independent query of the attention pool (timm AttentionPoolLatent)."""
    check(lib().skyemb_attnpool_q(_p(latent), _p(Wq), _p(bq), _p(q), q.numel(), _stream()), "skyemb_attnpool_q")


def attnpool_fwd(q, kv, out, prob, B, N, H, hd):
    check(lib().skyemb_attnpool_fwd(_p(q), _p(kv), dtype_code(kv.dtype), _p(out), _p(prob), B, N, H, hd, _stream()), "skyemb_attnpool_fwd")


def attnpool_bwd(q, kv, dout, prob, dkv, dq_part, B, N, H, hd):
    check(lib().skyemb_attnpool_bwd(_p(q), _p(kv), dtype_code(kv.dtype), _p(dout), _p(prob), _p(dkv), _p(dq_part), B, N, H, hd,
                                    _stream()), "skyemb_attnpool_bwd")


def attnpool_fwd_long(q, kv, out, prob, B, N, H, hd):
    """attnpool_fwd for any N <= 4098 tokens (attnpool_fwd takes N <= 256)."""
    check(lib().skyemb_attnpool_fwd_long(_p(q), _p(kv), dtype_code(kv.dtype), _p(out), _p(prob), B, N, H, hd, _stream()),
          "skyemb_attnpool_fwd_long")


def attnpool_bwd_long(q, kv, dout, prob, dkv, dq_part, B, N, H, hd):
    check(lib().skyemb_attnpool_bwd_long(_p(q), _p(kv), dtype_code(kv.dtype), _p(dout), _p(prob), _p(dkv), _p(dq_part), B, N, H, hd,
                                         _stream()), "skyemb_attnpool_bwd_long")


def attnpool_q_bwd(dq_part, latent, Wq, dWq, dbq, dlatent, ws):
    B, D = dq_part.shape
    check(lib().skyemb_attnpool_q_bwd(_p(dq_part), B, _p(latent), _p(Wq), _p(dWq), _p(dbq), _p(dlatent), _p(ws), D, _stream()),
          "skyemb_attnpool_q_bwd")


def simmim_mask_from_noise(noise, ratio_u, max_ratio, grid, p, out_mask):
    """Per-channel random patch masks for SimMIM (utils/dataloaders.py:197-219) from uniform draws: noise [B,C,L], ratio_u [B]."""
    B, C, L = noise.shape
    check(lib().skyemb_simmim_mask_from_noise(_p(noise), _p(ratio_u), max_ratio, B, C, L, grid, p, _p(out_mask), _stream()),
          "skyemb_simmim_mask_from_noise")


def patch_gather(imgs, pmv, ids_keep, out, p, keep, pixel_mean, pixel_std):
    B, C, H, W = imgs.shape
    check(lib().skyemb_patch_gather(_p(imgs), _p(pmv), _p(ids_keep), _p(out), dtype_code(out.dtype), B, C, H, W, p,
                                    keep, pixel_mean, pixel_std, _stream()), "skyemb_patch_gather")


def patch_gather_bwd_pmv(imgs, ids_keep, drows, partial, dpmv, p, keep):
    B, C, H, W = imgs.shape
    check(lib().skyemb_patch_gather_bwd_pmv(_p(imgs), _p(ids_keep), _p(drows), _p(partial), _p(dpmv), B, C, H, W, p,
                                            keep, _stream()), "skyemb_patch_gather_bwd_pmv")


def patch_gather_blend(imgs, pmv, ids_keep, pixel_mask, out, p, keep, pixel_mean, pixel_std):
    """SimMIM input path: NaN fill, then x * (1 - mask) + pmv * mask (pixel_mask None == patch_gather)."""
    B, C, H, W = imgs.shape
    check(lib().skyemb_patch_gather_blend(_p(imgs), _p(pmv), _p(ids_keep), _p(pixel_mask), _p(out), dtype_code(out.dtype), B, C,
                                          H, W, p, keep, pixel_mean, pixel_std, _stream()), "skyemb_patch_gather_blend")


def patch_gather_bwd_pmv_blend(imgs, ids_keep, pixel_mask, drows, partial, dpmv, p, keep):
    B, C, H, W = imgs.shape
    check(lib().skyemb_patch_gather_bwd_pmv_blend(_p(imgs), _p(ids_keep), _p(pixel_mask), _p(drows), _p(partial), _p(dpmv), B,
                                                  C, H, W, p, keep, _stream()), "skyemb_patch_gather_bwd_pmv_blend")


def radec_token_fwd(ra_dec, W0, b0, W1, b1, pos_row, x_rows, row_stride, B, D, sh, z):
    """x_rows: fp32 view starting at the first RA/Dec token row; consecutive samples are row_stride floats apart."""
    check(lib().skyemb_radec_token_fwd(_p(ra_dec), _p(W0), _p(b0), _p(W1), _p(b1), _p(pos_row), _p(x_rows), row_stride, B, D,
                                       _p(sh), _p(z), _stream()), "skyemb_radec_token_fwd")


def radec_token_bwd(g_rows, row_stride, W1, sh, z, dz_ws, dW0, db0, dW1, db1, B, D):
    check(lib().skyemb_radec_token_bwd(_p(g_rows), row_stride, _p(W1), _p(sh), _p(z), _p(dz_ws), _p(dW0), _p(db0), _p(dW1),
                                       _p(db1), B, D, _stream()), "skyemb_radec_token_bwd")


def simmim_pixel_loss(imgs, pred_tok, pixel_mask, loss, dpred_tok, dtype, pred_img, ws, p, extra, pixel_mean, pixel_std,
                      norm_pix, loss_l1, pooled=False, dscale=1.0):
    B, C, H, W = imgs.shape
    check(lib().skyemb_simmim_pixel_loss(_p(imgs), _p(pred_tok), _p(pixel_mask), _p(loss), _p(dpred_tok), dtype, _p(pred_img),
                                         _p(ws), B, C, H, W, p, extra, pixel_mean, pixel_std, int(norm_pix), int(loss_l1),
                                         int(pooled), float(dscale), _stream()), "skyemb_simmim_pixel_loss")


def layernorm_fwd(x, gamma, beta, y, mean, rstd, M, D, eps, y32=None, dtype=None):
    code = dtype if dtype is not None else dtype_code(y.dtype)
    check(lib().skyemb_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(y32), code, _p(mean), _p(rstd), M, D, eps,
                                     _stream()), "skyemb_layernorm_fwd")


def layernorm_bwd_blocks(M):
    return lib().skyemb_layernorm_bwd_blocks(M)


def layernorm_bwd(dy, x, gamma, mean, rstd, g_in, g_out, g_lp, part, dgamma, dbeta, M, D, dtype):
    dy_f32 = 1 if (dy.dtype == torch.float32 and dtype in (BF16, F16)) else 0
    check(lib().skyemb_layernorm_bwd(_p(dy), dy_f32, dtype, _p(x), _p(gamma), _p(mean), _p(rstd), _p(g_in), _p(g_out),
                                     _p(g_lp), _p(part), _p(dgamma), _p(dbeta), M, D, _stream()), "skyemb_layernorm_bwd")


def ln_reduce_items(entries, device):
    """Device tables of a batched column reduce from [(part, dgamma, dbeta, nblk, D), ...]; dbeta None = a single vector
    (part [nblk, D] -> dgamma: the bias-gradient partial sums of a grouped weight-gradient launch).
    -> (items: skyemb_ln_reduce_item x n (32 bytes each), blocks: int32 pairs {item, x | y << 16} per workgroup,
        first_block: [n + 1] host prefix of the items' workgroups)."""
    rows = [[part.data_ptr(), dg.data_ptr(), db.data_ptr() if db is not None else 0, nblk + (D << 32)] for part, dg, db, nblk, D in entries]
    blocks, first = [], [0]
    for k, (part, dg, db, nblk, D) in enumerate(entries):
        for y in range(2 if db is not None else 1):
            blocks += [[k, x | (y << 16)] for x in range((D + 31) // 32)]
        first.append(len(blocks))
    return (torch.tensor(rows, dtype=torch.int64).to(device), torch.tensor(blocks, dtype=torch.int32).to(device), first)


def layernorm_bwd_reduce_batch(table, first, count):
    """Items [first, first + count) of a table made by ln_reduce_items, one launch."""
    items, blocks, first_block = table
    b0, b1 = first_block[first], first_block[first + count]
    check(lib().skyemb_layernorm_bwd_reduce_batch(items.data_ptr(), blocks.data_ptr() + 8 * b0, b1 - b0, _stream()),
          "skyemb_layernorm_bwd_reduce_batch")


def mha_fwd(qkv, out, B, N, H, hd):
    check(lib().skyemb_mha_fwd(_p(qkv), _p(out), dtype_code(qkv.dtype), B, N, H, hd, _stream()), "skyemb_mha_fwd")


def mha_bwd(qkv, dout, dqkv, B, N, H, hd):
    check(lib().skyemb_mha_bwd(_p(qkv), _p(dout), _p(dqkv), dtype_code(qkv.dtype), B, N, H, hd, _stream()),
          "skyemb_mha_bwd")


def mha_plan(bwd, dtype, B, N, H, hd, switches=-1):
    """The launch mha_fwd (bwd=False) / mha_bwd makes for this shape, as a `_lib.MhaPlan`; touches no device.  `switches`: -1 = the
    process's environment, else `_lib.MHA_SW_*` bits.  Raises SkyembError where the entry points would refuse."""
    from ._lib import MhaPlan
    p = MhaPlan()
    check(lib().skyemb_mha_plan(int(bool(bwd)), dtype_code(dtype), B, N, H, hd, switches, p), "skyemb_mha_plan")
    return p


def fill_mask_tokens(x, mask, mask_token, dec_pos, B, L, Dd, n_extra=1):
    check(lib().skyemb_fill_mask_tokens(_p(x), _p(mask), _p(mask_token), _p(dec_pos), B, L, Dd, n_extra, _stream()),
          "skyemb_fill_mask_tokens")


def gather_rows(src, idx, out, out_lp, n_rows, D):
    code = dtype_code(out_lp.dtype) if out_lp is not None else F32
    check(lib().skyemb_gather_rows(_p(src), _p(idx), _p(out), _p(out_lp), code, n_rows, D, _stream()),
          "skyemb_gather_rows")


def rowsum_select(src, ld, sel, row0, inner, outer_stride, n_rows, D, partial, out):
    check(lib().skyemb_rowsum_select(_p(src), ld, _p(sel), row0, inner, outer_stride, n_rows, D, _p(partial), _p(out),
                                     _stream()), "skyemb_rowsum_select")


def masked_patch_loss(imgs, pred, mask, loss, dpred, dpred32, dtype, ws, p, extra, pixel_mean, pixel_std, norm_pix,
                      loss_l1, dscale=1.0):
    B, C, H, W = imgs.shape
    check(lib().skyemb_masked_patch_loss(_p(imgs), _p(pred), _p(mask), _p(loss), _p(dpred), _p(dpred32), dtype, _p(ws),
                                         B, C, H, W, p, extra, pixel_mean, pixel_std, int(norm_pix), int(loss_l1),
                                         float(dscale), _stream()), "skyemb_masked_patch_loss")


def adamw(p, g, m, v, p_lp, n, n_decay, hyper, beta1, beta2, eps, wd, grad_scale=1.0, zero_grad=False, lr=0.0, bc1=1.0,
          bc2=1.0):
    """hyper: device fp32[4] {lr, 1-b1^t, 1-b2^t} (graph-safe) or None to pass lr/bc1/bc2 by value."""
    code = dtype_code(p_lp.dtype) if p_lp is not None else F32
    check(lib().skyemb_adamw(_p(p), _p(g), _p(m), _p(v), _p(p_lp), code, n, n_decay, _p(hyper), lr, bc1, bc2, beta1,
                             beta2, eps, wd, grad_scale, int(zero_grad), dtype_code(g.dtype), _stream()), "skyemb_adamw")


def grad_probe(g, n, state):
    """Accumulates into `state` (device int32[2], zeroed by the caller once per step) whether any of the n gradients at g is
    +-inf / NaN (state[0] != 0) and the largest finite |g| (state[1]: its fp32 bits); see include/skyemb.h."""
    assert state.dtype == torch.int32 and state.numel() >= 2
    check(lib().skyemb_grad_probe(_p(g), dtype_code(g.dtype), n, _p(state), _stream()), "skyemb_grad_probe")


def adamw_guarded(p, g, m, v, p_lp, n, n_decay, hyper, beta1, beta2, eps, wd, skip, grad_scale=1.0, zero_grad=False, lr=0.0,
                  bc1=1.0, bc2=1.0):
    """adamw() that writes nothing when skip[0] != 0 (skip: the state of grad_probe, earlier on the same stream)."""
    assert skip.dtype == torch.int32
    code = dtype_code(p_lp.dtype) if p_lp is not None else F32
    check(lib().skyemb_adamw_guarded(_p(p), _p(g), _p(m), _p(v), _p(p_lp), code, n, n_decay, _p(hyper), lr, bc1, bc2, beta1,
                                     beta2, eps, wd, grad_scale, int(zero_grad), dtype_code(g.dtype), _p(skip), _stream()),
          "skyemb_adamw_guarded")


# skyemb_adamw_work: one work item of a segmented AdamW launch, 16 bytes
ADAMW_WORK_DTYPE = np.dtype([("offset", "<i8"), ("n", "<i4"), ("group", "<i4")])


def adamw_segments_limits():
    """(max_groups, chunk_elems, max_grid) of skyemb_adamw_segments: the most groups of one launch, the most elements of one work
    item, the most workgroups of a launch."""
    out = (ctypes.c_int32 * 3)()
    base = ctypes.addressof(out)
    check(lib().skyemb_adamw_segments_limits(base, base + 4, base + 8), "skyemb_adamw_segments_limits")
    return int(out[0]), int(out[1]), int(out[2])


def adamw_segments_plan(segments, n_groups, buffer_n):
    """segments: [(offset, n, group)] in elements of a flat buffer of buffer_n elements, in any order -> (table, n_work): the host
    table of skyemb_adamw_segments (numpy, ADAMW_WORK_DTYPE; see include/skyemb.h for how it is built).  No device is touched.
    ValueError with the library's text when the segments are refused."""
    segs = (_lib.AdamwSegment * max(len(segments), 1))()
    for s, (offset, n, group) in zip(segs, segments):
        s.offset, s.n, s.group = int(offset), int(n), int(group)
    need, n_work = ctypes.c_int64(0), ctypes.c_int32(0)
    L = lib()

    def call(table, nbytes):
        if L.skyemb_adamw_segments_plan(ctypes.addressof(segs), len(segments), int(n_groups), int(buffer_n), table, nbytes,
                                        ctypes.addressof(need), ctypes.addressof(n_work)) != 0:
            raise ValueError(L.skyemb_last_error().decode())
    call(None, 0)
    table = np.zeros(n_work.value, dtype=ADAMW_WORK_DTYPE)
    call(table.ctypes.data, table.nbytes)
    return table, int(n_work.value)


def adamw_groups(groups):
    """[(lr, bc1, bc2, beta1, beta2, eps, wd, decayed)] -> the skyemb_adamw_group array a launch takes (host memory)."""
    arr = (_lib.AdamwGroup * len(groups))()
    for a, (lr, bc1, bc2, beta1, beta2, eps, wd, decayed) in zip(arr, groups):
        a.lr, a.bc1, a.bc2, a.beta1, a.beta2, a.eps, a.wd, a.decayed = lr, bc1, bc2, beta1, beta2, eps, wd, int(bool(decayed))
    return arr


def adamw_segments(p, g, m, v, p_lp, table, n_work, groups, grad_scale=1.0, skip=None):
    """One AdamW launch over the segments planned into `table` (device copy of adamw_segments_plan's, int32 view) of the flat
    buffers p, g, m, v (fp32) and the shadow p_lp; groups: adamw_groups(...) or the tuples it takes; skip: None or the state of
    grad_probe (the launch writes nothing when skip[0] != 0)."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float32 and p.numel() == g.numel() == m.numel() == v.numel() == p_lp.numel()
    assert table.is_cuda and table.numel() * table.element_size() >= 16 * n_work
    assert skip is None or skip.dtype == torch.int32
    if not isinstance(groups, ctypes.Array):
        groups = adamw_groups(groups)
    check(lib().skyemb_adamw_segments(_p(p), _p(g), _p(m), _p(v), _p(p_lp), dtype_code(p_lp.dtype), _p(table), int(n_work),
                                      ctypes.addressof(groups), len(groups), grad_scale, _p(skip), _stream()), "skyemb_adamw_segments")


def set_scalars(dst, a, b=0.0, c=0.0, d=0.0):
    check(lib().skyemb_set_scalars(_p(dst), a, b, c, d, _stream()), "skyemb_set_scalars")


def cast(src, dst, n):
    check(lib().skyemb_cast(_p(src), _p(dst), dtype_code(dst.dtype), n, _stream()), "skyemb_cast")


def standardise(x, mu, sigma, out):
    N, D = x.shape
    check(lib().skyemb_standardise(_p(x), _p(mu), _p(sigma), _p(out), N, D, _stream()), "skyemb_standardise")


def weighted_norms(x, w, norms, xw_out=None):
    N, D = x.shape
    check(lib().skyemb_weighted_norms(_p(x), _p(w), _p(norms), _p(xw_out), N, D, _stream()), "skyemb_weighted_norms")


BANK_DTYPES = (torch.float32, torch.float16, torch.bfloat16)     # element types of a resident token bank


def bank_dtype_code(t: torch.dtype, who: str) -> int:
    """SKYEMB_* code of a token bank's element type; anything but fp32 / fp16 / bf16 is a ValueError naming the three."""
    if t not in BANK_DTYPES:
        raise ValueError(f"{who}: bank dtype {t} is not supported, expected one of torch.float32, torch.float16, torch.bfloat16")
    return dtype_code(t)


def weighted_norms_lp(x, w, norms):
    """weighted_norms of fp16 / bf16 rows: fp32 on the exactly widened values, bit-equal to weighted_norms(x.float(), ...)."""
    N, D = x.shape
    check(lib().skyemb_weighted_norms_lp(_p(x), bank_dtype_code(x.dtype, "weighted_norms_lp"), _p(w), _p(norms), N, D, _stream()),
          "skyemb_weighted_norms_lp")


def standardise_lp(x, mu, sigma, out):
    """standardise, then one rounding to nearest-even into ``out`` (fp16 or bf16)."""
    N, D = x.shape
    check(lib().skyemb_standardise_lp(_p(x), _p(mu), _p(sigma), _p(out), bank_dtype_code(out.dtype, "standardise_lp"), N, D, _stream()),
          "skyemb_standardise_lp")


def cosine_topk_chunks(N, Q, D, k):
    return lib().skyemb_cosine_topk_chunks(N, Q, D, k)


def cosine_topk(tw, qn, bank, xn, k, eps, idx_offset, nchunks, part_s, part_i, thr0=None):
    Q, D = tw.shape
    N = bank.shape[0]
    check(lib().skyemb_cosine_topk(_p(tw), _p(qn), _p(bank), _p(xn), Q, N, D, k, eps, idx_offset, nchunks, _p(thr0),
                                   _p(part_s), _p(part_i), _stream()), "skyemb_cosine_topk")


def kth_largest_floor(x, k, out):
    Q, S = x.shape
    check(lib().skyemb_kth_largest_floor(_p(x), Q, S, k, _p(out), _stream()), "skyemb_kth_largest_floor")


def sample_floor_applicable(Q, S, D, k, *tensors):
    """The library's own predicate (shape limits AND the SKYEMB_TOPK_STREAM switch) plus the 16-byte alignment the streaming
    scorer needs of the tensors it reads rows from."""
    return bool(lib().skyemb_cosine_sample_floor_applicable(Q, S, D, k)) and all(t.data_ptr() % 16 == 0 for t in tensors)


def cosine_sample_floor(tw, qn, sample, sample_norms, k, eps, ws, out):
    """Pruning floor of a small-Q search from a row sample (tile maxima + one-wave selection): see include/skyemb.h."""
    Q, D = tw.shape
    S = sample.shape[0]
    check(lib().skyemb_cosine_sample_floor(_p(tw), _p(qn), _p(sample), _p(sample_norms), Q, S, D, k, eps, _p(ws), _p(out), _stream()),
          "skyemb_cosine_sample_floor")


def topk_prefilter_applicable(Q, N, D, k):
    return bool(lib().skyemb_topk_prefilter_applicable(Q, N, D, k))


WS_FIELDS = ("qh", "ql", "qbase", "qpar", "tau", "bound", "cnt", "overflow", "nsel", "sel_i", "cand_i", "cand_d", "wg_list", "wg_count")


def topk_prefilter_ws_layout(Q, D, k):
    """Test and diagnostic hook (host arithmetic only): {field: byte offset} of the two-stage search's workspace in the library's
    own order, plus 'cap' and 'capw' (include/skyemb.h, skyemb_topk_prefilter_ws_layout)."""
    out = (ctypes.c_int64 * (len(WS_FIELDS) + 2))()
    check(lib().skyemb_topk_prefilter_ws_layout(Q, D, k, ctypes.addressof(out), len(out)), "skyemb_topk_prefilter_ws_layout")
    return dict(zip(WS_FIELDS + ("cap", "capw"), (int(v) for v in out)))


def bank16_prepare(bank, xn):
    """fp16 image of the bank for the prefiltered many-query top-k: (bank16 [rows, D] half, rowp [rows, 4] float), both
    padded to whole tiles of rows (``skyemb_bank16_rowp_rows``; ``skyemb_bank16_bytes`` is the image's size)."""
    N, D = bank.shape
    rows = lib().skyemb_bank16_rowp_rows(N)
    assert lib().skyemb_bank16_bytes(N, D) == rows * D * 2
    bank16 = torch.empty(rows, D, device=bank.device, dtype=torch.float16)
    rowp = torch.empty(rows, 4, device=bank.device, dtype=torch.float32)
    check(lib().skyemb_bank16_prepare(_p(bank), _p(xn), N, D, _p(bank16), _p(rowp), _stream()), "skyemb_bank16_prepare")
    return bank16, rowp


def _workspace(ws, need, device):
    """``ws`` when it holds ``need`` bytes, else a fresh workspace: what every two-stage wrapper returns for the next call."""
    return ws if ws is not None and ws.numel() >= need else torch.empty(need, device=device, dtype=torch.uint8)


def _check_aligned16(bank, who, what, verb="must start"):
    """ValueError, in the words of ``who``, unless the 16-bit ``bank`` (named ``what`` in the text) starts 16-byte aligned."""
    if bank.data_ptr() % 16:
        raise ValueError(f"{who}: {what} bank {verb} 16-byte aligned (the search reads it by 16-byte LDS-DMA); this tensor starts at "
                         "an odd offset of its storage -- clone() it")


def cosine_topk_prefiltered(tw, qn, bank, xn, bank16, rowp, k, eps, idx_offset, out_s, out_i, redo, thr0=None, ws=None):
    Q, D = tw.shape
    N = bank.shape[0]
    ws = _workspace(ws, lib().skyemb_topk_prefilter_ws_bytes(Q, D, k), tw.device)
    check(lib().skyemb_cosine_topk_prefiltered(_p(tw), _p(qn), Q, _p(bank), _p(xn), _p(bank16), _p(rowp), N, D, k, eps, idx_offset,
                                               _p(thr0), _p(ws), ws.numel(), _p(out_s), _p(out_i), _p(redo), _stream()),
          "skyemb_cosine_topk_prefiltered")
    return ws


def topk_prefilter_eps_a(D, lo=False, resident=False):
    """The proven relative error bound of the prefilter's fp16 dot products (host arithmetic only; see include/skyemb.h)."""
    return lib().skyemb_topk_prefilter_eps_a(D, int(lo), int(resident))


def bank16_rowp_lp(bank16, xn):
    """Per-row constants of a RESIDENT fp16 bank [N, D] for the prefiltered many-query top-k: (tail, rowp).  No image of the bank
    is written: ``rowp`` [rows, 4] float (``skyemb_bank16_rowp_rows``) and ``tail``, one zero-padded tile [256, D] holding the last
    N % 256 rows (None when there are none), are all the memory it takes.  ValueError when the bank is not 16-byte aligned."""
    N, D = bank16.shape
    assert bank16.dtype == torch.float16 and bank16.is_contiguous()
    _check_aligned16(bank16, "bank16_rowp_lp", "the fp16", "must be")
    rows = lib().skyemb_bank16_rowp_rows(N)
    rowp = torch.empty(rows, 4, device=bank16.device, dtype=torch.float32)
    tail = torch.empty(rows - N // 256 * 256, D, device=bank16.device, dtype=torch.float16) if rows != N else None
    check(lib().skyemb_bank16_rowp_lp(_p(bank16), _p(xn), N, D, _p(rowp), _p(tail), _stream()), "skyemb_bank16_rowp_lp")
    return tail, rowp


def cosine_topk_prefiltered_lp(tw, qn, bank16, xn, tail, rowp, k, eps, idx_offset, out_s, out_i, redo, thr0=None, ws=None):
    """``cosine_topk_prefiltered`` over a resident fp16 bank and the (tail, rowp) of ``bank16_rowp_lp``."""
    Q, D = tw.shape
    N = bank16.shape[0]
    ws = _workspace(ws, lib().skyemb_topk_prefilter_ws_bytes(Q, D, k), tw.device)
    check(lib().skyemb_cosine_topk_prefiltered_lp(_p(tw), _p(qn), Q, _p(bank16), _p(xn), _p(tail), _p(rowp), N, D, k, eps, idx_offset,
                                                  _p(thr0), _p(ws), ws.numel(), _p(out_s), _p(out_i), _p(redo), _stream()),
          "skyemb_cosine_topk_prefiltered_lp")
    return ws


def resident_dtype_code(t: torch.dtype, who: str) -> int:
    """SKYEMB_* code of a resident 16-bit bank's element type; anything but fp16 / bf16 is a ValueError naming the two."""
    if t not in LP_DTYPES:
        raise ValueError(f"{who}: bank dtype {t} is not supported, expected torch.float16 or torch.bfloat16")
    return dtype_code(t)


def topk_prefilter_eps_a_resident(D, dtype, lo=False):
    """``topk_prefilter_eps_a`` over a resident bank of ``dtype`` (torch.float16: the resident value; torch.bfloat16: the bf16
    search's bound, host arithmetic only; see include/skyemb.h)."""
    return lib().skyemb_topk_prefilter_eps_a_resident(D, int(lo), resident_dtype_code(dtype, "topk_prefilter_eps_a_resident"))


def resident_rowp(bank16, xn):
    """``bank16_rowp_lp`` for a resident bank of either 16-bit format, fp16 or bf16 (ValueError for any other): (tail, rowp), the
    tail tile in the bank's dtype.  ValueError when the bank is not 16-byte aligned."""
    N, D = bank16.shape
    code = resident_dtype_code(bank16.dtype, "resident_rowp")
    assert bank16.is_contiguous()
    _check_aligned16(bank16, "resident_rowp", "the 16-bit", "must be")
    rows = lib().skyemb_bank16_rowp_rows(N)
    rowp = torch.empty(rows, 4, device=bank16.device, dtype=torch.float32)
    tail = torch.empty(rows - N // 256 * 256, D, device=bank16.device, dtype=bank16.dtype) if rows != N else None
    check(lib().skyemb_resident_rowp(_p(bank16), code, _p(xn), N, D, _p(rowp), _p(tail), _stream()), "skyemb_resident_rowp")
    return tail, rowp


def cosine_topk_prefiltered_resident(tw, qn, bank16, xn, tail, rowp, k, eps, idx_offset, out_s, out_i, redo, thr0=None, ws=None):
    """``cosine_topk_prefiltered_lp`` over a resident bank of either 16-bit format and the (tail, rowp) of ``resident_rowp``."""
    Q, D = tw.shape
    N = bank16.shape[0]
    code = resident_dtype_code(bank16.dtype, "cosine_topk_prefiltered_resident")
    ws = _workspace(ws, lib().skyemb_topk_prefilter_ws_bytes(Q, D, k), tw.device)
    check(lib().skyemb_cosine_topk_prefiltered_resident(_p(tw), _p(qn), Q, _p(bank16), code, _p(xn), _p(tail), _p(rowp), N, D, k, eps,
                                                        idx_offset, _p(thr0), _p(ws), ws.numel(), _p(out_s), _p(out_i), _p(redo),
                                                        _stream()), "skyemb_cosine_topk_prefiltered_resident")
    return ws


def token_prefilter_refusal(Q, N, P, D, k):
    """None when the two-stage token search takes the shape, else the library's own statement of its limits."""
    L = lib()
    return None if L.skyemb_token_prefilter_applicable(Q, N, P, D, k) else L.skyemb_last_error().decode()


def token_prefilter_ws_layout(Q, D, k):
    """``topk_prefilter_ws_layout`` for the token search (host arithmetic only): the same fields -- the running lists' lengths live
    in 'nsel' -- plus 'list', the byte offset of the running lists u64 [Q, 256], which follow the row search's workspace
    (include/skyemb.h, skyemb_token_prefilter_ws_bytes)."""
    out = topk_prefilter_ws_layout(Q, D, k)
    out["list"] = lib().skyemb_topk_prefilter_ws_bytes(Q, D, k)
    return out


def cosine_topk_tokens_prefiltered(tw, qn, tokens, xn, tail, rowp, k, combine, eps, idx_offset, out_s, out_i, redo, thr0=None, ws=None):
    """The two-stage many-query search over a resident 16-bit token bank ``tokens`` [N, P, D] and the (tail, rowp) of
    ``resident_rowp`` over its flat rows; ``combine``: COMBINE_CODES['min'] or ['max'] (include/skyemb.h)."""
    Q, D = tw.shape
    N, P = tokens.shape[:2]
    code = resident_dtype_code(tokens.dtype, "cosine_topk_tokens_prefiltered")
    ws = _workspace(ws, lib().skyemb_token_prefilter_ws_bytes(Q, D, k), tw.device)
    check(lib().skyemb_cosine_topk_tokens_prefiltered(_p(tw), _p(qn), Q, _p(tokens), code, _p(xn), _p(tail), _p(rowp), N, P, D, k, combine,
                                                      eps, idx_offset, _p(thr0), _p(ws), ws.numel(), _p(out_s), _p(out_i), _p(redo),
                                                      _stream()), "skyemb_cosine_topk_tokens_prefiltered")
    return ws


def token_mse_prefilter_refusal(Q, N, P, D, k):
    """None when the two-stage weighted-MSE token search takes the shape, else the library's own statement of its limits.  Host
    arithmetic only."""
    L = lib()
    return None if L.skyemb_token_mse_prefilter_applicable(Q, N, P, D, k) else L.skyemb_last_error().decode()


def token_mse_prefilter_eps(D, dtype, lo=False):
    """eps_mse of the two-stage weighted-MSE search over a ``dtype`` bank (host arithmetic only; include/skyemb.h)."""
    return lib().skyemb_token_mse_prefilter_eps(D, int(lo), resident_dtype_code(dtype, "token_mse_prefilter_eps"))


def token_mse_prefilter_gamma(D):
    """gamma, the widening of the distance threshold for the contract's own roundings (host arithmetic only; include/skyemb.h)."""
    return lib().skyemb_token_mse_prefilter_gamma(D)


def token_mse_rowp(tokens, c):
    """(tail, rowp) of the two-stage weighted-MSE search: the row constants of a resident 16-bit token bank ``tokens`` [N, P, D]
    (or its flat rows [R, D]) under the weights ``c`` [D] (``prepare_distance_weights``), and the zero-padded tail tile [256, D]
    of the last R % 256 rows (None when there are none).  One launch per (bank, c)."""
    D = tokens.shape[-1]
    R = tokens.numel() // D
    code = resident_dtype_code(tokens.dtype, "token_mse_rowp")
    assert tokens.is_contiguous() and c.dtype == torch.float32 and c.is_contiguous() and tuple(c.shape) == (D,)
    _check_aligned16(tokens, "token_mse_rowp", "the 16-bit", "must be")
    rows = lib().skyemb_bank16_rowp_rows(R)
    rowp = torch.empty(rows, 4, device=tokens.device, dtype=torch.float32)
    tail = torch.empty(256, D, device=tokens.device, dtype=tokens.dtype) if rows != R else None
    check(lib().skyemb_token_mse_rowp(_p(tokens), code, _p(c), R, D, _p(rowp), _p(tail), _stream()), "skyemb_token_mse_rowp")
    return tail, rowp


def distance_topk_tokens_prefiltered(c, t, tokens, tail, rowp, k, combine, idx_offset, out_s, out_i, redo, thr0=None, ws=None):
    """The two-stage many-query weighted-MSE search over a resident 16-bit token bank ``tokens`` [N, P, D] and the (tail, rowp) of
    ``token_mse_rowp`` under the same ``c``; ``combine``: COMBINE_CODES['min'] or ['max'] of the DISTANCES.  ``out_s`` receives
    keys = -distance (include/skyemb.h)."""
    Q, D = t.shape
    N, P = tokens.shape[:2]
    code = resident_dtype_code(tokens.dtype, "distance_topk_tokens_prefiltered")
    ws = _workspace(ws, lib().skyemb_token_prefilter_ws_bytes(Q, D, k), t.device)
    check(lib().skyemb_distance_topk_tokens_prefiltered(_p(c), _p(t), Q, _p(tokens), code, _p(rowp), _p(tail), N, P, D, k, combine,
                                                        idx_offset, _p(thr0), _p(ws), ws.numel(), _p(out_s), _p(out_i), _p(redo),
                                                        _stream()), "skyemb_distance_topk_tokens_prefiltered")
    return ws


def token_mse_topt_prefilter_refusal(Q, N, P, D, k, combine, top_t):
    """None when the two-stage weighted-MSE token search takes the shape under ``top_t`` (``combine``: a COMBINE_CODES value of the
    DISTANCES), else the library's own reason: the plain search's limits, 1 <= top_t <= min(P, 16), and no mean."""
    L = lib()
    return None if L.skyemb_token_mse_topt_prefilter_applicable(Q, N, P, D, k, combine, top_t) else L.skyemb_last_error().decode()


def token_mse_topt_folds(P, combine, top_t):
    """``token_topt_folds`` for the weighted-MSE search, ``combine`` the DISTANCE combine -- the rule of include/skyemb.h restated in
    key space (key = -distance): distance 'min' is the key-space max whatever ``top_t`` says, distance 'max' the key-space min, so
    'max' with top_t in (0, P) is the plain search and 'max' with 1 <= top_t < P counts rows and sorts keys."""
    assert combine in (COMBINE_CODES['min'], COMBINE_CODES['max'])
    return token_topt_folds(P, COMBINE_CODES['max' if combine == COMBINE_CODES['min'] else 'min'], top_t)


def distance_topk_tokens_prefiltered_top(c, t, tokens, tail, rowp, k, combine, top_t, idx_offset, out_s, out_i, redo, thr0=None, ws=None):
    """``distance_topk_tokens_prefiltered`` under ``top_t`` (0: that call; include/skyemb.h): distance 'max' scores an image by its
    top_t-th smallest token distance, 'min' is the plain min."""
    Q, D = t.shape
    N, P = tokens.shape[:2]
    code = resident_dtype_code(tokens.dtype, "distance_topk_tokens_prefiltered_top")
    ws = _workspace(ws, lib().skyemb_token_prefilter_ws_bytes(Q, D, k), t.device)
    check(lib().skyemb_distance_topk_tokens_prefiltered_top(_p(c), _p(t), Q, _p(tokens), code, _p(rowp), _p(tail), N, P, D, k, combine, top_t,
                                                            idx_offset, _p(thr0), _p(ws), ws.numel(), _p(out_s), _p(out_i), _p(redo),
                                                            _stream()), "skyemb_distance_topk_tokens_prefiltered_top")
    return ws


def distance_topk_tokens_prefiltered_top_sel(c, t, tokens, tail, prepared, direct_end, k, combine, top_t, idx_offset, out_s, out_i, redo,
                                             thr0=None, ws=None):
    """``distance_topk_tokens_prefiltered_top`` under a selection of images: ``prepared`` is ``token_prefilter_select_prepare``'s result
    over the rowp of ``token_mse_rowp``, ``direct_end`` the position of the live-tile list at which the first slice ends (``top_t`` 0:
    the plain search under the selection; include/skyemb.h)."""
    Q, D = t.shape
    N, P = tokens.shape[:2]
    rowp_sel, tiles, n_live, last_live = prepared[:4]
    code = resident_dtype_code(tokens.dtype, "distance_topk_tokens_prefiltered_top_sel")
    ws = _workspace(ws, lib().skyemb_token_prefilter_ws_bytes(Q, D, k), t.device)
    check(lib().skyemb_distance_topk_tokens_prefiltered_top_sel(_p(c), _p(t), Q, _p(tokens), code, _p(rowp_sel), _p(tail), _p(tiles), n_live,
                                                                last_live, direct_end, N, P, D, k, combine, top_t, idx_offset, _p(thr0),
                                                                _p(ws), ws.numel(), _p(out_s), _p(out_i), _p(redo), _stream()),
          "skyemb_distance_topk_tokens_prefiltered_top_sel")
    return ws


def distance_topk_tokens_prefiltered_sel(c, t, tokens, tail, prepared, direct_end, k, combine, idx_offset, out_s, out_i, redo, thr0=None,
                                         ws=None):
    """``distance_topk_tokens_prefiltered`` under a selection of images (include/skyemb.h)."""
    Q, D = t.shape
    N, P = tokens.shape[:2]
    rowp_sel, tiles, n_live, last_live = prepared[:4]
    code = resident_dtype_code(tokens.dtype, "distance_topk_tokens_prefiltered_sel")
    ws = _workspace(ws, lib().skyemb_token_prefilter_ws_bytes(Q, D, k), t.device)
    check(lib().skyemb_distance_topk_tokens_prefiltered_sel(_p(c), _p(t), Q, _p(tokens), code, _p(rowp_sel), _p(tail), _p(tiles), n_live,
                                                            last_live, direct_end, N, P, D, k, combine, idx_offset, _p(thr0), _p(ws),
                                                            ws.numel(), _p(out_s), _p(out_i), _p(redo), _stream()),
          "skyemb_distance_topk_tokens_prefiltered_sel")
    return ws


def token_mse_pq_prefilter_refusal(Q, N, P, D, k):
    """None when the two-stage weighted-MSE token search with per-query weights takes the shape, else the library's own statement
    of its limits.  Host arithmetic only."""
    L = lib()
    return None if L.skyemb_token_mse_pq_prefilter_applicable(Q, N, P, D, k) else L.skyemb_last_error().decode()


def token_mse_pq_prefilter_eps(D, dtype, lo=False):
    """eps_pq of the two-stage weighted-MSE search with per-query weights over a ``dtype`` bank (host arithmetic only;
    include/skyemb.h)."""
    return lib().skyemb_token_mse_pq_prefilter_eps(D, int(lo), resident_dtype_code(dtype, "token_mse_pq_prefilter_eps"))


def token_mse_pq_image(tokens, image=None, rowp=None):
    """(image, rowp) of the two-stage weighted-MSE search with per-query weights: the second 16-bit image [rows, 2 D] of a resident
    token bank ``tokens`` [N, P, D] (or its flat rows [R, D]), rows [x ; r16(x o x)], and its row constants [rows, 4]; rows = R
    padded to whole 256-row tiles (zero rows, sentinel constants).  One launch per bank: neither depends on the weights.  ``image``
    / ``rowp``: buffers to write into (the tests' guard buffers), allocated when None."""
    D = tokens.shape[-1]
    R = tokens.numel() // D
    code = resident_dtype_code(tokens.dtype, "token_mse_pq_image")
    assert tokens.is_contiguous()
    _check_aligned16(tokens, "token_mse_pq_image", "the 16-bit", "must be")
    rows = lib().skyemb_bank16_rowp_rows(R)
    image = torch.empty(rows, 2 * D, device=tokens.device, dtype=tokens.dtype) if image is None else image
    rowp = torch.empty(rows, 4, device=tokens.device, dtype=torch.float32) if rowp is None else rowp
    assert image.is_contiguous() and rowp.is_contiguous() and image.numel() == rows * 2 * D and rowp.numel() == rows * 4
    assert image.dtype == tokens.dtype and rowp.dtype == torch.float32
    check(lib().skyemb_token_mse_pq_image(_p(tokens), code, R, D, _p(image), _p(rowp), _stream()), "skyemb_token_mse_pq_image")
    return image, rowp


def distance_topk_tokens_prefiltered_pq(c, t, tokens, image, rowp, k, combine, idx_offset, out_s, out_i, redo, thr0=None, ws=None):
    """The two-stage many-query weighted-MSE search with per-query weights ``c`` [Q, D] (``prepare_distance_weights`` of [Q, D]
    weights) over a resident 16-bit token bank ``tokens`` [N, P, D] and the (image, rowp) of ``token_mse_pq_image``; ``combine``:
    COMBINE_CODES['min'] or ['max'] of the DISTANCES.  ``out_s`` receives keys = -distance (include/skyemb.h)."""
    Q, D = t.shape
    N, P = tokens.shape[:2]
    assert tuple(c.shape) == (Q, D) and c.dtype == torch.float32 and c.is_contiguous() and t.is_contiguous()
    code = resident_dtype_code(tokens.dtype, "distance_topk_tokens_prefiltered_pq")
    ws = _workspace(ws, lib().skyemb_token_prefilter_ws_bytes(Q, 2 * D, k), t.device)
    check(lib().skyemb_distance_topk_tokens_prefiltered_pq(_p(c), _p(t), Q, _p(tokens), code, _p(image), _p(rowp), N, P, D, k, combine,
                                                           idx_offset, _p(thr0), _p(ws), ws.numel(), _p(out_s), _p(out_i), _p(redo),
                                                           _stream()), "skyemb_distance_topk_tokens_prefiltered_pq")
    return ws


def token_mse_mean_prefilter_refusal(Q, N, P, D, k):
    """None when the two-stage weighted-MSE token search under combine mean takes the shape (N >= 2048 images: stage 1 walks the
    pooled image), else the library's own statement of its limits.  Host arithmetic only."""
    L = lib()
    return None if L.skyemb_token_mse_mean_prefilter_applicable(Q, N, P, D, k) else L.skyemb_last_error().decode()


def token_mse_mean_prefilter_eps(D, dtype, lo=True):
    """eps of stage 1 of the weighted-MSE search under combine mean over a ``dtype`` bank: the pooled image's eps_m + 2^-22 (host
    arithmetic only; include/skyemb.h)."""
    return lib().skyemb_token_mse_mean_prefilter_eps(D, int(lo), resident_dtype_code(dtype, "token_mse_mean_prefilter_eps"))


def token_mse_mean_prefilter_gamma(D, P):
    """gamma of that search: ``token_mse_prefilter_gamma(D)`` widened for the mean's own P - 1 rounded additions (host arithmetic
    only; include/skyemb.h)."""
    return lib().skyemb_token_mse_mean_prefilter_gamma(D, P)


def token_mse_mean_pool(tokens):
    """(pooled, tail, aux) of ``skyemb_token_mse_mean_pool`` over a resident 16-bit token bank ``tokens`` [N, P, D]: the pooled
    image [N, D] in the bank's dtype -- the fp32 sum of each image's tokens in token order, scaled exactly by 1 / P and by the
    image's power of two 2^-e, rounded once --, its zero-padded tail tile (None when N % 256 == 0) and aux f32
    [ceil(N / 256) * 256, 2] = {R1, 2^-e}, the bank's share of the row constants.  One pass over the bank; nothing depends on the
    weights."""
    N, P, D = tokens.shape
    code = resident_dtype_code(tokens.dtype, "token_mse_mean_pool")
    assert tokens.is_contiguous()
    _check_aligned16(tokens, "token_mse_mean_pool", "the 16-bit", "must be")
    rows = lib().skyemb_bank16_rowp_rows(N)
    pooled = torch.empty(N, D, device=tokens.device, dtype=tokens.dtype)
    aux = torch.empty(rows, 2, device=tokens.device, dtype=torch.float32)
    tail = torch.empty(256, D, device=tokens.device, dtype=tokens.dtype) if rows != N else None
    check(lib().skyemb_token_mse_mean_pool(_p(tokens), code, N, P, D, _p(pooled), _p(aux), _p(tail), _stream()),
          "skyemb_token_mse_mean_pool")
    return pooled, tail, aux


def token_mse_mean_rowp(tokens, c, aux):
    """rowp f32 [ceil(N / 256) * 256, 4] of the weighted-MSE search under combine mean: the row constants of the pooled image of
    ``tokens`` [N, P, D] under the weights ``c`` [D] (``prepare_distance_weights``), from ``aux`` of ``token_mse_mean_pool``.  One
    more pass over the bank per (bank, c)."""
    N, P, D = tokens.shape
    code = resident_dtype_code(tokens.dtype, "token_mse_mean_rowp")
    assert tokens.is_contiguous() and c.dtype == torch.float32 and c.is_contiguous() and tuple(c.shape) == (D,)
    rows = lib().skyemb_bank16_rowp_rows(N)
    assert aux.dtype == torch.float32 and aux.is_contiguous() and tuple(aux.shape) == (rows, 2)
    rowp = torch.empty(rows, 4, device=tokens.device, dtype=torch.float32)
    check(lib().skyemb_token_mse_mean_rowp(_p(tokens), code, _p(c), _p(aux), N, P, D, _p(rowp), _stream()), "skyemb_token_mse_mean_rowp")
    return rowp


def distance_topk_tokens_mean_prefiltered(c, t, tokens, pooled, tail, rowp, k, idx_offset, out_s, out_i, redo, thr0=None, ws=None):
    """The two-stage many-query weighted-MSE search under combine mean over a resident 16-bit token bank ``tokens`` [N, P, D], the
    (pooled, tail) of ``token_mse_mean_pool`` and the rowp of ``token_mse_mean_rowp`` under the same ``c``.  ``out_s`` receives
    keys = -distance (include/skyemb.h)."""
    Q, D = t.shape
    N, P = tokens.shape[:2]
    code = resident_dtype_code(tokens.dtype, "distance_topk_tokens_mean_prefiltered")
    ws = _workspace(ws, lib().skyemb_token_mean_prefilter_ws_bytes(Q, D, k), t.device)
    check(lib().skyemb_distance_topk_tokens_mean_prefiltered(_p(c), _p(t), Q, _p(tokens), code, _p(pooled), _p(tail), _p(rowp), N, P, D, k,
                                                             idx_offset, _p(thr0), _p(ws), ws.numel(), _p(out_s), _p(out_i), _p(redo),
                                                             _stream()), "skyemb_distance_topk_tokens_mean_prefiltered")
    return ws


def token_mean_prefilter_refusal(Q, N, P, D, k):
    """None when the two-stage token search with combine mean takes the shape, else the library's own statement of its limits."""
    L = lib()
    return None if L.skyemb_token_mean_prefilter_applicable(Q, N, P, D, k) else L.skyemb_last_error().decode()


def token_mean_prefilter_eps_m(D, dtype, lo=True):
    """eps_m of stage 1 over the pooled image of a ``dtype`` token bank (host arithmetic only; include/skyemb.h)."""
    return lib().skyemb_token_mean_prefilter_eps_m(D, int(lo), resident_dtype_code(dtype, "token_mean_prefilter_eps_m"))


def token_mean_pool(tokens, xn):
    """(pooled, tail, rowp) of ``skyemb_token_mean_pool`` over a resident 16-bit token bank ``tokens`` [N, P, D] and the norms of
    its N * P rows: the pooled image [N, D] in the bank's dtype, its zero-padded tail tile (None when N % 256 == 0) and the row
    constants f32 [ceil(N / 256) * 256, 4] of the mean bound."""
    N, P, D = tokens.shape
    code = resident_dtype_code(tokens.dtype, "token_mean_pool")
    assert tokens.is_contiguous()
    rows = lib().skyemb_bank16_rowp_rows(N)
    pooled = torch.empty(N, D, device=tokens.device, dtype=tokens.dtype)
    rowp = torch.empty(rows, 4, device=tokens.device, dtype=torch.float32)
    tail = torch.empty(256, D, device=tokens.device, dtype=tokens.dtype) if rows != N else None
    check(lib().skyemb_token_mean_pool(_p(tokens), code, _p(xn), N, P, D, _p(pooled), _p(rowp), _p(tail), _stream()),
          "skyemb_token_mean_pool")
    return pooled, tail, rowp


def cosine_topk_tokens_mean_prefiltered(tw, qn, tokens, xn, pooled, tail, rowp, k, eps, idx_offset, out_s, out_i, redo, thr0=None, ws=None):
    """The two-stage many-query search with combine mean over a resident 16-bit token bank ``tokens`` [N, P, D] and the
    (pooled, tail, rowp) of ``token_mean_pool`` (include/skyemb.h)."""
    Q, D = tw.shape
    N, P = tokens.shape[:2]
    code = resident_dtype_code(tokens.dtype, "cosine_topk_tokens_mean_prefiltered")
    ws = _workspace(ws, lib().skyemb_token_mean_prefilter_ws_bytes(Q, D, k), tw.device)
    check(lib().skyemb_cosine_topk_tokens_mean_prefiltered(_p(tw), _p(qn), Q, _p(tokens), code, _p(xn), _p(tail), _p(rowp), N, P, D, k,
                                                           COMBINE_CODES['mean'], eps, idx_offset, _p(thr0), _p(ws), ws.numel(),
                                                           _p(out_s), _p(out_i), _p(redo), _p(pooled), _stream()),
          "skyemb_cosine_topk_tokens_mean_prefiltered")
    return ws


def token_mean_select_prefilter_refusal(Q, S, P, D, k):
    """None when the two-stage token search with combine mean takes a selection of ``S`` images as the bank stage 1 walks (its
    compacted pooled image: the rule of ``token_mean_prefilter_refusal`` with the selected images for the bank's), else the
    library's own statement of those limits."""
    return token_mean_prefilter_refusal(Q, S, P, D, k)


def token_mean_select_gather(pooled, rowp, idx):
    """(pooled_sel, tail_sel, rowp_sel, map) of ``skyemb_token_mean_select_gather``: the rows ``idx`` (i64 [S], ascending) of the
    pooled image [N, D] and of the row constants of ``token_mean_pool``, compacted -- the image [S, D] in the bank's dtype, its
    zero-padded tail tile (None when S % 256 == 0), the constants f32 [ceil(S / 256) * 256, 4] and compacted position -> image
    (i32 [S]).  One short launch; 2 D + 20 bytes per selected image and the tail tile."""
    N, D = pooled.shape
    S = int(idx.numel())
    code = resident_dtype_code(pooled.dtype, "token_mean_select_gather")
    assert pooled.is_contiguous() and idx.dtype == torch.int64 and idx.is_contiguous() and idx.device == pooled.device
    rows = lib().skyemb_bank16_rowp_rows(S)
    pooled_sel = torch.empty(S, D, device=pooled.device, dtype=pooled.dtype)
    rowp_sel = torch.empty(rows, 4, device=pooled.device, dtype=torch.float32)
    tail_sel = torch.empty(256, D, device=pooled.device, dtype=pooled.dtype) if rows != S else None
    cmap = torch.empty(S, device=pooled.device, dtype=torch.int32)
    check(lib().skyemb_token_mean_select_gather(_p(pooled), _p(rowp), _p(idx), N, S, D, code, _p(pooled_sel), _p(rowp_sel), _p(tail_sel),
                                                _p(cmap), _stream()), "skyemb_token_mean_select_gather")
    return pooled_sel, tail_sel, rowp_sel, cmap


def cosine_topk_tokens_mean_prefiltered_sel(tw, qn, tokens, xn, pooled_sel, tail_sel, rowp_sel, cmap, k, eps, idx_offset, out_s, out_i, redo,
                                            thr0=None, ws=None):
    """``cosine_topk_tokens_mean_prefiltered`` under a selection of images: (pooled_sel, tail_sel, rowp_sel, cmap) is
    ``token_mean_select_gather``'s result over the pooled image of ``tokens`` (include/skyemb.h)."""
    Q, D = tw.shape
    N, P = tokens.shape[:2]
    S = pooled_sel.shape[0]
    code = resident_dtype_code(tokens.dtype, "cosine_topk_tokens_mean_prefiltered_sel")
    ws = _workspace(ws, lib().skyemb_token_mean_prefilter_ws_bytes(Q, D, k), tw.device)
    check(lib().skyemb_cosine_topk_tokens_mean_prefiltered_sel(_p(tw), _p(qn), Q, _p(tokens), code, _p(xn), _p(tail_sel), _p(rowp_sel), N, S,
                                                               _p(cmap), P, D, k, COMBINE_CODES['mean'], eps, idx_offset, _p(thr0), _p(ws),
                                                               ws.numel(), _p(out_s), _p(out_i), _p(redo), _p(pooled_sel), _stream()),
          "skyemb_cosine_topk_tokens_mean_prefiltered_sel")
    return ws


def token_prefilter_select_prepare(words, N, P, rowp):
    """What the two-stage token search needs of a selection of IMAGES (packed ``words`` of ``pack_select`` over the N images) over
    a resident token bank of N x P rows with row constants ``rowp`` (``resident_rowp`` over the flat rows): (rowp_sel, tiles, n_live,
    last_live, cum) -- the masked copy of the constants (every row of a deselected image holds the padding sentinel), the ascending
    list of the live 256-row tiles (i32, its first n_live entries), their number, whether the bank's last tile is one of them, and
    as a host list the number of selected images up to and including each live tile.  Two short launches and one read-back."""
    rows = rowp.shape[0]
    rowp_sel = torch.empty_like(rowp)
    tiles = torch.empty(rows // 256, device=rowp.device, dtype=torch.int32)
    cum = torch.empty(rows // 256 + 2, device=rowp.device, dtype=torch.int32)       # the counts, then info: one read-back
    info = cum[rows // 256:]
    check(lib().skyemb_token_prefilter_select_prepare(_p(words), N, P, _p(rowp), _p(rowp_sel), _p(tiles), _p(cum), _p(info), _stream()),
          "skyemb_token_prefilter_select_prepare")
    host = cum.cpu().numpy()
    n_live, last_live = int(host[-2]), int(host[-1])
    return rowp_sel, tiles, n_live, last_live, host[:n_live].tolist()


def cosine_topk_tokens_prefiltered_sel(tw, qn, tokens, xn, tail, prepared, direct_end, k, combine, eps, idx_offset, out_s, out_i, redo,
                                       thr0=None, ws=None):
    """``cosine_topk_tokens_prefiltered`` under a selection of images: ``prepared`` is ``token_prefilter_select_prepare``'s result,
    ``direct_end`` the position of the live-tile list at which the first slice ends (include/skyemb.h)."""
    Q, D = tw.shape
    N, P = tokens.shape[:2]
    rowp_sel, tiles, n_live, last_live = prepared[:4]
    code = resident_dtype_code(tokens.dtype, "cosine_topk_tokens_prefiltered_sel")
    ws = _workspace(ws, lib().skyemb_token_prefilter_ws_bytes(Q, D, k), tw.device)
    check(lib().skyemb_cosine_topk_tokens_prefiltered_sel(_p(tw), _p(qn), Q, _p(tokens), code, _p(xn), _p(tail), _p(rowp_sel), _p(tiles),
                                                          n_live, last_live, direct_end, N, P, D, k, combine, eps, idx_offset, _p(thr0),
                                                          _p(ws), ws.numel(), _p(out_s), _p(out_i), _p(redo), _stream()),
          "skyemb_cosine_topk_tokens_prefiltered_sel")
    return ws


def token_topt_prefilter_refusal(Q, N, P, D, k, combine, top_t):
    """None when the two-stage token search takes the shape under ``top_t`` (``combine``: a COMBINE_CODES value), else the library's
    own reason: the plain search's limits, 1 <= top_t <= min(P, 16), and no mean."""
    L = lib()
    return None if L.skyemb_token_topt_prefilter_applicable(Q, N, P, D, k, combine, top_t) else L.skyemb_last_error().decode()


def token_topt_folds(P, combine, top_t):
    """(stage 1 fold, stage 2 fold) the library runs for a two-stage token search under ``top_t`` -- host arithmetic, the rule of
    include/skyemb.h restated: stage 1 'and' | 'or' | 'count', stage 2 'min' | 'max' | 'top'.  'max' and top_t in (0, P) map onto the
    plain search; 'min' with top_t == 1 takes the OR fold and the top-t re-score."""
    if combine == COMBINE_CODES['max']:
        return 'or', 'max'
    assert combine == COMBINE_CODES['min'] and 0 <= top_t <= min(P, 16)
    if top_t in (0, P):
        return 'and', 'min'
    return ('or' if top_t == 1 else 'count'), 'top'


def cosine_topk_tokens_prefiltered_top(tw, qn, tokens, xn, tail, rowp, k, combine, top_t, eps, idx_offset, out_s, out_i, redo, thr0=None,
                                       ws=None):
    """``cosine_topk_tokens_prefiltered`` under the top-t combine (``top_t`` 0: that call; include/skyemb.h): 'min' scores an image
    by its top_t-th best token, 'max' is the plain max."""
    Q, D = tw.shape
    N, P = tokens.shape[:2]
    code = resident_dtype_code(tokens.dtype, "cosine_topk_tokens_prefiltered_top")
    ws = _workspace(ws, lib().skyemb_token_prefilter_ws_bytes(Q, D, k), tw.device)
    check(lib().skyemb_cosine_topk_tokens_prefiltered_top(_p(tw), _p(qn), Q, _p(tokens), code, _p(xn), _p(tail), _p(rowp), N, P, D, k, combine,
                                                          top_t, eps, idx_offset, _p(thr0), _p(ws), ws.numel(), _p(out_s), _p(out_i),
                                                          _p(redo), _stream()), "skyemb_cosine_topk_tokens_prefiltered_top")
    return ws


def cosine_topk_tokens_prefiltered_top_sel(tw, qn, tokens, xn, tail, prepared, direct_end, k, combine, top_t, eps, idx_offset, out_s, out_i,
                                           redo, thr0=None, ws=None):
    """``cosine_topk_tokens_prefiltered_sel`` under the top-t combine (``top_t`` 0: that call; include/skyemb.h)."""
    Q, D = tw.shape
    N, P = tokens.shape[:2]
    rowp_sel, tiles, n_live, last_live = prepared[:4]
    code = resident_dtype_code(tokens.dtype, "cosine_topk_tokens_prefiltered_top_sel")
    ws = _workspace(ws, lib().skyemb_token_prefilter_ws_bytes(Q, D, k), tw.device)
    check(lib().skyemb_cosine_topk_tokens_prefiltered_top_sel(_p(tw), _p(qn), Q, _p(tokens), code, _p(xn), _p(tail), _p(rowp_sel), _p(tiles),
                                                              n_live, last_live, direct_end, N, P, D, k, combine, top_t, eps, idx_offset,
                                                              _p(thr0), _p(ws), ws.numel(), _p(out_s), _p(out_i), _p(redo), _stream()),
          "skyemb_cosine_topk_tokens_prefiltered_top_sel")
    return ws


def prefilter_select_prepare(words, N, rowp):
    """What the two-stage search needs of a selection (packed ``words`` of ``pack_select``) over a bank of N rows with row constants
    ``rowp`` (``bank16_prepare`` / ``bank16_rowp_lp``): (rowp_sel, tiles, n_live, last_live) -- the masked copy of the constants (a
    deselected row holds the padding sentinel), the ascending list of the live 256-row tiles (i32, its first n_live entries), their
    number and whether the bank's last tile is one of them.  Two short launches and one read-back of eight bytes."""
    rows = rowp.shape[0]
    rowp_sel = torch.empty_like(rowp)
    tiles = torch.empty(rows // 256, device=rowp.device, dtype=torch.int32)
    info = torch.empty(2, device=rowp.device, dtype=torch.int32)
    check(lib().skyemb_prefilter_select_prepare(_p(words), N, _p(rowp), _p(rowp_sel), _p(tiles), _p(info), _stream()),
          "skyemb_prefilter_select_prepare")
    n_live, last_live = info.tolist()
    return rowp_sel, tiles, n_live, last_live


def cosine_topk_prefiltered_sel(tw, qn, bank, xn, bank16, tail, prepared, k, eps, idx_offset, out_s, out_i, redo, ws=None):
    """``cosine_topk_prefiltered`` (``bank`` fp32 and its image ``bank16``) or ``cosine_topk_prefiltered_lp`` / ``_resident`` (``bank``
    None: ``bank16`` is the resident fp16 / bf16 bank, ``tail`` its tail tile) under a selection: ``prepared`` is
    ``prefilter_select_prepare``'s result."""
    Q, D = tw.shape
    rowp_sel, tiles, n_live, last_live = prepared
    N = xn.shape[0]
    ws = _workspace(ws, lib().skyemb_topk_prefilter_ws_bytes(Q, D, k), tw.device)
    if bank is not None:                                   # the entry point and its arguments between Q and the masked row constants
        entry, lead = "skyemb_cosine_topk_prefiltered_sel", (_p(bank), _p(xn), _p(bank16))
    elif bank16.dtype == torch.bfloat16:
        entry, lead = "skyemb_cosine_topk_prefiltered_resident_sel", (_p(bank16), dtype_code(bank16.dtype), _p(xn), _p(tail))
    else:
        entry, lead = "skyemb_cosine_topk_prefiltered_lp_sel", (_p(bank16), _p(xn), _p(tail))
    check(getattr(lib(), entry)(_p(tw), _p(qn), Q, *lead, _p(rowp_sel), _p(tiles), n_live, last_live, N, D, k, eps, idx_offset, _p(ws),
                                ws.numel(), _p(out_s), _p(out_i), _p(redo), _stream()), entry)
    return ws


def prefilter_plan(kind, bank, Q, N, D, k, P=1, combine=0, top_t=0, thr0=False, n_live=None, last_live=0, direct_sel=0, lo=-1, eps=1e-6):
    """The launch plan of the two-stage search entry point serving this call, as a `_lib.PrefilterPlan`; touches no device.  kind:
    `_lib.PF_ROWS` / `PF_TOKENS` / `PF_TOKENS_MEAN`; bank: `_lib.PF_BANK_*`; N: rows, images on the token routes; n_live (None: no
    selection), last_live, direct_sel: the selection as the `_sel` entries take it; lo: 0, 1, `_lib.PF_LO_UNSET`, or -1 = what
    SKYEMB_PREFILTER_LO says now.  Raises SkyembError with the entry point's own text where it would refuse."""
    from ._lib import PrefilterPlan, PrefilterRequest
    r = PrefilterRequest(kind, bank, Q, P, D, k, N, combine, top_t, int(bool(thr0)), int(n_live is not None), n_live or 0, last_live,
                         direct_sel, lo, eps)
    p = PrefilterPlan()
    check(lib().skyemb_prefilter_plan(r, p), "skyemb_prefilter_plan")
    return p


def topk_merge(in_s, in_i, Q, nlists, k, out_s, out_i, ws=None):
    """ws: optional int32 [Q] scratch enabling the gather + block-sort path for many short lists."""
    check(lib().skyemb_topk_merge(_p(in_s), _p(in_i), Q, nlists, k, _p(out_s), _p(out_i), _p(ws), _stream()),
          "skyemb_topk_merge")


def cosine_scores(tw, qn, bank, xn, eps, scores):
    Q, D = tw.shape
    N = bank.shape[0]
    check(lib().skyemb_cosine_scores(_p(tw), _p(qn), _p(bank), _p(xn), Q, N, D, eps, _p(scores), _stream()),
          "skyemb_cosine_scores")


COMBINE_CODES = {"min": COMBINE_MIN, "mean": COMBINE_MEAN, "max": COMBINE_MAX}


def cosine_token_applicable(Q, P, D, k):
    """The library's shape predicate of the patch-token search (no device work): see include/skyemb.h."""
    return bool(lib().skyemb_cosine_token_applicable(Q, P, D, k))


def cosine_token_refusal(Q, P, D, k):
    """None when the shape is taken, else the library's own statement of the limits (the predicate leaves it as its error text)."""
    L = lib()
    return None if L.skyemb_cosine_token_applicable(Q, P, D, k) else L.skyemb_last_error().decode()


def cosine_token_topk_chunks(N, P, Q, D, k):
    return lib().skyemb_cosine_token_topk_chunks(N, P, Q, D, k)


def pack_select(flags, words):
    """flags u8 [N] on the device (non-zero = selected) -> words i32 [ceil(N / 32)]: bit i & 31 of word i >> 5 is image i, padding
    bits zero (skyemb_pack_select)."""
    check(lib().skyemb_pack_select(_p(flags), flags.shape[0], _p(words), _stream()), "skyemb_pack_select")


def cosine_token_scores(tw, qn, bank, xn, combine, eps, scores, top_t=0, select=None):
    """bank [N, P, D] fp32, fp16 or bf16, xn [N * P], combine: a COMBINE_* code -> scores [Q, N].  top_t: 0 = all tokens (the
    plain calls), else only the top_t best token scores of an image count (skyemb_cosine_token_scores_top).  select: None, or
    the packed words of a selection of images (pack_select): deselected images score -inf (skyemb_cosine_token_scores_sel)."""
    Q, D = tw.shape
    N, P = bank.shape[0], bank.shape[1]
    if select is not None:
        check(lib().skyemb_cosine_token_scores_sel(_p(tw), _p(qn), _p(bank), bank_dtype_code(bank.dtype, "cosine_token_scores"), _p(xn),
                                                   Q, N, P, D, combine, top_t, eps, _p(scores), _p(select), _stream()),
              "skyemb_cosine_token_scores_sel")
        return
    if top_t != 0:
        check(lib().skyemb_cosine_token_scores_top(_p(tw), _p(qn), _p(bank), bank_dtype_code(bank.dtype, "cosine_token_scores"), _p(xn),
                                                   Q, N, P, D, combine, top_t, eps, _p(scores), _stream()),
              "skyemb_cosine_token_scores_top")
        return
    if bank.dtype != torch.float32:
        check(lib().skyemb_cosine_token_scores_lp(_p(tw), _p(qn), _p(bank), bank_dtype_code(bank.dtype, "cosine_token_scores"), _p(xn),
                                                  Q, N, P, D, combine, eps, _p(scores), _stream()), "skyemb_cosine_token_scores_lp")
        return
    check(lib().skyemb_cosine_token_scores(_p(tw), _p(qn), _p(bank), _p(xn), Q, N, P, D, combine, eps, _p(scores), _stream()),
          "skyemb_cosine_token_scores")


def cosine_token_topk(tw, qn, bank, xn, k, combine, eps, idx_offset, nlists, part_s, part_i, thr0=None, top_t=0, select=None):
    Q, D = tw.shape
    N, P = bank.shape[0], bank.shape[1]
    if select is not None:
        check(lib().skyemb_cosine_token_topk_sel(_p(tw), _p(qn), _p(bank), bank_dtype_code(bank.dtype, "cosine_token_topk"), _p(xn), Q,
                                                 N, P, D, k, combine, top_t, eps, idx_offset, nlists, _p(thr0), _p(part_s), _p(part_i),
                                                 _p(select), _stream()), "skyemb_cosine_token_topk_sel")
        return
    if top_t != 0:
        check(lib().skyemb_cosine_token_topk_top(_p(tw), _p(qn), _p(bank), bank_dtype_code(bank.dtype, "cosine_token_topk"), _p(xn), Q,
                                                 N, P, D, k, combine, top_t, eps, idx_offset, nlists, _p(thr0), _p(part_s), _p(part_i),
                                                 _stream()), "skyemb_cosine_token_topk_top")
        return
    if bank.dtype != torch.float32:
        check(lib().skyemb_cosine_token_topk_lp(_p(tw), _p(qn), _p(bank), bank_dtype_code(bank.dtype, "cosine_token_topk"), _p(xn), Q, N,
                                                P, D, k, combine, eps, idx_offset, nlists, _p(thr0), _p(part_s), _p(part_i), _stream()),
              "skyemb_cosine_token_topk_lp")
        return
    check(lib().skyemb_cosine_token_topk(_p(tw), _p(qn), _p(bank), _p(xn), Q, N, P, D, k, combine, eps, idx_offset, nlists, _p(thr0),
                                         _p(part_s), _p(part_i), _stream()), "skyemb_cosine_token_topk")


METRIC_CODES = {"MSE": METRIC_MSE, "MAE": METRIC_MAE}     # the distance metrics of the patch-token search (SKYEMB_METRIC_*)


def distance_token_scores(c, t, bank, metric, combine, scores, top_t=0, select=None):
    """c [D] = fp32(w / sum(w)), t [Q, D] queries, bank [N, P, D] fp32, fp16 or bf16, metric: a METRIC_* code, combine: a COMBINE_*
    code -> scores [Q, N] combined DISTANCES (+inf for an image the packed ``select`` words leave out).  include/skyemb.h."""
    Q, D = t.shape
    N, P = bank.shape[0], bank.shape[1]
    check(lib().skyemb_distance_token_scores(_p(c), _p(t), _p(bank), bank_dtype_code(bank.dtype, "distance_token_scores"), Q, N, P, D,
                                             metric, combine, top_t, _p(scores), _p(select), _stream()), "skyemb_distance_token_scores")


def distance_token_topk(c, t, bank, metric, combine, k, idx_offset, nlists, part_s, part_i, thr0=None, top_t=0, select=None):
    """Per-wave lists [Q, nlists, k] in KEY space (part_s = -distance, best first; nlists: cosine_token_topk_chunks), which
    topk_merge merges as they are.  thr0 [Q]: key floors.  include/skyemb.h."""
    Q, D = t.shape
    N, P = bank.shape[0], bank.shape[1]
    check(lib().skyemb_distance_token_topk(_p(c), _p(t), _p(bank), bank_dtype_code(bank.dtype, "distance_token_topk"), Q, N, P, D, metric,
                                           combine, top_t, k, idx_offset, nlists, _p(thr0), _p(part_s), _p(part_i), _p(select), _stream()),
          "skyemb_distance_token_topk")


# ---- per-query feature weights: every query of a call has its own row of w / c [Q, D] (include/skyemb.h)
def cosine_token_pq_refusal(Q, P, D, k):
    """cosine_token_refusal for the calls with per-query weights (two operand images in LDS: 128 D + 32 Q k <= 163840)."""
    L = lib()
    return None if L.skyemb_cosine_token_pq_applicable(Q, P, D, k) else L.skyemb_last_error().decode()


def cosine_token_scores_pq(tw, qn, bank, w, combine, eps, scores, top_t=0, select=None):
    """cosine_token_scores with w [Q, D] in place of the bank norms: the norm of a row under query q's weights is computed in the
    pass (skyemb_cosine_token_scores_pq)."""
    Q, D = tw.shape
    N, P = bank.shape[0], bank.shape[1]
    check(lib().skyemb_cosine_token_scores_pq(_p(tw), _p(qn), _p(bank), bank_dtype_code(bank.dtype, "cosine_token_scores_pq"), _p(w), Q, N,
                                              P, D, combine, top_t, eps, _p(scores), _p(select), _stream()),
          "skyemb_cosine_token_scores_pq")


def cosine_token_topk_pq(tw, qn, bank, w, k, combine, eps, idx_offset, nlists, part_s, part_i, thr0=None, top_t=0, select=None):
    Q, D = tw.shape
    N, P = bank.shape[0], bank.shape[1]
    check(lib().skyemb_cosine_token_topk_pq(_p(tw), _p(qn), _p(bank), bank_dtype_code(bank.dtype, "cosine_token_topk_pq"), _p(w), Q, N, P,
                                            D, k, combine, top_t, eps, idx_offset, nlists, _p(thr0), _p(part_s), _p(part_i), _p(select),
                                            _stream()), "skyemb_cosine_token_topk_pq")


def distance_token_scores_pq(c, t, bank, metric, combine, scores, top_t=0, select=None):
    """distance_token_scores with c [Q, D]: row q = fp32(w_q / sum(w_q)) serves query q (skyemb_distance_token_scores_pq)."""
    Q, D = t.shape
    N, P = bank.shape[0], bank.shape[1]
    check(lib().skyemb_distance_token_scores_pq(_p(c), _p(t), _p(bank), bank_dtype_code(bank.dtype, "distance_token_scores_pq"), Q, N, P,
                                                D, metric, combine, top_t, _p(scores), _p(select), _stream()),
          "skyemb_distance_token_scores_pq")


def distance_token_topk_pq(c, t, bank, metric, combine, k, idx_offset, nlists, part_s, part_i, thr0=None, top_t=0, select=None):
    Q, D = t.shape
    N, P = bank.shape[0], bank.shape[1]
    check(lib().skyemb_distance_token_topk_pq(_p(c), _p(t), _p(bank), bank_dtype_code(bank.dtype, "distance_token_topk_pq"), Q, N, P, D,
                                              metric, combine, top_t, k, idx_offset, nlists, _p(thr0), _p(part_s), _p(part_i), _p(select),
                                              _stream()), "skyemb_distance_token_topk_pq")


# ---- linear-probe fits on the device (csrc/probe.hip; driven by sky_embeddings_amd/probe.py)
def probe_colstats(X, n=None, F=None, ldx=None):
    """X [n, F] fp32 (row stride ``ldx`` elements) -> (mean, var, scale) fp64 [F]; scale is exactly 1 where var == 0."""
    n, F = (X.shape[0] if n is None else n), (X.shape[1] if F is None else F)
    mean, var, scale = (torch.empty(F, device=X.device, dtype=torch.float64) for _ in range(3))
    ws = torch.empty(_lib.PROBE_CHUNKS * F, device=X.device, dtype=torch.float64)
    check(lib().skyemb_probe_colstats(_p(X), X.stride(0) if ldx is None else ldx, n, F, _p(mean), _p(var), _p(scale), _p(ws), _stream()),
          "skyemb_probe_colstats")
    return mean, var, scale


def probe_scale(X, mean, scale, out, n=None, F=None, ldx=None, ldo=None):
    """out = fp32((X - mean) / scale) (``scale`` None: centre only)."""
    n, F = (X.shape[0] if n is None else n), (X.shape[1] if F is None else F)
    check(lib().skyemb_probe_scale(_p(X), X.stride(0) if ldx is None else ldx, n, F, _p(mean), _p(scale), _p(out),
                                   out.stride(0) if ldo is None else ldo, _stream()), "skyemb_probe_scale")
    return out


def probe_softmax_ws_bytes(m, F, K):
    return int(lib().skyemb_probe_softmax_ws_bytes(m, F, K))


def probe_softmax_loss_grad(X, y, W, b, l2, loss, gW, gb, ws, m=None, F=None, K=None, ldx=None):
    m, F, K = (X.shape[0] if m is None else m), (X.shape[1] if F is None else F), (W.shape[0] if K is None else K)
    check(lib().skyemb_probe_softmax_loss_grad(_p(X), X.stride(0) if ldx is None else ldx, _p(y), m, F, K, _p(W), _p(b), float(l2), _p(loss),
                                               _p(gW), _p(gb), _p(ws), 0 if ws is None else ws.numel() * ws.element_size(), _stream()),
          "skyemb_probe_softmax_loss_grad")


def probe_gram(Xc, yc, G, q, ynorm2, m=None, F=None, ldx=None):
    m, F = (Xc.shape[0] if m is None else m), (Xc.shape[1] if F is None else F)
    check(lib().skyemb_probe_gram(_p(Xc), Xc.stride(0) if ldx is None else ldx, _p(yc), m, F, _p(G), _p(q), _p(ynorm2), _stream()),
          "skyemb_probe_gram")


def probe_enet_cd(G, q, ynorm2, a1, b2, max_iter, tol, w, status, gap, F=None):
    F = q.numel() if F is None else F
    check(lib().skyemb_probe_enet_cd(_p(G), _p(q), _p(ynorm2), F, float(a1), float(b2), int(max_iter), float(tol), _p(w), _p(status),
                                     _p(gap), _stream()), "skyemb_probe_enet_cd")
