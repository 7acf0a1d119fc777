/*
 * skyemb.h -- C ABI of libskyemb (MI355X / gfx950 hot path of sky_embeddings).
 *
 * The reference (teaghan/sky_embeddings) has no FFI layer: its hot path is Python
 * (torch + timm).  This header is the lower drop-in boundary the build inserts beneath
 * the reference's module API: every entry point below names the
 * reference lines (paths relative to the reference root) whose arithmetic it replaces.
 *
 * Conventions
 *   - plain C, raw DEVICE pointers + sizes, no torch types; caller owns every buffer
 *     (workspaces included); nothing is allocated or freed inside the library;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no host
 *     synchronisation, safe under stream capture (hipGraph);
 *   - return 0 on success, non-zero on error with the text in skyemb_last_error()
 *     (thread-local);
 *   - `dtype` selects the ACTIVATION element type of the call: SKYEMB_BF16 / SKYEMB_F16
 *     (throughput modes: 16-bit operands on v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulate)
 *     or SKYEMB_F32 (parity mode: exact-fp32 v_mfma_f32_16x16x4_f32).  Statistics, losses, the
 *     residual stream, gradients of parameters and optimiser state are always fp32.
 */
#ifndef SKYEMB_H
#define SKYEMB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKYEMB_BF16 0
#define SKYEMB_F32 1
#define SKYEMB_F16 2 /* IEEE half operands on v_mfma_f32_16x16x32_f16 (same rate as bf16, 11-bit significand): the throughput mode
                        that holds loss and reconstructed pixels within 1e-3 of the fp32 reference.  Every
                        `dtype` argument below that accepts SKYEMB_BF16 accepts SKYEMB_F16 with the same layouts and constraints.
                        fp16 underflows where bf16 does not: the caller scales d loss / d pred (`dscale` of the loss entry points)
                        and removes the factor in skyemb_adamw's / skyemb_adamw_desc's grad_scale. */

/* operand layouts of skyemb_gemm (logical A[M,K], B[N,K]; C = A * B^T) */
#define SKYEMB_KC 0 /* k contiguous:   X(r,k) at X[r*ld + k] */
#define SKYEMB_RC 1 /* row contiguous: X(r,k) at X[k*ld + r] */

/* epilogue activations */
#define SKYEMB_ACT_NONE 0
#define SKYEMB_ACT_GELU 1  /* out = gelu(v) (exact erf); out2 = v (pre-activation)  */
#define SKYEMB_ACT_DGELU 2 /* out = v * gelu'(aux)                                  */

const char *skyemb_last_error(void);
int skyemb_version(void);
/* Measurement aid for bench.py: entry points of the kernel families in `mask` return 0 without launching (bit 0: the MFMA
 * GEMM launches), so a timed region with and without them gives the family's in-step time.  Returns the previous mask.
 * MEASUREMENT BUILD ONLY: libskyemb_measure.so (-DSKYEMB_MEASURE).  In the product library (libskyemb.so) the switch is not
 * compiled in: the call returns -1 with skyemb_last_error set and no launch can ever be skipped. */
int skyemb_debug_skip(int mask);
/* Diagnostic: launches issued so far by each GEMM kernel family of this process (out[i] for the slots below; reset != 0 zeroes
 * them after reading).  Tests use it to assert that a shape ran on the kernel it is meant to exercise (e.g. the 256 x 256 tile
 * at ViT-L width); no product path reads it. */
#define SKYEMB_GEMM_COUNT_FALLBACK 0 /* gemm.hip: register-staged kernel (fp32 parity mode, shapes outside the pipe subset) */
#define SKYEMB_GEMM_COUNT_PIPE 1     /* gemm_pipe_kernel: LDS-DMA ring, every tile shape but 256 x 256                       */
#define SKYEMB_GEMM_COUNT_256 2      /* gemm256_kernel / gemm256_wgrad_kernel: single 256 x 256 launches                     */
#define SKYEMB_GEMM_COUNT_GROUP 3    /* gemm_pipe_group_kernel: grouped launches on ring tiles                               */
#define SKYEMB_GEMM_COUNT_GROUP256 4 /* gemm256_group_kernel: grouped launches on 256 x 256 tiles                            */
#define SKYEMB_GEMM_COUNT_SPLITK 5   /* splitk_reduce_kernel                                                                 */
#define SKYEMB_GEMM_COUNT_SLOTS 8
int skyemb_gemm_launch_counts(long long *out, int n, int reset);

/* ---------------------------------------------------------------- GEMM ----
 * Replaces every nn.Linear / Conv2d(k=s=p) contraction of timm PatchEmbed / Block /
 * the MAE decoder (utils/mim_vit.py:206,231-233,269,276-281) and their autograd
 * backward (dgrad, wgrad) (utils/pretrain_fns.py:34).
 *
 *   v[m,n]   = alpha * sum_k A(m,k) * B(n,k)  + bias[n] + table[tab_row[m], n] + resid[orow, n]
 *   orow     = dst_row ? dst_row[m] : m        (orow < 0: row is not stored)
 *   out_f32[orow, n] / out[orow, n] / out2[orow, n] per `act` (see above).
 * A, B, aux, out, out2 have element type `dtype`; bias/table/resid/out_f32 are fp32.
 * Constraint: the contiguous extent of A and of B (K for KC, rows for RC) is a
 * multiple of 8 (bf16) / 4 (f32) elements and 16-byte aligned.
 */
typedef struct skyemb_gemm_args {
    const void *A;
    const void *B;
    int64_t lda, ldb;
    int32_t a_layout, b_layout; /* SKYEMB_KC / SKYEMB_RC */
    int32_t M, N, K;
    int32_t dtype;
    float alpha;
    const float *bias;          /* [N] or NULL */
    const float *table;         /* fp32 rows added by index, or NULL */
    const int32_t *tab_row;     /* [M] */
    int64_t ldt;
    const int32_t *dst_row;     /* [M] or NULL */
    const float *resid;         /* fp32 [*, ldr] or NULL (indexed by orow) */
    int64_t ldr;
    const void *aux;            /* dtype [M, ldaux] (ACT_DGELU), indexed by m */
    int64_t ldaux;
    int32_t act;
    float *out_f32;             /* or NULL */
    int64_t ldo32;
    void *out;                  /* dtype, or NULL */
    int64_t ldo;
    void *out2;                 /* dtype, or NULL (ACT_GELU pre-activation) */
    int64_t ldo2;
    int32_t tile;               /* 0 = auto, 64 or 128 */
    float *colsum_a;            /* optional, A must be RC: colsum_a[m] = sum_k A(m,k)  (bias gradient fused
                                   into the wgrad launch: A = dy, so this is sum over tokens of dy[:, m]) */
    void *ws;                   /* optional fp32 workspace enabling split-K: partial slabs [split][M][N] + [split][M]
                                   are summed by a second launch in a fixed order (deterministic), which applies
                                   the epilogue.  One workspace per stream. */
    int64_t ws_bytes;
    int32_t split_k;            /* 0 = auto (1 when ws == NULL), 1 = off, n = force n-way */
    int32_t prefetch_wgs;       /* resolved by the library (callers leave 0): workgroups behind the tiles that carry the prefetch hint */
    const void *prefetch;       /* optional hint, no effect on results: `prefetch_bytes` bytes (a multiple of 4, 4-byte aligned) that a LATER
                                   launch will read -- the next layer's weight matrix -- are touched once by this launch's workgroups
                                   (one 4-byte LDS-DMA read per 128-byte line, ahead of their first operand loads), so that they sit in
                                   the memory-side cache when that launch starts instead of coming from HBM inside its k-loops.
                                   Where the launch leaves workgroup slots of the device free, extra workgroups behind its tiles do the
                                   touching (the tiles' own request queues stay clear); else the tiles' waves do, ahead of their first loads.
                                   Honoured by the pipelined bf16 kernels (gemm_pipe.hip); ignored elsewhere. */
    int64_t prefetch_bytes;
} skyemb_gemm_args;

int skyemb_gemm(const skyemb_gemm_args *args, void *stream);

/* Grouped launch: n <= 32 independent 16-bit problems (all bf16 or all f16) run as ONE grid (the four weight-gradient GEMMs of a transformer
 * block fill the chip together: no split-K, no reduce launch).
 * skyemb_gemm_group_plan validates the problems and fills a HOST blob of skyemb_gemm_group_blob_bytes(n) bytes; the
 * caller copies it to device memory once (pointers inside are fixed) and replays skyemb_gemm_group_launch.
 * plan returns -1 (with skyemb_last_error set) when a problem is outside the subset: launch them singly then.
 * A plan that returns 0 names a launch that is built: skyemb_gemm_group_launch of its blob and info does not refuse the group for its
 * tile, class mask or format (a KC.RC + RC.RC mix on a tile without the mixed instance, 9128128, is refused by the plan). */
typedef struct skyemb_gemm_group_info {
    int32_t total_blocks; /* grid size of the launch                                                          */
    int32_t tile;         /* tile code the plan chose (BM * 1000 + BN): 64064, 128064, 128128 or 256256        */
    int32_t class_mask;   /* operand-layout classes present: 1 KC.KC, 2 KC.RC (dgrad), 4 RC.RC (wgrad)        */
    int32_t reserved;     /* bit 0: the tiles' epilogue is the AdamW step (plan_adamw); bit 1: side jobs (plan_side_adamw, attach_ln_bwd);
                             bit 2: the problems are SKYEMB_F16 */
} skyemb_gemm_group_info;
int64_t skyemb_gemm_group_blob_bytes(int n);
/* tile = 0: chosen from the total tile count.  The problems share ONE tile shape and may mix the data-gradient
 * (KC.RC) and weight-gradient (RC.RC) layout classes: a Linear's dX and dW read the same dY and do not depend on
 * each other, so one launch computes both. */
int skyemb_gemm_group_plan(const skyemb_gemm_args *args, int n, int tile, void *blob_host, int64_t blob_bytes,
                           skyemb_gemm_group_info *info);
int skyemb_gemm_group_launch(const void *blob_dev, const skyemb_gemm_group_info *info, void *stream);
/* The same grouped weight-gradient launch with the optimiser step fused into its epilogue (one process per model replica only:
 * with N > 1 the gradients are summed over the ranks between backward and AdamW).  Every problem's out_f32 points into the flat
 * gradient buffer `g_base`; p / m / v / p_lp are the flat parameter, moment and low-precision-shadow buffers with the SAME element
 * offsets.  An output tile is then not stored as a gradient at all: the kernel reads p, m, v, applies torch.optim.AdamW's update
 * to them (utils/mim_vit.py:126-129, utils/pretrain_fns.py:36-41; bit-identical to skyemb_adamw on the stored gradient) and writes
 * p, m, v and the bf16 shadow -- 26 instead of 4 + 30 bytes per parameter through HBM, and no separate pass over those tensors.
 * hyper: device fp32[4] {lr, 1 - beta1^t, 1 - beta2^t} of the step being taken (written before the launch: graph-safe).
 * Elements of the flat buffers below n_decay are weight-decayed.  bias gradients (colsum_a) are still stored as gradients.
 * RC.RC problems only; plan it with skyemb_gemm_group_plan_adamw, launch it with skyemb_gemm_group_launch. */
typedef struct skyemb_adamw_desc {
    float *g_base, *p, *m, *v;
    void *p_lp;            /* 16-bit shadow of p, in the format of the group's problems (bf16 / f16) */
    const float *hyper;
    int64_t n_decay;
    float beta1, beta2, eps, weight_decay, grad_scale;
    int32_t enabled;       /* set by the plan */
} skyemb_adamw_desc;
int skyemb_gemm_group_plan_adamw(const skyemb_gemm_args *args, int n, int tile, const skyemb_adamw_desc *adamw, void *blob_host,
                                 int64_t blob_bytes, skyemb_gemm_group_info *info);
/* The optimiser step as a SIDE JOB of a grouped weight-gradient launch (round 5).  In the epilogue form above a tile's parameters are
 * stepped after that tile's own k-loop: every tile ends at the same moment, so the launch is a matrix phase followed by an HBM
 * phase.  Here `side_blocks` extra workgroups behind the launch's tiles step the slice [side_lo, side_hi) of the flat buffers --
 * the weights whose gradients the PREVIOUS grouped launch of the backward pass stored in g_base (skyemb_adamw on that slice, bit
 * for bit) -- while the tile workgroups multiply: they are dispatched into the slots the tiles leave free (a grouped launch
 * rarely fills the chip evenly: 192 tiles of 256 x 256 for 256 compute units at ViT-L) and into the tiles' slots as those finish.
 * own_step = 0: the launch's own tiles are stored as gradients (a later launch's side job, or skyemb_adamw, steps them);
 * own_step = 1: they are stepped in the epilogue as with skyemb_gemm_group_plan_adamw (the LAST block of a backward pass: nothing
 * follows it that could carry its step).  An empty side range (side_lo == side_hi, side_blocks = 0) is allowed.  RC.RC problems
 * only; launch with skyemb_gemm_group_launch.  info->reserved: bit 0 = own_step, bit 1 = side job. */
int skyemb_gemm_group_plan_side_adamw(const skyemb_gemm_args *args, int n, int tile, const skyemb_adamw_desc *adamw, int own_step,
                                      int64_t side_lo, int64_t side_hi, int side_blocks, void *blob_host, int64_t blob_bytes,
                                      skyemb_gemm_group_info *info);
/* A LayerNorm backward as a SIDE JOB of a planned grouped weight-gradient launch (round 5): the backward of a transformer block's
 * norm1 (timm Block: x + attn(norm1(x)); utils/mim_vit.py:231-233 through autograd) depends on the block's qkv data gradient only,
 * not on its weight gradients -- so instead of a launch of its own behind the grouped launch, its rows are taken by extra workgroups
 * inside it (bf16 compute dtype; same rows per four-wave block, same partial-sum table and same bits as skyemb_layernorm_bwd with
 * dgamma = dbeta = NULL: the caller reduces `part` as before).  Call AFTER skyemb_gemm_group_plan / _plan_adamw / _plan_side_adamw
 * on the same host blob (weight-gradient groups only); grows info->total_blocks and sets bit 1 of info->reserved.  D <= 1024 on 256 x 256 tiles, <= 768 on the ring tiles. */
typedef struct skyemb_ln_bwd_side {
    const void *dy;             /* [M, D] bf16: d loss / d (LayerNorm output) */
    const float *x, *gamma, *mean, *rstd;
    const float *g_in;          /* fp32 residual gradient added to the result (may equal g_out), or NULL */
    float *g_out;               /* [M, D] fp32 */
    void *g_lp;                 /* [M, D] bf16 copy of g_out, or NULL */
    float *part;                /* [2, skyemb_layernorm_bwd_blocks(M), D] */
    int32_t M, D;
} skyemb_ln_bwd_side;
int skyemb_gemm_group_attach_ln_bwd(void *blob_host, int64_t blob_bytes, skyemb_gemm_group_info *info, const skyemb_ln_bwd_side *ln);

/* column sums: out[n] = sum_m X[m,n]; X is `dtype` (bias gradients) or fp32 partials
 * (LayerNorm dgamma/dbeta second stage).  Replaces autograd's bias-gradient reductions. */
int skyemb_colsum(const void *X, int dtype, int64_t ldx, int M, int N, float *out, void *stream);

/* ----------------------------------------------------------- front end ----
 * utils/mim_vit.py:354-379 random_masking with the noise supplied by the caller
 * (ties -> lower index).  noise [B,L] -> ids_restore i64 [B,L], mask f32 [B,L]
 * (1 = removed), ids_keep i32 [B,keep] (first `keep` of the shuffle, in shuffle order).
 * Optional (NULL to skip) decoder un-shuffle maps for utils/mim_vit.py:446-453, one entry per
 * encoder token (the n_extra = 1 (cls) or 2 (cls, RA/Dec) extra tokens first): dec_dst i32 [B,n_extra+keep] = row of
 * the [B,n_extra+L] decoder sequence the token lands on, dec_tab i32 [B,n_extra+keep] = its decoder_pos_embed row. */
int skyemb_random_mask_from_noise(const float *noise, int B, int L, int keep, int64_t *ids_restore, float *mask,
                                  int32_t *ids_keep, int32_t *dec_dst, int32_t *dec_tab, int n_extra, void *stream);
/* SimMIM mask generator on the device (replaces utils/dataloaders.py:197-219 MaskGenerator.__call__, which runs per item in
 * the loader workers): per sample ratio = ratio_u[b] * max_ratio, count = ceil(L * ratio); per channel the `count` patches
 * with the smallest noise[b, c, :] are masked (a uniformly random subset, like randperm(L)[:count]); out_mask float 0 / 1
 * [B, C, grid*p, grid*p].  noise [B, C, L] and ratio_u [B] are uniform [0, 1) draws supplied by the caller.
 * Both generators take L <= 4096 (here L == grid * grid, p % 4 == 0, 0 <= max_ratio <= 1): a row of noise is ranked in LDS, 16 L
 * bytes per workgroup in skyemb_random_mask_from_noise (64 KB at the limit) and 32 L bytes here (128 KB at the limit; above 64 KB
 * the kernel's dynamic-LDS limit is raised first).  Any other shape returns 1 before any launch, skyemb_last_error set. */
int skyemb_simmim_mask_from_noise(const float *noise, const float *ratio_u, double max_ratio, int B, int C, int L, int grid, int p,
                                  float *out_mask, void *stream);

/* utils/mim_vit.py:385-392 + the im2row half of timm PatchEmbed (:206,402): for every kept
 * patch (b, ids_keep[b,j]) write the row  out[b*keep + j, c*p*p + py*p + px] =
 * isnan(x) ? pmv[c,py,px] : (x - mean)/std   in `dtype`.  ids_keep == NULL: all L patches in order. */
int skyemb_patch_gather(const float *imgs, const float *pmv, const int32_t *ids_keep, void *out, int dtype, int B,
                        int C, int H, int W, int p, int keep, float pixel_mean, float pixel_std, void *stream);

/* SimMIM mode (utils/mim_vit.py:394-399): same with  x = x * (1 - mask) + pmv * mask  after the NaN fill;
 * pixel_mask fp32 [B,C,H,W], 1 = hidden.  The matching patch_mask_values gradient weights drows by
 * d x / d pmv = isnan(pixel) ? 1 : pixel_mask. */
int skyemb_patch_gather_blend(const float *imgs, const float *pmv, const int32_t *ids_keep, const float *pixel_mask, void *out,
                              int dtype, int B, int C, int H, int W, int p, int keep, float pixel_mean, float pixel_std,
                              void *stream);
int skyemb_patch_gather_bwd_pmv_blend(const float *imgs, const int32_t *ids_keep, const float *pixel_mask, const float *drows,
                                      float *partial, float *dpmv, int B, int C, int H, int W, int p, int keep, void *stream);

/* RA/Dec token (utils/mim_vit.py:209-216, 410-414; utils/location_encoder.py:138-243): real spherical harmonics
 * (l < 5, 25 features) -> sin(30 (W0 sh + b0)) [8] -> W1 h + b1 (+ pos_row) written to x[b * row_stride + d], d < D.
 * sh [B,25] and z [B,8] (pre-sine) are saved for the backward, which takes g = d loss / d token rows (same stride) and
 * returns the four parameter gradients (dz_ws: fp32 [B,8] scratch).  Batch reductions run in a fixed order. */
int skyemb_radec_token_fwd(const float *ra_dec, const float *W0, const float *b0, const float *W1, const float *b1,
                           const float *pos_row, float *x, int64_t row_stride, int B, int D, float *sh, float *z, void *stream);
int skyemb_radec_token_bwd(const float *g, int64_t row_stride, const float *W1, const float *sh, const float *z, float *dz_ws,
                           float *dW0, float *db0, float *dW1, float *db1, int B, int D, void *stream);

/* gradient of patch_mask_values: dpmv[c,py,px] = sum over gathered NaN pixels of drows (fp32
 * [B*keep, C*p*p]); deterministic two-stage reduction, `partial` is fp32 [B, C*p*p]. */
int skyemb_patch_gather_bwd_pmv(const float *imgs, const int32_t *ids_keep, const float *drows, float *partial,
                                float *dpmv, int B, int C, int H, int W, int p, int keep, void *stream);

/* -------------------------------------------------------- LayerNorm -------
 * nn.LayerNorm(eps=1e-6) of timm Block.norm1/norm2 and the final norms
 * (utils/mim_vit.py:236,280,429,458).  x fp32 [M,D] -> y dtype [M,D] (+ y32 fp32 copy if
 * non-NULL), mean/rstd fp32 [M]. */
int skyemb_layernorm_fwd(const float *x, const float *gamma, const float *beta, void *y, float *y32, int dtype,
                         float *mean, float *rstd, int M, int D, float eps, void *stream);

/* dx = LN'(dy); g_out = (g_in ? g_in : 0) + dx (fp32; g_out may alias g_in); g_lp = dtype copy
 * of g_out (or NULL).  dy is `dtype` (or fp32 when dy_is_f32).  dgamma/dbeta: deterministic two-stage
 * reduction through part[2, nblk, D] (fp32 workspace, nblk = skyemb_layernorm_bwd_blocks(M)). */
int skyemb_layernorm_bwd_blocks(int M);
/* dgamma == NULL: leave the partial sums in `part` for skyemb_layernorm_bwd_reduce_batch, which finishes the
 * dgamma / dbeta of many LayerNorms (e.g. all of one backward stage) in ONE launch; `items` is a DEVICE array. */
typedef struct {
    const float *part;   /* [2, nblk, D] written by skyemb_layernorm_bwd */
    float *dgamma, *dbeta;      /* dbeta == NULL: a single vector (part [nblk][D] -> dgamma) */
    int32_t nblk, D;
} skyemb_ln_reduce_item;
/* blocks: device int32 pairs {item index into `items`, x | y << 16}, one per workgroup: columns [32 x, +32) of half y (0 = dgamma,
 * 1 = dbeta) of that item.  The caller lists ceil(D / 32) pairs per half of every item of the stage (a flat list: items of
 * different widths share the launch without idle workgroups). */
int skyemb_layernorm_bwd_reduce_batch(const skyemb_ln_reduce_item *items, const int32_t *blocks, int n_blocks, void *stream);
int skyemb_layernorm_bwd(const void *dy, int dy_is_f32, int dtype, const float *x, const float *gamma,
                         const float *mean, const float *rstd, const float *g_in, float *g_out, void *g_lp,
                         float *part, float *dgamma, float *dbeta, int M, int D, void *stream);

/* -------------------------------------------------------- attention -------
 * timm Attention core / F.scaled_dot_product_attention, no mask, 1 <= N <= SKYEMB_MHA_MAX_N tokens
 * (the front end's 4096 patches + cls + RA/Dec), any head dim hd % 8 == 0 (hd <= 512 once a head outgrows LDS):
 * qkv dtype [B, N, 3, H, hd] -> out dtype [B, N, H*hd];  softmax(q k^T hd^-0.5) v in fp32.
 * bf16 / fp16 at hd 32 / 64 run on MFMA (N > 128: K/V streamed through LDS, online softmax); other shapes run fp32
 * kernels.  Backward recomputes the probabilities from q, k; it needs no workspace and is deterministic.
 * N > SKYEMB_MHA_MAX_N returns 1 before anything is launched. */
#define SKYEMB_MHA_MAX_N 4098
int skyemb_mha_fwd(const void *qkv, void *out, int dtype, int B, int N, int H, int hd, void *stream);
int skyemb_mha_bwd(const void *qkv, const void *dout, void *dqkv, int dtype, int B, int N, int H, int hd,
                   void *stream);
/* Read-only query (additive to ABI version 111: nothing above changes): the launch skyemb_mha_fwd (bwd = 0) / skyemb_mha_bwd
 * (bwd != 0) makes for this shape.  Validates as they do (same texts, same return code 1) and touches no device.
 * `switches`: -1 = what the process's environment says (SKYEMB_MHA_MFMA, SKYEMB_MHA_WPB, read once), else SKYEMB_MHA_SW_* bits. */
#define SKYEMB_MHA_LDS 0         /* whole heads in LDS as fp32: `waves` heads per workgroup, `per_wave_floats` each           */
#define SKYEMB_MHA_STREAM 1      /* the fp32 streaming kernels: a head that outgrows LDS                                      */
#define SKYEMB_MHA_MFMA_PACKED 2 /* N <= 16: 32 / N samples per 32-row tile; `waves` = tiles per workgroup (1 or 4) of `nheads` */
#define SKYEMB_MHA_MFMA_SINGLE 3 /* 16 < N <= 32: one (sample, head) per tile; `waves`, `nheads` as above                      */
#define SKYEMB_MHA_MFMA_STRIP 4  /* 32 < N <= 128: `waves` = strips of 32 tokens (2, 3, 4)                                    */
#define SKYEMB_MHA_MFMA_LONG 5   /* N > 128: K / V streamed through LDS                                                       */
#define SKYEMB_MHA_SW_NO_MFMA 1  /* SKYEMB_MHA_MFMA=0                                                                         */
#define SKYEMB_MHA_SW_WPB1 2     /* SKYEMB_MHA_WPB=1                                                                          */
#define SKYEMB_MHA_SW_WPB4 4     /* SKYEMB_MHA_WPB=<any other non-zero number>                                                */
typedef struct {
    int32_t family;                  /* SKYEMB_MHA_* above */
    int32_t hd;                      /* the MFMA kernels' head-dim instance (32 / 64); 0 for lds and stream */
    int32_t waves;                   /* waves per workgroup: the kernel's template or run-time parameter named per family above */
    int32_t per_wave_floats, nheads; /* lds / packed and single; 0 elsewhere */
    int32_t grid_x, grid_y, block;
    int64_t lds_bytes;               /* dynamic LDS of the launch */
    int64_t lds_limit;               /* the dynamic-LDS limit the kernel needs raised before it (0: none) */
} skyemb_mha_plan_t;
int skyemb_mha_plan(int bwd, int dtype, int B, int N, int H, int hd, int switches, skyemb_mha_plan_t *out);

/* -------------------------------------------------------- decoder glue ----
 * utils/mim_vit.py:446-453: rows of the decoder sequence that hold a mask token:
 * x[b, 1+l, :] = mask_token + dec_pos[1+l] for every l with mask[b,l]==1 (x fp32 [B, 1+L, Dd]). */
int skyemb_fill_mask_tokens(float *x, const float *mask, const float *mask_token, const float *dec_pos, int B,
                            int L, int Dd, int n_extra, void *stream);
/* gather fp32 rows: out[i, :] = src[idx[i], :] (also emits a dtype copy when out_lp != NULL) */
int skyemb_gather_rows(const float *src, const int32_t *idx, float *out, void *out_lp, int dtype, int n_rows,
                       int D, void *stream);
/* selected row sum (d mask_token, d cls_token): out[d] = sum_i [sel == NULL || sel[i] != 0] src[r(i)*ld + d],
 * r(i) = row0 + (i / inner) * outer_stride + (i % inner), i in [0, n_rows); `partial` fp32 [256, D]. */
int skyemb_rowsum_select(const float *src, int64_t ld, const float *sel, int row0, int inner, int outer_stride,
                         int n_rows, int D, float *partial, float *out, void *stream);

/* ------------------------------------------------------------- loss -------
 * utils/mim_vit.py:326-338,473-521,614-627: patchify + NaN-aware per-patch mean / biased
 * variance normalisation + masked MSE (loss_l1 == 0) or L1 + NaN exclusion.
 * pred fp32 [B, Nd, pv] with the first `extra` rows of each sample ignored (cls / ra_dec).
 * Outputs: loss (fp32 scalar, device), dpred dtype/fp32 [B, Nd, pv] (extra + unmasked rows
 * zero) = dscale * d loss / d pred.  NaN target elements contribute zero gradient (DESIGN.md deviation).
 * dscale: static loss scale of the backward pass (1 = none; a power of two for SKYEMB_F16, whose data gradients would
 * underflow otherwise -- every later step of backward is linear in dpred, so the caller divides it out again through
 * grad_scale of skyemb_adamw / skyemb_adamw_desc); `loss` itself is never scaled.
 * `ws` fp32 workspace of 4*B*L + 4 floats.  p % 4 == 0, W % 4 == 0, 16-byte aligned buffers. */
int skyemb_masked_patch_loss(const float *imgs, const float *pred, const float *mask, float *loss, void *dpred,
                             float *dpred32, int dtype, float *ws, int B, int C, int H, int W, int p, int extra,
                             float pixel_mean, float pixel_std, int norm_pix, int loss_l1, float dscale, void *stream);

/* SimMIM mode (utils/mim_vit.py:469, 480-493, 497-521): pixel-wise loss on the head GEMM's token rows
 * pred_tok fp32 [B*(L+extra), C*p*p] (column c*p*p + py*p + px == PixelShuffle(p) of the Conv1x1 output) with
 * weights w = pixel_mask where the target is not NaN:  loss = sum(w*l) / (sum(w) + 1e-5), optional per-patch
 * normalisation of the target.  Outputs: loss, dpred_tok (dtype, same layout; extra rows zero; may be NULL),
 * pred_img fp32 [B,C,H,W] (the reference's `pred`; may be NULL).  ws: 4*B*L + 4 floats.
 * pooled != 0 (attention-pooled models, utils/mim_vit.py:250): pred_tok / dpred_tok are [B, C*H*W], one row per image laid
 * out like the image (PixelShuffle(img_size) of the head's output); p stays the patch size of the normalisation; extra = 0.
 * dscale: as in skyemb_masked_patch_loss (dpred_tok = dscale * d loss / d pred_tok). */
int skyemb_simmim_pixel_loss(const float *imgs, const float *pred_tok, const float *pixel_mask, float *loss, void *dpred_tok,
                             int dtype, float *pred_img, float *ws, int B, int C, int H, int W, int p, int extra,
                             float pixel_mean, float pixel_std, int norm_pix, int loss_l1, int pooled, float dscale, void *stream);

/* dst[0..3] = {a, b, c, d} by a kernel launch (the values travel as kernel arguments): how the scalars of optimiser step t --
 * lr, 1 - beta1^t, 1 - beta2^t -- reach the device buffer `hyper` of skyemb_adamw / skyemb_adamw_desc in front of a replayed HIP
 * graph (torch.optim.AdamW keeps them on the host: utils/pretrain_fns.py:36-41). */
int skyemb_set_scalars(float *dst, float a, float b, float c, float d, void *stream);
/* ----------------------------------------------------------- optimiser ----
 * torch.optim.AdamW single-tensor update order (utils/mim_vit.py:126-129,
 * utils/pretrain_fns.py:36-41) over one flat fp32 parameter buffer:
 * elements [0, n_decay) use weight decay `wd`, the rest 0.  Step scalars {lr, 1-beta1^t, 1-beta2^t}
 * come from `hyper` (device fp32[4], for launches captured in a HIP graph) when non-NULL, else
 * from the lr/bc1/bc2 arguments.  Also refreshes the dtype shadow copy `p_lp` used by the GEMMs
 * (NULL to skip), scales gradients by grad_scale (DDP averaging, and the inverse of the backward pass's loss scale)
 * and optionally zeroes g.  `g` holds `grad_dtype` elements: SKYEMB_F32 (the flat gradient buffer the kernels write), or
 * SKYEMB_BF16 / SKYEMB_F16 (the copy a 16-bit gradient all-reduce worked on: half the xGMI bytes per step). */
int skyemb_adamw(float *p, void *g, float *m, float *v, void *p_lp, int dtype, int64_t n, int64_t n_decay,
                 const float *hyper, float lr, float bc1, float bc2, float beta1, float beta2, float eps, float wd,
                 float grad_scale, int zero_grad, int grad_dtype, void *stream);
int skyemb_cast(const float *src, void *dst, int dtype, int64_t n, void *stream);
/* Overflow guard of an optimiser step whose gradients carry a DYNAMIC loss scale (the downstream predictor in fp16: its loss is the
 * caller's code, so no scale can be planned ahead).  Additive to ABI version 111.
 * skyemb_grad_probe: one read of the `n` gradients at `g` (grad_dtype SKYEMB_F32 / SKYEMB_F16 / SKYEMB_BF16; n % 4 == 0, alignment
 * as skyemb_adamw: 16 bytes for fp32, 8 for the 16-bit formats).  `state`: two device words the caller zeroes once per step; launches
 * ACCUMULATE into them: state[0] becomes non-zero if any element is +-inf or NaN (exponent field all ones; +-0 and subnormals are
 * finite), state[1] is the bit pattern, as fp32, of the largest finite |g| (non-negative floats order like their unsigned bits).
 * skyemb_adamw_guarded: skyemb_adamw's kernel with `skip` = that state: skip[0] != 0 -> the launch writes NOTHING (p, m, v, p_lp
 * untouched, g not zeroed); skip[0] == 0 -> bit-identical to skyemb_adamw.  Stream order is the contract: every probe of a step
 * first, then its guarded launches, all on one stream. */
int skyemb_grad_probe(const void *g, int grad_dtype, int64_t n, uint32_t *state, void *stream);
int skyemb_adamw_guarded(float *p, void *g, float *m, float *v, void *p_lp, int dtype, int64_t n, int64_t n_decay,
                         const float *hyper, float lr, float bc1, float bc2, float beta1, float beta2, float eps, float wd,
                         float grad_scale, int zero_grad, int grad_dtype, const uint32_t *skip, void *stream);
/* Multi-tensor AdamW: one launch steps any set of disjoint segments of a flat buffer, each with the scalars of its parameter group
 * (the downstream predictor: layer-wise lr decay, linear probes, the head's own buffer).  Additive to ABI version 111.  Per segment
 * the result is bit-identical to skyemb_adamw over that segment with the group's lr, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, beta1,
 * beta2, eps, wd and n_decay = n (decayed != 0) or 0; nothing outside the segments is written and g is only read.
 * skyemb_adamw_segments_limits: three compile-time constants -- the most groups of one launch (they travel by value in the
 *   kernel arguments), the most elements of one work item, and the most workgroups of a launch.
 * skyemb_adamw_segments_plan: HOST function, no stream and no device: checks the segments (offsets and lengths in ELEMENTS of the
 *   flat buffer of buffer_n elements: multiples of 4, length > 0, inside the buffer, disjoint in any input order, group in
 *   [0, n_groups), n_groups in 1 .. max_groups; a refusal names the input index of the offending segment and the value) and writes
 *   the table the launch walks: (1) the segments sorted by offset, (2) neighbours that touch and share a group joined into one
 *   run, (3) every run cut from its start into work items of chunk_elems elements, the remainder (if any) last.  The table is
 *   n_work records of skyemb_adamw_work (16 bytes each, in that order); *need_bytes = 16 n_work.  table_host == NULL: only
 *   *need_bytes and *n_work are reported; a table of fewer than *need_bytes bytes is refused.
 * skyemb_adamw_segments: the launch.  p, g, m, v: the fp32 flat buffers; p_lp: the compute-dtype shadow (`dtype` SKYEMB_F32 /
 *   SKYEMB_BF16 / SKYEMB_F16; required); table_dev: a device copy of the planned table (16-byte aligned); groups: n_groups HOST
 *   structs, copied into the kernel arguments by the call (the caller may reuse them at once); grad_scale as skyemb_adamw's; skip:
 *   NULL, or the state of skyemb_grad_probe -- skip[0] != 0: the launch writes nothing, skip[0] == 0: the same bits as NULL.
 *   Workgroups of 256 threads stride over the work items, min(n_work, max_grid) of them. */
typedef struct skyemb_adamw_group { float lr, bc1, bc2, beta1, beta2, eps, wd; int32_t decayed; } skyemb_adamw_group;   /* 32 bytes */
typedef struct skyemb_adamw_segment { int64_t offset, n; int32_t group, reserved; } skyemb_adamw_segment;               /* 24 bytes */
typedef struct skyemb_adamw_work { int64_t offset; int32_t n, group; } skyemb_adamw_work;       /* 16 bytes: elements [offset, offset + n) */
int skyemb_adamw_segments_limits(int32_t *max_groups, int32_t *chunk_elems, int32_t *max_grid);
int skyemb_adamw_segments_plan(const skyemb_adamw_segment *segs, int n_segs, int n_groups, int64_t buffer_n, void *table_host,
                               int64_t table_bytes, int64_t *need_bytes, int32_t *n_work);
int skyemb_adamw_segments(float *p, const float *g, float *m, float *v, void *p_lp, int dtype, const void *table_dev, int32_t n_work,
                          const skyemb_adamw_group *groups, int n_groups, float grad_scale, const uint32_t *skip, void *stream);

/* ------------------------------------------------------------ input feeder -
 * utils/dataloaders.py:285-328 (H5Dataset.__getitem__): the reference opens the file and reads ONE cutout per python
 * call.  Here a minibatch of rows is gathered by native threads from the memory-mapped contiguous dataset into a (pinned)
 * staging buffer -- HOST function, no stream -- copied to the device once, then clipped at pixel_min / pixel_max (NaN
 * kept) and centre-cropped on the device (utils/dataloaders.py:293-300). */
int skyemb_gather_rows_host(const void *src, int64_t row_bytes, const int64_t *idx, int64_t n, int64_t src_rows, void *dst,
                            int nthreads);
/* Chunked HDF5 dataset -> contiguous row-major image (host threads; see hdf5_lite.py).  The reference's ETL writes its
 * train / validation files chunked (data_processing/2_create_h5_files.py:70-81: maxshape=(None, ...) + resize); they are
 * un-chunked once into a cache file and then served by the mmap fast path above.  file_base / file_bytes: the mapped file;
 * chunk i: byte address chunk_addr[i], element offsets chunk_off[i*rank ..], extent chunk_dims (edge chunks stored whole). */
int skyemb_h5_unchunk_host(const void *file_base, int64_t file_bytes, const int64_t *chunk_addr, const int64_t *chunk_off,
                           int64_t nchunks, int rank, const int64_t *chunk_dims, const int64_t *dset_dims, int elem_size, void *dst,
                           int nthreads);
/* The tiles of a FITS tile-compressed image (FITS 4.0 section 10; the reference reads such survey tiles through astropy / CFITSIO,
 * utils/dataloaders.py:418) -> integer pixels in the host's byte order, native threads over the tiles; see fits_lite.py, which
 * dequantises floating-point images afterwards.  HOST function.  codec 1 = RICE_1 (what fpack and astropy's CompImageHDU write by
 * default; pixels of `bytepix` = 1, 2 or 4 bytes coded in blocks of `blocksize` differences), 2 = PLIO_1 (integer masks), 3 =
 * HCOMPRESS_1 (both int32 pixels: bytepix = 4; an HCOMPRESS tile's stream carries its own dimensions, whose product must be npix[t];
 * for HCOMPRESS `blocksize` carries the SMOOTH flag of the image, 0 or 1).
 * Tile t: bytes [off[t], off[t] + len[t]) of `base` hold npix[t] pixels; they are written to dst + dst_off[t] * bytepix (dst holds
 * dst_pixels pixels). */
int skyemb_fits_decode_tiles_host(int codec, const void *base, int64_t base_bytes, const int64_t *off, const int64_t *len,
                                  const int64_t *npix, const int64_t *dst_off, int64_t ntiles, int bytepix, int blocksize, void *dst,
                                  int64_t dst_pixels, int nthreads);
/* Quantised floating-point tiles of such an image -> float32 pixels placed in the image (FITS 4.0 section 10.2): q * ZSCALE + ZZERO,
 * or (q - r + 0.5) * ZSCALE + ZZERO with the convention's subtractive dither (method 1 / 2; 2: q == -2147483646 is exactly 0; method 0:
 * none).  rand: the convention's 10 000 random numbers (fits_lite.dither_sequence), table_row[t]: the tile's 0-based row in the table.
 * Tile t: q + q_off[t], h[t] x w[t] pixels -> out[(y0[t] + y) * W + x0[t] + x]; has_blank[t] != 0: q == blank[t] -> NaN (both may be
 * NULL).  big_endian_out != 0: floats stored byte-swapped, the layout of an uncompressed FITS image.  HOST function. */
int skyemb_fits_dequantise_tiles_host(const int32_t *q, const int64_t *q_off, const int64_t *y0, const int64_t *x0, const int64_t *h,
                                      const int64_t *w, const int64_t *table_row, int64_t ntiles, const double *zscale, const double *zzero,
                                      const int32_t *blank, const uint8_t *has_blank, const float *rand, int method, int zdither0,
                                      float *out, int64_t H, int64_t W, int big_endian_out, int nthreads);
/* Survey-tile sampler: FitsDataset.__getitem__ (utils/dataloaders.py:589-654) cuts `cutouts_per_tile` windows out of a
 * multi-band FITS tile with a python loop (random_cutouts :449-476 / overlapping_cutouts :507-536) and clips them (:618-621).
 * Here the tile [C, H, W] sits in HBM as the files' own 4-byte words (big_endian[c] != 0: plane c still holds FITS
 * big-endian floats; a missing band is a plane of NaNs) and ONE launch writes out [n, C, S, S] = tile[:, h0[i]:+S, w0[i]:+S],
 * decoded and clipped at lo / hi (NaN kept).  h0 / w0: int32 device arrays, window origins (caller guarantees they fit). */
int skyemb_tile_cutouts(const void *tile, const int *big_endian, int C, int H, int W, const int *h0, const int *w0, int n, int S,
                        float lo, float hi, int use_lo, int use_hi, float *out, void *stream);
int skyemb_clip_crop(const float *src, float *dst, int64_t n_planes, int Hs, int Ws, int size, float lo, float hi,
                     int use_lo, int use_hi, void *stream);

/* Target augmentations of the similarity search (utils/dataloaders.py:14-106 get_augmentations as applied by
 * utils/eval_fns.py:88-108: per sample the original + A augmented copies): flips, RandomResizedCrop back to S x S
 * (crop + anti-aliased bilinear resize), brightness factor, additive noise, channels set to NaN -- one launch per batch.
 *   imgs [B, C, S, S] -> out [B * (1 + A), C, S, S], copy 0 of every sample unchanged
 *   params [B * (1 + A), 8] = {flip_h, flip_v, crop_top, crop_left, crop_h, crop_w, brightness, sigma} (drawn by the caller)
 *   nan_mask [B * (1 + A)]: bit c set -> channel c is NaN;  noise [B * (1 + A), C, S, S] standard normal draws or NULL */
int skyemb_augment(const float *imgs, float *out, const float *params, const int32_t *nan_mask, const float *noise, int B, int C,
                   int S, int A, void *stream);

/* ------------------------------------------------------ similarity search -
 * Addressing limits of the search calls below ("Addressing limits", has the table per kernel).  Every element and
 * byte offset into a bank (row * D, rows of 2 or 4 bytes) and every slot of a [Q, N] score matrix is formed in 64 bits: N * D
 * and Q * N are bounded by memory, not by these calls.  What is 32 bits wide:
 *   rows of a bank or shard as list entries    N < 2^31 per call of skyemb_cosine_topk and of the two prefiltered calls
 *                                              (refused); N * P < 2^31 token rows per call of the token / distance calls
 *                                              (refused), hence fewer than 2^31 images; skyemb_pack_select N < 2^31 (refused).
 *                                              Returned indices are int64: idx_offset + row, any idx_offset.
 *   stage 1 of the prefiltered calls           ceil(N / 2048) * ceil(Q / 256) * (D / 32) < 2^31 (work items and k-steps per
 *                                              launch; Q / 128 under SKYEMB_PREFILTER_LO=1) -- at D = 768 about Q * N < 4.6e13;
 *                                              refused, search the queries in batches.
 *   launch grids                               skyemb_weighted_norms[_lp]: N / 256 workgroups, N < 2^40; skyemb_bank16_prepare
 *                                              and skyemb_bank16_rowp_lp: N / 4, covered by N < 2^31; skyemb_standardise[_lp]
 *                                              and the score calls run grid-stride loops over 64-bit counters.
 * Tested on banks of 2 800 192 x 768 (fp16: past element 2^31 and byte 2^32; fp32: past byte 2^33), tests/test_large_bank_gpu.py;
 * banks past 2^32 elements (an fp32 bank of 17 GB) are correct by the same reading, not measured.
 *
 * utils/similarity.py:98-102: standardise bank rows in place or to `out`:
 * (x - mu) / (sigma + 1e-8). */
int skyemb_standardise(const float *x, const float *mu, const float *sigma, float *out, int64_t N, int D,
                       void *stream);
/* utils/similarity.py:166-167: weighted norms sqrt(sum_d w x^2) in the oracle's fixed fma order:
 * rows[n] (bank) ; for queries also tw = w * t (utils/similarity.py:163). w == NULL -> ones. */
int skyemb_weighted_norms(const float *x, const float *w, float *norms, float *xw_out, int64_t N, int D,
                          void *stream);
/* utils/similarity.py:149-172 + 18-35 fused: per-(query tile, bank chunk) exact partial top-k.
 *   tw [Q,D] (= w*t), qn [Q], bank [N,D], xn [N]  ->  part_s f32 / part_i i64 [Q, nchunks, k]
 * (nchunks = skyemb_cosine_topk_chunks(N, Q, D, k): bank chunks of the tiled kernel, or one list per
 * wavefront of the bank-streaming kernel used when Q <= 16).  The tiled kernel accepts any caller-chosen nchunks > 0: chunks
 * are ceil(ceil(N / nchunks) / tile) * tile rows long (tile = 256 bank rows; 128 under SKYEMB_TOPK_NW=4 for Q > 16, k <= 128),
 * so trailing chunks may be ragged or empty, and an empty chunk's list is a lone terminator.  The bank-streaming kernel
 * (Q <= 16, k <= 128, D % 64 == 0, D <= 1024, unless SKYEMB_TOPK_STREAM=0) does not: any count but the library's is refused.
 * thr0 (optional, [Q]): a pruning floor per query -- only rows scoring STRICTLY above it are kept.  Any value
 * below the true k-th best score is valid (e.g. nextafter(k-th best of a row sample, -inf)) and leaves
 * the result unchanged while removing most list insertions.
 * sorted by (score desc, index asc); idx = idx_offset + local row.  A list with fewer than k rows ends at its first
 * entry with a NEGATIVE index (score -inf); the slots behind that terminator are unspecified.  Then skyemb_topk_merge. */
int skyemb_cosine_topk_chunks(int64_t N, int Q, int D, int k);
int skyemb_cosine_topk(const float *tw, const float *qn, const float *bank, const float *xn, int Q, int64_t N,
                       int D, int k, float eps, int64_t idx_offset, int nchunks, const float *thr0, float *part_s,
                       int64_t *part_i, void *stream);
/* merge `nlists` sorted length-k lists per query (bank chunks, or per-rank results after the
 * RCCL all-gather): in [Q, nlists, k] -> out [Q, k].  `ws` (optional, Q ints) enables the gather + block-sort
 * path used for the many short lists of the bank-streaming kernel (per-query fallback to the tournament). */
/* out[q] = the k-th largest value of x[q, 0..S) minus one ulp (NaN ranks as -inf): the pruning floor a search derives from
 * the exact scores of a bank sample (host glue of the build; the reference has no counterpart -- it sorts everything). */
int skyemb_kth_largest_floor(const float *x, int Q, int S, int k, float *out, void *stream);
/* The same floor for Q <= 16 queries in two launches, without the [Q, S] score matrix: exact scores of the S sample rows reduced
 * on the fly to the maximum of every 16-row tile, then the k-th largest of the S / 16 maxima per query, one ulp lower (the score
 * of at least k different rows: a valid floor, and within a few ranks of the sample's own k-th best when S / 16 >> k).
 *   sample [S, D] rows of the bank, sample_norms [S] their weighted norms; ws: Q * ceil(S / 16) floats; floor_out [Q].
 * Needs D % 64 == 0, D <= 1024, k <= S / 16 <= 2048.  (Build-level helper like skyemb_kth_largest_floor: the reference sorts
 * every score, utils/similarity.py:18-35.) */
int skyemb_cosine_sample_floor(const float *tw, const float *qn, const float *sample, const float *sample_norms, int Q, int64_t S,
                               int D, int k, float eps, float *ws, float *floor_out, void *stream);
/* 1 when skyemb_cosine_sample_floor accepts (Q, S, D, k) in THIS process -- the shape limits above and the streaming kernels not
 * switched off (SKYEMB_TOPK_STREAM=0) -- else 0: the caller then uses skyemb_cosine_scores + skyemb_kth_largest_floor.  Base
 * addresses of tw and sample must additionally be 16-byte aligned (checked by the call itself). */
int skyemb_cosine_sample_floor_applicable(int Q, int64_t S, int D, int k);
int skyemb_topk_merge(const float *in_s, const int64_t *in_i, int Q, int nlists, int k, float *out_s,
                      int64_t *out_i, void *ws, void *stream);

/* Many-query exact top-k in two stages (Q >= 17): an fp16 matrix-core pass over a half-precision image of the bank with
 * a proven error bound keeps, per query, only the rows whose score could still reach its top-k; the survivors are
 * re-scored with the contract's fp32 fma chain.  Results are bit-identical to skyemb_cosine_topk + skyemb_topk_merge.
 * Replaces the same reference code as skyemb_cosine_topk (utils/similarity.py:18-35,149-172).
 *   skyemb_bank16_prepare   once per bank / weights: bank16 = fp16 rows scaled by 2^-e_i, rowp = 4 floats per row
 *                           {xn 2^-e, ||x'||_2, 2^-e, 0}; BOTH hold skyemb_bank16_rowp_rows(N) rows (N rounded up to whole
 *                           tiles: the search kernel reads whole tiles), i.e. skyemb_bank16_bytes(N, D) bytes of bank16
 *   skyemb_cosine_topk_prefiltered   whole pipeline on `stream`; out_s / out_i [Q, k] final lists; redo[q] != 0 marks a query
 *                           whose answer could not be certified (too many near-ties, candidate overflow, fewer than k
 *                           finite rows): the caller runs those through skyemb_cosine_topk.  thr0 as in skyemb_cosine_topk
 *                           (NULL: the first bank slice supplies the floor).  ws: skyemb_topk_prefilter_ws_bytes(Q, D, k).
 * The same search over a RESIDENT fp16 bank (bank16 [N, D] fp16, 16-byte aligned, D % 32 == 0): the bank is the fp32 bank its
 * elements widen to (xn: skyemb_weighted_norms_lp), both stages read it directly -- no fp32 copy, no second image -- and the
 * result is bit-identical to skyemb_cosine_topk_prefiltered on the widened bank.  bf16 rows are not representable in the
 * fp16 matrix operands: a resident bf16 bank takes the _resident calls further down, which multiply bf16 operands.
 *   skyemb_bank16_rowp_lp  once per bank / weights: rowp = {xn, ||x||_2 + the row's fp16-subnormal term, 1, 0} for
 *                           skyemb_bank16_rowp_rows(N) rows.  tail: one tile [256, D] fp16 (16-byte aligned) that receives a
 *                           zero-padded copy of the last N % 256 rows -- the search reads whole tiles and never reads past the
 *                           bank's N * D elements; may be NULL when N % 256 == 0.  Extra memory: 16 bytes per row + that tile.
 *   skyemb_cosine_topk_prefiltered_lp   skyemb_cosine_topk_prefiltered with the resident bank in place of bank + bank16 and
 *                           the tail tile of skyemb_bank16_rowp_lp; redo[q] != 0: the caller runs the query through
 *                           skyemb_cosine_token_topk_lp with one token per row.
 *   skyemb_topk_prefilter_eps_a   host only: the relative error bound eps_a of stage 1 (|dot^ - dot'| <= eps_a ||q'|| ||x'||) for
 *                           D features, one (lo = 0) or two (lo = 1) fp16 query passes, over the scaled image of an fp32 bank
 *                           (resident = 0) or a resident fp16 bank (resident = 1; then a row with nsub fp16-subnormal elements
 *                           adds ||q'|| sqrt(nsub) 2^-14).  Derivation: csrc/topk_prefilter.hip. */
int skyemb_topk_prefilter_applicable(int Q, int64_t N, int D, int k);
int64_t skyemb_topk_prefilter_ws_bytes(int Q, int D, int k);
/* Test and diagnostic hook (host only, nothing is launched): where the arrays of that workspace lie.  out[0 .. 13] are the byte offsets
 * of qh, ql, qbase, qpar, tau, bound, cnt, overflow, nsel, sel_i, cand_i, cand_d, wg_list, wg_count, out[14] = cap (slots of one
 * query's candidate list), out[15] = capw (entries of one workgroup's region of wg_list); n must be 16, anything else is refused.
 * With Qp = Q rounded up to 256, what the row search (every skyemb_cosine_topk_prefiltered* call above and below, not the token
 * search) leaves there when it returns:
 *   qh, ql [Qp, D] 16-bit   the scaled query images (the bank's operand format), rows Q .. Qp-1 zero
 *   qbase [Q] float4        {qn 2^-f, eps_a ||q'|| (1 + D 2^-22), 2^-f, qn}
 *   qpar [Qp] float4        the candidate test's parameters of the LAST threshold, rows Q .. Qp-1 NaN
 *   tau [Q] float           the last threshold published between phases (thr0, or -inf, when there was none)
 *   cnt [Q] int             entries appended to the query's list (may exceed cap: the excess was dropped and the query flagged)
 *   cand_i, cand_d [Q, cap] the list: row numbers and raw dot^ of stage 1, NOT compacted by the final selection
 *   overflow [Q] int        1: the query's scale left the bound's window, its list or a workgroup's region overflowed, or the staging
 *                           list of one of its work items did (then for every query of the item) -- redo[q] = 1
 *   sel_i [Q, 256], nsel [Q], bound [Q]   the rows re-scored exactly, their number, the largest upper bound left out
 *   wg_list, wg_count       staging of the last staged launch only: scratch. */
int skyemb_topk_prefilter_ws_layout(int Q, int D, int k, int64_t *out, int n);
int64_t skyemb_bank16_bytes(int64_t N, int D);
int64_t skyemb_bank16_rowp_rows(int64_t N);
int skyemb_bank16_prepare(const float *bank, const float *xn, int64_t N, int D, void *bank16, float *rowp, void *stream);
int skyemb_cosine_topk_prefiltered(const float *tw, const float *qn, int Q, const float *bank, const float *xn, const void *bank16,
                                   const float *rowp, int64_t N, int D, int k, float eps, int64_t idx_offset, const float *thr0,
                                   void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo, void *stream);
int skyemb_bank16_rowp_lp(const void *bank16, const float *xn, int64_t N, int D, float *rowp, void *tail, void *stream);
int skyemb_cosine_topk_prefiltered_lp(const float *tw, const float *qn, int Q, const void *bank16, const float *xn, const void *tail,
                                      const float *rowp, int64_t N, int D, int k, float eps, int64_t idx_offset, const float *thr0,
                                      void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo, void *stream);
double skyemb_topk_prefilter_eps_a(int D, int lo, int resident);
/* The resident search for either 16-bit format: `dtype` is SKYEMB_F16 or SKYEMB_BF16, as skyemb_weighted_norms_lp takes it (anything
 * else is refused).  With SKYEMB_F16 each call below IS its _lp counterpart above, same arguments, same bits.  With SKYEMB_BF16 the
 * bank is a resident bf16 bank [N, D] (16-byte aligned, D % 32 == 0; xn: skyemb_weighted_norms_lp): stage 1 multiplies the stored
 * rows and a bf16 split of the query on v_mfma_f32_16x16x32_bf16 -- same tiles, lists, phases and workspace --, stage 2 widens the
 * selected rows into the contract's fp32 chain: the result is bit-identical to skyemb_cosine_topk_prefiltered on the widened bank.
 *   skyemb_resident_rowp    skyemb_bank16_rowp_lp for the format given.  bf16: rowp = {xn, ||x||_2, 1, 0}; a row with an inf / NaN
 *                           element, a nonzero element outside [2^-60, 2^120), or a weighted norm xn that is not finite cannot be
 *                           bounded and takes the "keep for every query" constants {0, inf, 1, 0}: stage 2 decides it.  Same tail
 *                           tile (bf16 bits), same extra memory.
 *   skyemb_cosine_topk_prefiltered_resident / _resident_sel   skyemb_cosine_topk_prefiltered_lp / _lp_sel (the latter declared
 *                           below, with the selection calls) for the format given; redo[q] != 0: the caller runs the query
 *                           through skyemb_cosine_token_topk_lp / _sel with one token per row.  A bf16 search also flags every
 *                           query whose largest |tw| lies outside [2^-50, 2^79). Variant: SKYEMB_PREFILTER_LO=1 runs the two-pass
 *                           (hi + lo) query split, =0 the one-pass (hi only) one; unset, a bf16 bank runs hi only (measured
 *                           faster), an fp16 bank as ever.  The 2^31 work-item limit above holds with
 *                           the query tile of the variant in use (256 queries hi only, 128 hi + lo).
 *   skyemb_topk_prefilter_eps_a_resident   host only: eps_a of stage 1 over a resident bank of the format given; SKYEMB_F16:
 *                           skyemb_topk_prefilter_eps_a(D, lo, 1); SKYEMB_BF16: (lo ? 2^-18 : 2^-9) + 6.06 D 2^-24 + D 2^-38, no
 *                           additive row term.  Derivation: csrc/topk_prefilter.hip. */
int skyemb_resident_rowp(const void *bank16, int dtype, const float *xn, int64_t N, int D, float *rowp, void *tail, void *stream);
int skyemb_cosine_topk_prefiltered_resident(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                            const void *tail, const float *rowp, int64_t N, int D, int k, float eps,
                                            int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes, float *out_s,
                                            int64_t *out_i, int *redo, void *stream);
double skyemb_topk_prefilter_eps_a_resident(int D, int lo, int dtype);
/* The two searches above under a SELECTION of the bank's rows (words: skyemb_pack_select over the N rows; one selection for all
 * queries).  The result is that of the same search over the compacted bank of the selected rows -- scores bit for bit, order
 * (score desc, row asc) -- with every index mapped back to this bank; a deselected row contributes nothing, whatever it holds.
 * Fewer than k selected rows: the list ends in (-inf, -1) entries and the query is NOT flagged for that; a selected row that
 * scores -inf (a NaN in it) is then not returned, as in the token calls.
 *   skyemb_prefilter_select_prepare   once per selection, bank and version of rowp: rowp_sel [skyemb_bank16_rowp_rows(N), 4] = rowp
 *                           with the padding sentinel {0, NaN, 0, 0} in every deselected row (it fails the candidate test for every
 *                           query, also where rowp held the "keep for every query" constant of an unboundable row); tiles
 *                           (int32 [ceil(N / 256)]) = the LIVE tiles, ascending: the 256-row tiles with a selected row;
 *                           info (int32 [2], device) = {their number, 1 if the bank's last tile is one of them}.  Two short launches.
 *   skyemb_cosine_topk_prefiltered_sel / _lp_sel   the pipelines of skyemb_cosine_topk_prefiltered / _lp with rowp_sel, tiles and
 *                           the two values of info (read back by the caller: n_live >= 1, and at least one live WHOLE tile over a
 *                           resident bank) -- stage 1 walks the live tiles only, its phase schedule runs over their number, and the
 *                           tail tile of a resident bank is launched only when it is live.  No thr0.  Shape limits, workspace and
 *                           redo as for the unselected calls (on the whole bank's N); redo[q] != 0: the caller runs the query
 *                           through skyemb_cosine_token_topk_sel with one token per row, under the same words. */
int skyemb_prefilter_select_prepare(const uint32_t *words, int64_t N, const float *rowp, float *rowp_sel, int *tiles, int *info,
                                    void *stream);
int skyemb_cosine_topk_prefiltered_sel(const float *tw, const float *qn, int Q, const float *bank, const float *xn, const void *bank16,
                                       const float *rowp_sel, const int *tiles, int n_live, int last_live, int64_t N, int D, int k,
                                       float eps, int64_t idx_offset, void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i,
                                       int *redo, void *stream);
int skyemb_cosine_topk_prefiltered_lp_sel(const float *tw, const float *qn, int Q, const void *bank16, const float *xn,
                                          const void *tail, const float *rowp_sel, const int *tiles, int n_live, int last_live,
                                          int64_t N, int D, int k, float eps, int64_t idx_offset, void *ws, int64_t ws_bytes,
                                          float *out_s, int64_t *out_i, int *redo, void *stream);
int skyemb_cosine_topk_prefiltered_resident_sel(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                                const void *tail, const float *rowp_sel, const int *tiles, int n_live, int last_live,
                                                int64_t N, int D, int k, float eps, int64_t idx_offset, void *ws, int64_t ws_bytes,
                                                float *out_s, int64_t *out_i, int *redo, void *stream);
/* The two-stage many-query search over a resident 16-bit PATCH-TOKEN bank [N, P, D] (dtype SKYEMB_F16 or SKYEMB_BF16; 16-byte
 * aligned), per-image combine SKYEMB_COMBINE_MIN or SKYEMB_COMBINE_MAX: scores and image indices are bit for bit those of
 * skyemb_cosine_token_topk_lp + skyemb_topk_merge over the same bank -- order (score desc, image asc), images scoring -inf never
 * returned, tail (-inf, -1).  xn: skyemb_weighted_norms_lp of the N P rows; rowp / tail: skyemb_resident_rowp over the flat
 * [N P, D] rows.  Stage 1 is the row search's matrix-core pass; an image is a candidate when every (min) / some (max) row of it
 * passes the row test.  After every slice of tiles each candidate image is re-scored exactly (P token scores by the contract's
 * chain on the widened rows, then the combine) and merged into the query's running top-k, whose k-th best score is the next
 * slice's threshold: an exact lower bound at all times, so nothing is left to certify.  thr0 [Q] (or NULL): a floor, the k-th best
 * combined score over any sample of whole images.  redo[q] != 0: a candidate list or staging region was full, or the query is
 * outside what stage 1 bounds (a zero query; bf16: skyemb_cosine_topk_prefiltered_resident's window) -- the caller runs it through
 * skyemb_cosine_token_topk_lp.  Variant: SKYEMB_PREFILTER_LO as for the row search.
 *   skyemb_token_prefilter_applicable   the shape limits: P a divisor of 64, D % 32 == 0, 128 <= D <= 4096, k <= 256, k <= N,
 *                                       2048 <= N P < 2^31.  A refusal leaves them as the error text (skyemb_last_error).
 *   skyemb_token_prefilter_ws_bytes     bytes of `ws`: the row search's workspace (skyemb_topk_prefilter_ws_bytes(Q, D, k) bytes, the
 *                                       fields of skyemb_topk_prefilter_ws_layout; `nsel` [Q] holds the lengths of the running lists),
 *                                       then the running lists, uint64 [Q, 256] keys (score desc, image asc), padded to 256 bytes. */
int skyemb_token_prefilter_applicable(int Q, int64_t N, int P, int D, int k);
int64_t skyemb_token_prefilter_ws_bytes(int Q, int D, int k);
int skyemb_cosine_topk_tokens_prefiltered(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                          const void *tail, const float *rowp, int64_t N, int P, int D, int k, int combine, float eps,
                                          int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes, float *out_s,
                                          int64_t *out_i, int *redo, void *stream);
/* The search above under a SELECTION of the bank's images (words: skyemb_pack_select over the N images; one selection for all
 * queries).  The result is that of skyemb_cosine_token_topk_sel + skyemb_topk_merge under the same words, bit for bit: the search
 * over the compacted bank of the selected images, indices mapped back; a deselected image contributes nothing, whatever it holds.
 *   skyemb_token_prefilter_select_prepare   once per selection, bank and version of rowp (skyemb_resident_rowp over the flat N P
 *                           rows; P a divisor of 64): rowp_sel [skyemb_bank16_rowp_rows(N P), 4] = rowp with the padding sentinel
 *                           {0, NaN, 0, 0} in every row of a deselected image -- also where rowp held the "keep for every query"
 *                           constant of an unboundable row, which under max would make its image a candidate of every query --;
 *                           tiles (int32 [ceil(N P / 256)]) = the LIVE tiles, ascending: the 256-row tiles with a selected image;
 *                           cum (int32, same length) = for each live tile the number of selected images up to and including it;
 *                           info (int32 [2], device) = {the number of live tiles, 1 if the bank's last tile is one of them}.  Two
 *                           short launches.
 *   skyemb_cosine_topk_tokens_prefiltered_sel   the pipeline of skyemb_cosine_topk_tokens_prefiltered with rowp_sel, tiles and the
 *                           two values of info (read back by the caller: 1 <= n_live <= ceil(N P / 256), at least one live WHOLE
 *                           tile).  Stage 1 walks positions of the live list, the slice schedule runs over their number, the tail
 *                           tile is launched as the list's last position only when it is live.  direct_end (1 .. n_live): the
 *                           position at which the first, direct-append slice ends -- the caller takes it from cum (the first position
 *                           whose count reaches 96 k, at least n_live / 128).  thr0: a floor over a sample of SELECTED whole images.
 *                           Shape limits and workspace as for the unselected call (on the whole bank's N); redo[q] != 0: the caller
 *                           runs the query through skyemb_cosine_token_topk_sel under the same words. */
int skyemb_token_prefilter_select_prepare(const uint32_t *words, int64_t N, int P, const float *rowp, float *rowp_sel, int *tiles,
                                          int *cum, int *info, void *stream);
int skyemb_cosine_topk_tokens_prefiltered_sel(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                              const void *tail, const float *rowp_sel, const int *tiles, int n_live, int last_live,
                                              int direct_end, int64_t N, int P, int D, int k, int combine, float eps,
                                              int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes, float *out_s,
                                              int64_t *out_i, int *redo, void *stream);
/* Both searches above under the top-t combine (top_t, the reference's n_top_sims; skyemb_cosine_token_topk_top's rule): with
 * d[0] >= d[1] >= ... an image's token scores in descending order, -inf (a NaN score) last, SKYEMB_COMBINE_MIN scores d[top_t-1] and
 * SKYEMB_COMBINE_MAX d[0].  Scores and image indices are bit for bit those of skyemb_cosine_token_topk_top (_sel) +
 * skyemb_topk_merge over the same bank; an image with fewer than top_t scores above -inf scores -inf and is never returned.  The
 * arguments are those of the plain calls with top_t after combine.
 *   top_t == 0               IS the plain call: same checks, same kernels.
 *   max, any top_t           IS the plain max call (d[0] does not depend on top_t).
 *   min, top_t == P          IS the plain min call (d[P-1] is the min).
 *   min, 1 <= top_t < P      d[top_t-1] >= tau needs at least top_t rows of the image to pass the row test, so stage 1 makes an image
 *                            a candidate iff the COUNT of its passing rows is >= top_t (top_t == 1: some row passes, the fold of max),
 *                            and stage 2 sorts the image's P exact token scores by skyemb_cosine_token_topk_top's own network and
 *                            takes d[top_t-1].  top_t == 1 is not promised to equal the plain max call to the bit (a NaN score is
 *                            -inf in both, but the orders of fmaxf differ).
 *   mean, top_t != 0         refused with a text: the mean of the top_t best scores is not bounded by a count of passing rows; the
 *                            caller runs skyemb_cosine_token_topk_top.
 *   skyemb_token_topt_prefilter_applicable   skyemb_token_prefilter_applicable's shape limits, combine min or max, and
 *                            1 <= top_t <= min(P, 16).  A refusal leaves its reason as the error text (skyemb_last_error).
 * Workspace, thr0 (a floor of the k-th best score UNDER THE SAME top_t), redo and the variant switch as for the plain calls; a
 * flagged query is re-run through skyemb_cosine_token_topk_top (_sel) with the same top_t. */
int skyemb_token_topt_prefilter_applicable(int Q, int64_t N, int P, int D, int k, int combine, int top_t);
int skyemb_cosine_topk_tokens_prefiltered_top(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                              const void *tail, const float *rowp, int64_t N, int P, int D, int k, int combine,
                                              int top_t, float eps, int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes,
                                              float *out_s, int64_t *out_i, int *redo, void *stream);
int skyemb_cosine_topk_tokens_prefiltered_top_sel(const float *tw, const float *qn, int Q, const void *bank16, int dtype,
                                                  const float *xn, const void *tail, const float *rowp_sel, const int *tiles, int n_live,
                                                  int last_live, int direct_end, int64_t N, int P, int D, int k, int combine, int top_t,
                                                  float eps, int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes,
                                                  float *out_s, int64_t *out_i, int *redo, void *stream);
/* The same search with per-image combine SKYEMB_COMBINE_MEAN: scores and image indices are bit for bit those of
 * skyemb_cosine_token_topk_lp + skyemb_topk_merge under mean -- token scores by the contract's chain, (((0 + s_0) + s_1) + ...) /
 * float32(P) in token order, an image with a NaN token scores -inf and is never returned.  The mean of an image's token cosines is,
 * up to eps and rounding, one dot product with the image's pooled unit tokens m = (1/P) sum_p x_p / xn_p, so stage 1 is the ROW
 * search's matrix-core pass over a derived 16-bit image [N, D] of m (P times fewer rows than the bank) under a proven bound U >= mean
 * (csrc/topk_prefilter.hip, "combine 'mean'"); stage 2 re-scores every candidate image's P tokens from the bank after each slice, as
 * above.  No selection, no weights assumption: the bound uses only |tw . x| <= ||tw|| ||x||, so negative weights are served too.
 *   skyemb_token_mean_pool   one launch per bank and weights version (xn): pooled16 [N, D] in the bank's dtype = the 16-bit rounding
 *                           of m 2^-e (largest element in [2^13, 2^14); bf16: elements below 2^-40 stored as zero), formed in fp32 as
 *                           fl(fl(sum_p fl(x_p / xn_p)) / P), p ascending; rowp [skyemb_bank16_rowp_rows(N), 4] = {2^-e, ||m 2^-e||_2 +
 *                           (kappa / eps_m) c1 2^-e, c2 2^-e, 0} with c1 = mean_p ||x_p / xn_p||_2, c2 = mean_p ||x_p / xn_p||_2 / xn_p,
 *                           kappa = (1.02 D + 2.03 P + 4) 2^-24, all rounded up; rows past N: the padding sentinel {0, NaN, 0, 0}; tail
 *                           (NULL when N % 256 == 0): a zero-padded [256, D] copy of the last N % 256 pooled rows.  An image with an
 *                           inf / NaN element (bf16: a nonzero element outside [2^-60, 2^120)), a token norm outside [2^-40, 2^40] (zero
 *                           included), ||x_p / xn_p|| outside [2^-20, 2^20], 0 < max |m| < 2^-40 or a constant >= 2^60 cannot be bounded:
 *                           zeros and {0, inf, 1, 0}, a candidate of every query, decided by stage 2.  Extra memory: 2 D + 16 bytes per
 *                           image and the tail tile.
 *   skyemb_token_mean_prefilter_applicable   the shape limits, rows = images: P a divisor of 64, D % 32 == 0, 128 <= D <= 4096,
 *                           k <= 256, k <= N, N >= 2048, N P < 2^31.  A refusal leaves them as the error text (skyemb_last_error).
 *   skyemb_token_mean_prefilter_ws_bytes     bytes of `ws` (= skyemb_token_prefilter_ws_bytes: same layout).
 *   skyemb_token_mean_prefilter_eps_m        host only: eps_m of stage 1 over the pooled image; SKYEMB_F16: skyemb_topk_prefilter_eps_a(D,
 *                           lo, 0); SKYEMB_BF16: (lo ? 2^-9 : 2^-8) + 2^-17 + 6.06 D 2^-24 + D 2^-37.
 *   skyemb_cosine_topk_tokens_mean_prefiltered   the arguments of skyemb_cosine_topk_tokens_prefiltered in their order, with tail and
 *                           rowp those of skyemb_token_mean_pool, and pooled16 before the stream; combine must be SKYEMB_COMBINE_MEAN.
 *                           redo[q] != 0: a full list or staging region, or a query outside the bound's windows (a zero query, qn
 *                           outside [2^-20, 2^20], scale outside [2^-34, 2^34], eps negative or not finite) -- the caller runs it
 *                           through skyemb_cosine_token_topk_lp.  Variant: hi + lo unless SKYEMB_PREFILTER_LO=0. */
int skyemb_token_mean_pool(const void *bank16, int dtype, const float *xn, int64_t N, int P, int D, void *pooled16, float *rowp,
                           void *tail, void *stream);
int skyemb_token_mean_prefilter_applicable(int Q, int64_t N, int P, int D, int k);
int64_t skyemb_token_mean_prefilter_ws_bytes(int Q, int D, int k);
double skyemb_token_mean_prefilter_eps_m(int D, int lo, int dtype);
int skyemb_cosine_topk_tokens_mean_prefiltered(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                               const void *tail, const float *rowp, int64_t N, int P, int D, int k, int combine,
                                               float eps, int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes,
                                               float *out_s, int64_t *out_i, int *redo, const void *pooled16, void *stream);
/* Combine mean under a selection of images, by COMPACTION: stage 1 under mean never reads the bank, only the pooled image and its row
 * constants, so the selected images' rows of both are gathered once into a compact image [S, D] and stage 1 is the unselected pass
 * above over S rows, not N -- its work falls with the selection however the selected images are scattered over the bank.  A deselected
 * image appears nowhere: nothing it holds (NaN, inf, huge values) can matter.  Scores and image indices are bit for bit those of
 * skyemb_cosine_token_topk_sel (lp) + skyemb_topk_merge under mean and the same words.
 *   skyemb_token_mean_select_gather   one launch per selection, bank and weights version.  pooled16 [N, D] and rowp are those of
 *                           skyemb_token_mean_pool (dtype: the bank's); idx [S] the selected images, ASCENDING, 0 <= idx < N (an entry
 *                           outside is never followed: its row becomes padding).  Writes pooled_sel [S, D], row j = the bits of pooled
 *                           row idx[j]; rowp_sel [skyemb_bank16_rowp_rows(S), 4], row j = rowp row idx[j] bit for bit -- the {0, inf, 1, 0}
 *                           of an unboundable image included: it stays a candidate of every query, decided by stage 2 --, rows past S
 *                           the padding sentinel {0, NaN, 0, 0}; tail_sel (NULL when S % 256 == 0, then untouched): a zero-padded
 *                           [256, D] copy of the last S % 256 rows; map int32 [S] = idx.  pooled16, pooled_sel and tail_sel 16-byte
 *                           aligned.  Extra memory: 2 D + 20 bytes per selected image and the tail tile.
 *   skyemb_cosine_topk_tokens_mean_prefiltered_sel   the arguments of skyemb_cosine_topk_tokens_mean_prefiltered with tail / rowp /
 *                           pooled16 the COMPACTED ones, and S and map behind N.  N stays the bank's image count (the bank's bounds,
 *                           N P < 2^31).  It plans as the request {SKYEMB_PF_TOKENS_MEAN, N = S, sel = 0} of skyemb_prefilter_plan; stage
 *                           2 reads candidate c's tokens at image map[c] of the bank, and keys and out_i carry idx_offset + map[c] (map
 *                           ascending keeps the order (score desc, image asc)).  Refused before any launch, under this entry's name:
 *                           combine not mean, S < 2048, k > S, S > N, N P >= 2^31, a null map, pooled_sel or tail_sel not 16-byte
 *                           aligned, no tail_sel when S % 256 != 0, and whatever the plan refuses.  thr0: a floor of the k-th best
 *                           SELECTED score.  redo[q] != 0: as above -- the caller runs the query through skyemb_cosine_token_topk_sel. */
int skyemb_token_mean_select_gather(const void *pooled16, const float *rowp, const int64_t *idx, int64_t N, int64_t S, int D, int dtype,
                                    void *pooled_sel, float *rowp_sel, void *tail_sel, int *map, void *stream);
int skyemb_cosine_topk_tokens_mean_prefiltered_sel(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                                   const void *tail_sel, const float *rowp_sel, int64_t N, int64_t S, const int *map, int P,
                                                   int D, int k, int combine, float eps, int64_t idx_offset, const float *thr0, void *ws,
                                                   int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo, const void *pooled_sel,
                                                   void *stream);
/* Weighted MSE over a resident 16-bit token bank in the same two stages (additive to ABI version 111): the many-query form of
 * skyemb_distance_token_topk with metric SKYEMB_METRIC_MSE, combine min | max, shared weights c [D], no top_t, no selection (those: the
 * _top / _sel / _top_sel forms below).
 * Scores are the distance contract's below ("weighted MSE / MAE": 16 partial sums, four folds, one division), keys are
 * key = -dist; out_s [Q, k] holds KEYS (descending; the caller negates), out_i the images, order (key desc, image asc), missing
 * entries (-inf, -1): bit for bit skyemb_distance_token_topk + skyemb_topk_merge over the same bank.
 * In real arithmetic D dist = A_q + B_r - 2 (c o t_q) . x_r with A_q = sum c_d t_d^2, B_r = sum c_d x_d^2: one dot product with
 * tw = fl(c o t), which stage 1 multiplies on the 16-bit matrix cores under the resident bound above,
 *   |dot^ - 2^-f sum tw_d x_d| <= eps_mse ||q'|| nx,   eps_mse = eps_a (resident, dtype, hi | hi + lo) + 2^-22 (tw's own rounding),
 * so D dist_real >= A_dn + B_dn - 2 2^f (dot^ + eps_mse ||q'|| nx) with A_dn, B_dn the fp32 sums lowered by D 2^-22 relative (0 below
 * 2^-100).  With c >= 0 every term of the contract's sum is non-negative, so its n = 4 ceil(D / 64) + 9 roundings (the subtraction,
 * square, product, the additions into a partial, four folds, the division) each move it by at most 2^-24 relative: a token can
 * reach the distance threshold theta only if that lower bound is <= D theta (1 + gamma) + 2^-126, gamma = (4 ceil(D / 64) + 12) 2^-24.
 * Distance min: an image is a candidate when SOME token can (key-space max); distance max: when EVERY token can (key-space min).
 * Every candidate image's P tokens are re-scored by the contract's chain after each slice, which makes the threshold exact.
 *   skyemb_token_mse_prefilter_applicable   1 / 0 (+ text): the shape rule of skyemb_token_prefilter_applicable
 *   skyemb_token_mse_prefilter_eps / _gamma eps_mse (lo: 0 hi only, 1 hi + lo) and gamma, before the (1 + 1e-6) raise: host arithmetic
 *   skyemb_token_mse_rowp   one launch per (bank, c): rowp [skyemb_bank16_rowp_rows(R), 4] over the R = N P flat rows, row i =
 *                           {B_dn, nx, 1, 0}: B_dn the lower bound of B_r under this c, nx the norm slot of skyemb_resident_rowp
 *                           (rounded up; fp16: + sqrt(nsub) 2^-14 / eps_mse; bf16: rule (R)); an unboundable row -- an inf / NaN
 *                           element, a bf16 element outside [2^-60, 2^120), B^ negative, not finite or >= 2^36 (fp16) / 2^96
 *                           (bf16) -- holds {0, inf, 1, 0}: a candidate of every query; padding rows the sentinel {0, NaN, 0, 0};
 *                           tail (NULL when R % 256 == 0): the zero-padded tile [256, D] of the last R % 256 rows.
 *   skyemb_distance_topk_tokens_prefiltered   c [D], t [Q, D] the raw queries (both 16-byte aligned), rowp / tail those of
 *                           skyemb_token_mse_rowp for this c, combine the DISTANCE combine (min | max; anything else is
 *                           refused); thr0 NULL or [Q] floors of the k-th best KEY; ws: skyemb_token_prefilter_ws_bytes(Q, D, k).
 *                           It plans as the request {SKYEMB_PF_TOKENS, combine = the key-space code (min -> max, max -> min)} of
 *                           skyemb_prefilter_plan for the variant, the slices and the stage-1 instances.  Three launch values are NOT
 *                           the plan's: stage 1's eps is eps_mse (skyemb_token_mse_prefilter_eps), not eps_a / eps_a_f32; the token
 *                           re-score takes lds_close + 4 D bytes of dynamic LDS (c [D] beside t) and its limit is raised to
 *                           lds_close_limit + 16384; gfac (-1 in the plan) carries gamma.  redo[q] != 0: a full candidate list, tw = 0, a scale 2^-f outside (0, 2^90)
 *                           (fp16) / (2^-100, 2^30) (bf16), A_q not finite, a test parameter outside fp32's range, or any c_d
 *                           negative, NaN or above 2^10 (then every query): the caller runs the query through
 *                           skyemb_distance_token_topk. */
int skyemb_token_mse_prefilter_applicable(int Q, int64_t N, int P, int D, int k);
double skyemb_token_mse_prefilter_eps(int D, int lo, int dtype);
double skyemb_token_mse_prefilter_gamma(int D);
int skyemb_token_mse_rowp(const void *bank16, int dtype, const float *c, int64_t R, int D, float *rowp, void *tail, void *stream);
int skyemb_distance_topk_tokens_prefiltered(const float *c, const float *t, int Q, const void *bank16, int dtype, const float *rowp,
                                            const void *tail, int64_t N, int P, int D, int k, int combine, int64_t idx_offset,
                                            const float *thr0, void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo,
                                            void *stream);
/* The weighted-MSE search above under top_t and under a SELECTION of the bank's images (additive to ABI version 111): the many-query
 * forms of skyemb_distance_token_topk with top_t and with selection words, bit for bit.  The argument lists are those of the cosine
 * _top / _sel / _top_sel entries with c, t in place of tw, qn, xn and eps (rowp before tail, as in the plain MSE call).
 * Key space (key = -distance), with a[0] <= a[1] <= ... the token distances of an image, a NaN distance ranking as +inf (key -inf, last):
 *   top_t == 0               IS the plain call: same checks, same kernels.
 *   min, any top_t           IS the plain min call (a[0] does not depend on top_t).
 *   max, top_t == P          IS the plain max call (a[P-1] is the max).
 *   max, 1 <= top_t < P      a[top_t-1] is the top_t-th LARGEST key: key-space 'min' under top_t.  It reaches the threshold only when at
 *                            least top_t rows of the image pass the MSE row test, so stage 1 runs the counting fold (top_t == 1: some
 *                            row passes), and stage 2 computes the P token keys by the distance contract's chain, sorts them by
 *                            skyemb_distance_token_topk's own network and takes the top_t-th.  An image with fewer than top_t finite
 *                            token distances scores +inf (key -inf) and is never returned.
 *   mean                     refused with a text: the grouped search serves it.
 * They plan as the requests {SKYEMB_PF_TOKENS, key-space combine, top_t (0 under distance min), sel} of skyemb_prefilter_plan -- the
 * plans of the cosine _top / _sel entries of the same shape -- with the three launch values of the plain MSE call (eps_mse, lds_close +
 * 4 D, gamma in gfac).
 * Selection: skyemb_token_prefilter_select_prepare is applied to the rowp of skyemb_token_mse_rowp as it stands.  Its kernel writes
 * the padding sentinel {0, NaN, 0, 0} into every row of a deselected image whatever rowp held there, the unboundable {0, inf, 1, 0}
 * included; and the sentinel fails the MSE row test under both folds: t = dot^ - a 0 + c NaN + g 0 is NaN, no pass bit is set, so the row
 * neither opens the OR fold nor counts.  A selected image keeps its constants, an unboundable row of it stays a candidate of every
 * query and is decided by stage 2, which re-scores candidates exactly as the unselected call does (they are images of the whole bank).
 * n_live, last_live, direct_end, tiles: as for skyemb_cosine_topk_tokens_prefiltered_sel (1 <= n_live <= ceil(N P / 256), at least one
 * live WHOLE tile, 1 <= direct_end <= n_live); thr0: a floor of the k-th best key UNDER THE SAME top_t over a sample of SELECTED images.
 * Refusals (before any launch, under the entry's name): mean, top_t outside 0 .. min(P, 16), the shape rule, the selection's limits.
 * redo[q] as for the plain MSE call: the caller re-runs the query through skyemb_distance_token_topk with the same top_t and words.
 *   skyemb_token_mse_topt_prefilter_applicable   skyemb_token_mse_prefilter_applicable's shape rule, combine min or max and
 *                            1 <= top_t <= min(P, 16); a refusal leaves its reason as the error text. */
int skyemb_token_mse_topt_prefilter_applicable(int Q, int64_t N, int P, int D, int k, int combine, int top_t);
int skyemb_distance_topk_tokens_prefiltered_top(const float *c, const float *t, int Q, const void *bank16, int dtype, const float *rowp,
                                                const void *tail, int64_t N, int P, int D, int k, int combine, int top_t,
                                                int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes, float *out_s,
                                                int64_t *out_i, int *redo, void *stream);
int skyemb_distance_topk_tokens_prefiltered_sel(const float *c, const float *t, int Q, const void *bank16, int dtype, const float *rowp_sel,
                                                const void *tail, const int *tiles, int n_live, int last_live, int direct_end, int64_t N,
                                                int P, int D, int k, int combine, int64_t idx_offset, const float *thr0, void *ws,
                                                int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo, void *stream);
int skyemb_distance_topk_tokens_prefiltered_top_sel(const float *c, const float *t, int Q, const void *bank16, int dtype,
                                                    const float *rowp_sel, const void *tail, const int *tiles, int n_live, int last_live,
                                                    int direct_end, int64_t N, int P, int D, int k, int combine, int top_t,
                                                    int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes, float *out_s,
                                                    int64_t *out_i, int *redo, void *stream);
/* The weighted-MSE search with PER-QUERY weights c [Q, D] in the same two stages (additive to ABI version 111): the many-query form of
 * skyemb_distance_token_topk_pq with metric SKYEMB_METRIC_MSE, combine min | max, no top_t, no selection; bit for bit that call +
 * skyemb_topk_merge.  B_r = sum c_qd x_d^2 depends on the query, so it joins the dot product: with c_q >= 0, in real arithmetic
 *   D dist = A_q - 2 u_q . y_x,   u_q = [c_q o t_q ; -c_q / 2],   y_x = [x ; x o x],   A_q = sum c_qd t_qd^2   (2 D numbers each).
 * Stage 1 runs the same instances over a second resident 16-bit image of the bank, rows [x ; r16(x o x)] of length 2 D (r16: one
 * round-to-nearest-even of the exact fp32 square; 4 N P D bytes beside the bank's 2 N P D, independent of the weights), under
 *   |dot^ - 2^-f u_q . y_x| <= eps_pq ||u'|| ny,   eps_pq = eps_a (2 D; resident, dtype, hi | hi + lo) + rho (1 + rho) + 2^-22 (+ kappa),
 * rho = 2^-11 (fp16) / 2^-8 (bf16), the format's unit roundoff, for the one rounding of each square; bf16 only: kappa = 2^-9 (hi only) /
 * 2^-16 - 2^-18 (hi + lo) prices the query split at the same unit roundoff (derivation: csrc/topk_prefilter.hip), so
 * D dist_real >= A_dn - 2 2^f (dot^ + eps_pq ||u'|| ny); the threshold test, gamma (at the real D) and stage 2 are the plain call's,
 * stage 2 reading row q of c.  Cosine with per-query weights is NOT served this way: its row norm sum w_qd x_d^2 sits under a square
 * root in the denominator, so the candidate test is no single linear instruction.
 *   skyemb_token_mse_pq_prefilter_applicable   1 / 0 (+ text): D % 32 == 0, 128 <= D <= 2048, skyemb_token_prefilter_applicable's
 *                           shape rule on (Q, N, P, 2 D, k), fewer than 2^31 rows after padding to whole 256-row tiles
 *   skyemb_token_mse_pq_prefilter_eps   eps_pq (lo: 0 hi only, 1 hi + lo), before the (1 + 1e-6) raise: host arithmetic
 *   skyemb_token_mse_pq_image   one launch per bank: image [skyemb_bank16_rowp_rows(R), 2 D] in the bank's dtype and rowp [the same rows, 4]
 *                           over the R = N P flat rows; row i = {0, ny, 1, 0}, ny >= ||[x ; r16(x o x)]||_2 rounded up (fp16: + (sqrt(nsub)
 *                           2^-14 + sqrt(nsq) 2^-25) / eps_pq (hi + lo): nsub the fp16-subnormal elements of both halves, nsq the
 *                           squares below 2^-14).  An unboundable row -- an inf / NaN element, fp16: an |x| >= 2^8, bf16: a nonzero
 *                           element whose stored square is outside [2^-60, 2^120), ny not finite -- holds {0, inf, 1, 0} and a ZERO
 *                           image row: a candidate of every query.  Padding rows: zeros and the sentinel {0, NaN, 0, 0}; no tail tile.
 *   skyemb_distance_topk_tokens_prefiltered_pq   c [Q, D], t [Q, D], image and rowp those of skyemb_token_mse_pq_image for this bank
 *                           (all 16-byte aligned); combine, thr0, out_s (KEYS), out_i, redo as for the plain call; ws:
 *                           skyemb_token_prefilter_ws_bytes(Q, 2 D, k).  It plans as the request {SKYEMB_PF_TOKENS, the bank's format,
 *                           D' = 2 D, N' = the padded rows / P, the key-space combine} of skyemb_prefilter_plan; stage 1's eps is eps_pq,
 *                           gfac carries gamma (D), the token re-score takes lds_close as planned (t [D] and c_q [D] fill the plan's
 *                           2 D floats) and reads the BANK at D.  redo[q] != 0 as for the plain call, except that a negative, NaN or
 *                           above-2^10 weight flags only the queries whose own row holds it; c_q o t_q = 0 flags the query too.  The
 *                           caller re-runs flagged queries through skyemb_distance_token_topk_pq. */
int skyemb_token_mse_pq_prefilter_applicable(int Q, int64_t N, int P, int D, int k);
double skyemb_token_mse_pq_prefilter_eps(int D, int lo, int dtype);
int skyemb_token_mse_pq_image(const void *bank16, int dtype, int64_t R, int D, void *image, float *rowp, void *stream);
int skyemb_distance_topk_tokens_prefiltered_pq(const float *c, const float *t, int Q, const void *bank16, int dtype, const void *image,
                                               const float *rowp, int64_t N, int P, int D, int k, int combine, int64_t idx_offset,
                                               const float *thr0, void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo,
                                               void *stream);
/* The weighted-MSE search under combine MEAN in the same two stages (additive to ABI version 111): the many-query form of
 * skyemb_distance_token_topk with metric SKYEMB_METRIC_MSE, combine SKYEMB_COMBINE_MEAN, shared weights c [D], no top_t, no selection; bit
 * for bit that call + skyemb_topk_merge.  The mean is linear in the tokens: per image i and query q, in real arithmetic (P a power of two),
 *   D mean_p dist(q, x_p) = A_q + Bbar_i - 2 (c o t_q) . m_i,   m_i = (1/P) sum_p x_p,   Bbar_i = (1/P) sum_p sum_d c_d x_pd^2,
 * the operand shape of skyemb_distance_topk_tokens_prefiltered with a row that is an image: stage 1 is the ROW pass over a pooled 16-bit
 * image [N, D] (P times fewer rows than the bank), stage 2 re-scores every candidate image's P tokens by the contract's chain and folds
 * the keys -dist_p in token order, (((0 + s_0) + s_1) + ...) / float(P) -- the negation of the contract's mean bit for bit; a sum that is
 * not a number is key -inf, never returned.  Bound (derivation: csrc/topk_prefilter.hip): the pooled row is m' = m_fl 2^-e, m_fl the fp32
 * sum of the widened tokens in token order scaled exactly by 1 / P, e the power of two that puts its largest element in [2^13, 2^14),
 * rounded once to the bank's dtype (bf16: elements below 2^-40 stored as zero), and
 *   |dot^ - 2^-(f + e) (c o t) . m| <= eps ||q'|| R1,   eps = eps_m (skyemb_token_mean_prefilter_eps_m) + 2^-22,
 *   R1 = ||m'|| + (kappa / eps_m(hi + lo)) c1 2^-e (raised),   kappa = 1.01 P 2^-24,   c1 = mean_p ||x_p||_2   (the pooling's P - 1 additions),
 * so D mean_real >= A_dn + Bbar_dn - 2 2^(f + e) (dot^ + eps ||q'|| R1) =: L, and an image can reach the distance threshold theta only if
 * L <= D theta (1 + gamma) + 2^-126, gamma = skyemb_token_mse_prefilter_gamma(D) + P 2^-24 (the mean's own P - 1 rounded additions).
 *   skyemb_token_mse_mean_prefilter_applicable   1 / 0 (+ text): skyemb_token_mean_prefilter_applicable's shape rule (N >= 2048 images)
 *   skyemb_token_mse_mean_prefilter_eps / _gamma  eps (lo: 0 hi only, 1 hi + lo; before the (1 + 1e-6) raise) and gamma: host arithmetic
 *   skyemb_token_mse_mean_pool   one pass over the bank, independent of the weights: pooled16 [N, D] in the bank's dtype, its zero-padded tail
 *                           tile [256, D] (needed when N % 256 != 0) and paux f32 [skyemb_bank16_rowp_rows(N), 2] = {R1, 2^-e} per image.
 *                           An image the bank alone makes unboundable -- an inf / NaN element, bf16: a nonzero element outside
 *                           [2^-60, 2^120), R1 or 2^-e at or above 2^60 -- holds a ZERO pooled row and {inf, 1}; padding rows {NaN, 0}.
 *                           An image whose tokens cancel to a zero pooled row is an ordinary image (e = 0).
 *   skyemb_token_mse_mean_rowp   one more pass over the bank per weight vector c [D] (16-byte aligned): rowp f32 [the same rows, 4] =
 *                           {Bbar_dn 2^-e, R1, 2^-e, 0}, Bbar_dn = Bbar^ (1 - (n_B + 8) 2^-23) <= Bbar, n_B = 8 P ceil(D / 512) the fused multiply-adds of one lane's chain (0 below 2^-100; a product that
 *                           underflows is lowered to 0).  Unboundable -- {0, inf, 1, 0}, a candidate of every query -- when paux says so,
 *                           when Bbar^ is not a number in [0, 2^36) (fp16) / [0, 2^96) (bf16), or when Bbar_dn 2^-e leaves that window.
 *                           Padding rows: the sentinel {0, NaN, 0, 0}.
 *   skyemb_distance_topk_tokens_mean_prefiltered   c [D], t [Q, D] (16-byte aligned); pooled16 and tail those of _pool, rowp that of _rowp
 *                           under the same c; thr0, out_s (KEYS = -distance), out_i, redo as for skyemb_distance_topk_tokens_prefiltered;
 *                           ws: skyemb_token_mean_prefilter_ws_bytes(Q, D, k).  It plans as the request {SKYEMB_PF_TOKENS_MEAN, the
 *                           bank's format, D, combine mean} of skyemb_prefilter_plan (hi + lo unless SKYEMB_PREFILTER_LO=0); stage 1's eps
 *                           is the eps above, the re-score's gfac carries gamma.  redo[q] != 0: a full candidate list, a zero or
 *                           out-of-range query, a weight that is negative, NaN or above 2^10 (then every query).  The caller re-runs
 *                           flagged queries through skyemb_distance_token_topk. */
int skyemb_token_mse_mean_prefilter_applicable(int Q, int64_t N, int P, int D, int k);
double skyemb_token_mse_mean_prefilter_eps(int D, int lo, int dtype);
double skyemb_token_mse_mean_prefilter_gamma(int D, int P);
int skyemb_token_mse_mean_pool(const void *bank16, int dtype, int64_t N, int P, int D, void *pooled16, float *paux, void *tail, void *stream);
int skyemb_token_mse_mean_rowp(const void *bank16, int dtype, const float *c, const float *paux, int64_t N, int P, int D, float *rowp,
                               void *stream);
int skyemb_distance_topk_tokens_mean_prefiltered(const float *c, const float *t, int Q, const void *bank16, int dtype, const void *pooled16,
                                                 const void *tail, const float *rowp, int64_t N, int P, int D, int k, int64_t idx_offset,
                                                 const float *thr0, void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo,
                                                 void *stream);
/* Read-only query of the launch plan of every two-stage search above (csrc/prefilter_plan.h): what the entry point serving `req`
 * decides on the host -- variant, slices, kernel instances, LDS bytes -- and then launches.  Host arithmetic only, touches no device.
 * Returns 0 and fills *out, or 1 with the text (skyemb_last_error) and under the name of the entry point that would refuse the
 * same request; pointer arguments (null, alignment, tail tile, workspace size) are the entry points' own business.
 *   kind        SKYEMB_PF_ROWS: skyemb_cosine_topk_prefiltered (_lp, _resident, _sel); SKYEMB_PF_TOKENS: skyemb_cosine_topk_tokens_
 *               prefiltered (_top, _sel); SKYEMB_PF_TOKENS_MEAN: skyemb_cosine_topk_tokens_mean_prefiltered
 *   bank        SKYEMB_PF_BANK_F32 (rows only: an fp32 bank and its fp16 image), _F16, _BF16 (a resident 16-bit bank)
 *   N           rows of the bank; images on the token routes.  P, combine, top_t: token routes (P = 1, top_t = 0 otherwise)
 *   sel         the search runs under a selection: n_live, last_live (the prepare call's info), direct_sel (tokens: direct_end)
 *   lo          0 / 1: SKYEMB_PREFILTER_LO=0 / =1; SKYEMB_PF_LO_UNSET; -1: what the process's environment says now
 * The plan: slices in launch order; a slice is one stage-1 launch over positions [t0, t1) -- MODE mode of prefilter_kernel<mode,
 * use_lo, sel, bf, tok, cnt> --, bucket_kernel when `bucket`, the tail tile's launch when `tail` (MODE 1 over position tail_pos, with
 * the SEL instance when tail_sel) and select_kernel (rows) / the token re-score, told `final`. */
#define SKYEMB_PF_ROWS 0
#define SKYEMB_PF_TOKENS 1
#define SKYEMB_PF_TOKENS_MEAN 2
#define SKYEMB_PF_BANK_F32 0
#define SKYEMB_PF_BANK_F16 1
#define SKYEMB_PF_BANK_BF16 2
#define SKYEMB_PF_LO_UNSET 2
#define SKYEMB_PF_MAX_SLICES 6
typedef struct {
    int32_t kind, bank;
    int32_t Q, P, D, k;
    int64_t N;
    int32_t combine, top_t;
    int32_t has_thr0;
    int32_t sel, n_live, last_live, direct_sel;
    int32_t lo;
    float eps;
} skyemb_prefilter_request_t;
typedef struct {
    int32_t mode, t0, t1;            /* stage 1 */
    int32_t bucket;
    int32_t tail, tail_sel, tail_pos;
    int32_t final;
} skyemb_prefilter_slice_t;
typedef struct {
    int32_t use_lo, cap;
    int32_t T, T_tail, has_tail;     /* positions the slices walk; the tile the tail stands for; a tail launch happens */
    int32_t first, first_rows;       /* tiles / list slots of the take-all slice (0 on the token routes) */
    int32_t direct_end, ends[SKYEMB_PF_MAX_SLICES];
    int32_t sel, bf, tok, cnt;       /* the stage-1 instance family */
    int32_t tok_word, lgp, fold, top_t;   /* prefilter_kernel's `tok`; log2 P; 0 min 1 max 2 mean; top_t normalised (max, top_t == P: 0) */
    int32_t q_padded;
    int32_t lds_stage1, lds_close, lds_rescore;          /* dynamic LDS bytes: stage 1; select_kernel / token re-score; final re-score */
    int32_t lds_stage1_limit, lds_close_limit;           /* what the instances' dynamic-LDS limit is raised to */
    float eps_a_f32, gfac;           /* the float handed to query16_kernel; mean: eps / eps_m raised (else -1) */
    double eps_a;                    /* before the (1 + 1e-6) factor */
    int64_t rows;                    /* rows stage 1 walks: N, N P on the min / max token route */
    int32_t n_slices;
    skyemb_prefilter_slice_t slice[SKYEMB_PF_MAX_SLICES];
} skyemb_prefilter_plan_t;
int skyemb_prefilter_plan(const skyemb_prefilter_request_t *req, skyemb_prefilter_plan_t *out);
/* Attention pooling with one learned query (timm AttentionPoolLatent as built at utils/mim_vit.py:246-249 and applied at
 * :426-427; SimMIM models with attn_pool = True).  q [D] = Wq latent + bq is sample-independent (skyemb_attnpool_q);
 * kv [B, N, 2, H, hd] is the kv projection's output (compute dtype); fwd: out [B, D] (compute dtype) = softmax(scale q.k) v
 * per head, prob [B, H, N] fp32 saved for backward; bwd: dkv [B, N, 2, H, hd], dq_part [B, D] fp32 (per-sample dq);
 * skyemb_attnpool_q_bwd sums dq_part over the batch -> dWq = dq latent^T, dbq = dq, dlatent = Wq^T dq (ws: D floats). */
int skyemb_attnpool_q(const float *latent, const float *Wq, const float *bq, float *q, int D, void *stream);
int skyemb_attnpool_fwd(const float *q, const void *kv, int dtype, void *out, float *prob, int B, int N, int H, int hd, void *stream);
int skyemb_attnpool_bwd(const float *q, const void *kv, int dtype, const void *dout, const float *prob, void *dkv, float *dq_part,
                        int B, int N, int H, int hd, void *stream);
/* the same two calls for 1 <= N <= SKYEMB_MHA_MAX_N tokens (the plain ones take N <= 256): past 256 the token loop runs in chunks,
 * the softmax statistics passing through prob */
int skyemb_attnpool_fwd_long(const float *q, const void *kv, int dtype, void *out, float *prob, int B, int N, int H, int hd,
                             void *stream);
int skyemb_attnpool_bwd_long(const float *q, const void *kv, int dtype, const void *dout, const float *prob, void *dkv,
                             float *dq_part, int B, int N, int H, int hd, void *stream);
int skyemb_attnpool_q_bwd(const float *dq_part, int B, const float *latent, const float *Wq, float *dWq, float *dbq, float *dlatent,
                          float *ws, int D, void *stream);
/* plain score matrix for the reference-shaped path with P>1 patches per sample
 * (utils/similarity.py:262-267 combine over patches happens on these): scores [Q, N]. */
int skyemb_cosine_scores(const float *tw, const float *qn, const float *bank, const float *xn, int Q, int64_t N,
                         int D, float eps, float *scores, void *stream);
/* Patch-token bank search (utils/similarity.py:214-268 with max_pool = False: every patch token of a test image is scored,
 * then the P token scores are combined per image): the bank is [N, P, D] fp32, viewed as N * P rows with weighted norms
 * xn [N * P] (skyemb_weighted_norms); tw / qn as for skyemb_cosine_topk.  One pass over the bank: token score = the contract's
 * fma chain + the same last step as skyemb_cosine_topk (NaN -> -inf), combined in registers, in fp32:
 *   MIN / MAX  exact;  MEAN  (((0 + s[0]) + s[1]) + ... + s[P-1]) / (float)P -- token order, one IEEE division, independent of
 *   launch geometry and of Q.  A -inf token gives -inf for MIN and MEAN and is ignored by MAX.
 * Shapes: Q <= 16, D % 64 == 0, D <= 1024, 1 <= P <= 4096 with 16 % P == 0 or P % 16 == 0, N * P < 2^31 and, for the lists,
 * 1 <= k <= 512 with 64 D + 32 Q k <= 163840 (A image + four waves' lists in LDS); skyemb_cosine_token_applicable says so without
 * touching the device (0 leaves the limits and the refused shape as skyemb_last_error), everything else returns 1 before any launch.  bank and tw 16-byte aligned.
 *   skyemb_cosine_token_scores   scores [Q, N]: the combined score of every image.
 *   skyemb_cosine_token_topk     part_s f32 / part_i i64 [Q, nlists, k] (nlists = skyemb_cosine_token_topk_chunks(N, P, Q, D, k)):
 *                                one sorted list per wavefront, ONE insertion attempt per image, (score desc, image asc),
 *                                idx = idx_offset + image, thr0 and the (-inf, -1) terminator as in skyemb_cosine_topk; images
 *                                whose combined score is -inf are never listed.  Then skyemb_topk_merge. */
#define SKYEMB_COMBINE_MIN 0
#define SKYEMB_COMBINE_MEAN 1
#define SKYEMB_COMBINE_MAX 2
int skyemb_cosine_token_applicable(int Q, int P, int D, int k);
int skyemb_cosine_token_topk_chunks(int64_t N, int P, int Q, int D, int k);
int skyemb_cosine_token_scores(const float *tw, const float *qn, const float *bank, const float *xn, int Q, int64_t N, int P, int D,
                               int combine, float eps, float *scores, void *stream);
int skyemb_cosine_token_topk(const float *tw, const float *qn, const float *bank, const float *xn, int Q, int64_t N, int P, int D,
                             int k, int combine, float eps, int64_t idx_offset, int nlists, const float *thr0, float *part_s,
                             int64_t *part_i, void *stream);
/* Half-precision resident banks (additive to ABI version 111: nothing above changes).  A 16-bit bank IS the fp32 bank obtained by
 * widening every stored element exactly (fp16 subnormals included, fp16 inf stays inf): after the load the `_lp` calls run the
 * arithmetic of their fp32 namesakes -- the same fma chain, last step, combine order, lists -- so their results are bit-identical
 * to the fp32 calls on the widened bank, at half the bytes per pass.  The only approximation is the rounding when the bank is
 * stored.  bank_dtype / dtype / out_dtype: SKYEMB_BF16 or SKYEMB_F16; SKYEMB_F32 and every other code are refused before any
 * launch.  Shapes, alignment (16 bytes for bank and tw) and the remaining arguments as for the calls above;
 * skyemb_cosine_token_applicable and skyemb_cosine_token_topk_chunks hold unchanged for 16-bit banks.
 *   skyemb_weighted_norms_lp   norms [N] of 16-bit rows x [N, D] (D % 4 == 0, x 8-byte aligned): fp32 on the widened values in
 *                              skyemb_weighted_norms' operation order, bit-equal to that call on the widened array.
 *   skyemb_standardise_lp      x fp32 [N, D] -> out 16-bit [N, D] (D % 4 == 0): skyemb_standardise's value, then ONE rounding to
 *                              nearest-even (fp16: overflow -> +-inf, subnormals kept; NaN stays NaN), so a 16-bit bank can be
 *                              built batch by batch without its fp32 image ever existing at full size. */
int skyemb_cosine_token_scores_lp(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn, int Q,
                                  int64_t N, int P, int D, int combine, float eps, float *scores, void *stream);
int skyemb_cosine_token_topk_lp(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn, int Q,
                                int64_t N, int P, int D, int k, int combine, float eps, int64_t idx_offset, int nlists,
                                const float *thr0, float *part_s, int64_t *part_i, void *stream);
int skyemb_weighted_norms_lp(const void *x, int dtype, const float *w, float *norms, int64_t N, int D, void *stream);
int skyemb_standardise_lp(const float *x, const float *mu, const float *sigma, void *out, int out_dtype, int64_t N, int D,
                          void *stream);
/* Top-t combine (additive to ABI version 111: nothing above changes): the reference's n_top_sims.  Only the top_t best token
 * scores of an image count.  With d[0] >= d[1] >= ... >= d[P-1] the image's token scores in descending order (-inf, which a
 * NaN score ranks as, last -- torch.topk would rank NaN largest):
 *   MAX   d[0], the plain MAX bit for bit (any top_t);
 *   MIN   d[top_t-1]; top_t == P is the plain MIN bit for bit;
 *   MEAN  (((0 + d[0]) + d[1]) + ... + d[top_t-1]) / (float)top_t: one fp32 rounding per add, LARGEST FIRST, one IEEE division,
 *         NaN -> -inf.  Equal values are interchangeable, so the sum does not depend on how ties are ordered, nor on launch
 *         geometry, Q or bank dtype.  top_t == P is NOT the plain MEAN, which sums in token order.
 * An image with fewer than top_t scores above -inf gives -inf under MIN and MEAN and is never listed.
 * top_t: 1 .. min(P, 16), or 0 = all tokens: then the call IS the plain call for that bank type (same kernel, same bits, one
 * launch).  bank_dtype: SKYEMB_F32, SKYEMB_F16 or SKYEMB_BF16 (`bank` points to that element type).  Everything else -- shapes
 * (skyemb_cosine_token_applicable), nlists (skyemb_cosine_token_topk_chunks), alignment, thr0, idx_offset, list format -- as
 * for skyemb_cosine_token_scores / skyemb_cosine_token_topk.  A bad dtype, an unknown combine, a top_t out of range or a bad
 * shape returns 1 before any launch with the cause as skyemb_last_error. */
int skyemb_cosine_token_scores_top(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn, int Q,
                                   int64_t N, int P, int D, int combine, int top_t, float eps, float *scores, void *stream);
int skyemb_cosine_token_topk_top(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn, int Q,
                                 int64_t N, int P, int D, int k, int combine, int top_t, float eps, int64_t idx_offset, int nlists,
                                 const float *thr0, float *part_s, int64_t *part_i, void *stream);
/* Selection (additive to ABI version 111: nothing above changes): the `_top` calls restricted to a selection of the bank's
 * images.  `select` is a packed bitmask on the device: bit (i & 31) of 32-bit word (i >> 5) is image i, ceil(N / 32) words, the
 * padding bits of the last word zero (skyemb_pack_select writes exactly that); it is only read.  The result is that of the same
 * call over the compacted bank (the selected images in their order), every image index mapped back to the whole bank and then
 * offset by idx_offset: scores bit-equal, order (score desc, image asc).  Deselected images contribute nothing -- a NaN or inf in
 * their tokens changes no output -- and, for 16 | P, none of their rows or norms is loaded (P | 16: a 16-row tile is passed over
 * when every image in it is deselected).  skyemb_cosine_token_scores_sel writes all [Q, N] slots: -inf for a deselected image.
 * Fewer than k selected images: the lists end with the (-inf, -1) terminator as ever.  Launch geometry, nlists and every limit
 * are those of the whole bank; one selection serves all queries of the call.  select == NULL IS the `_top` call.  Refusals
 * before any launch: those of the `_top` calls, and a `select` that is not 4-byte aligned.
 *   skyemb_pack_select   flags u8 [N] on the device (non-zero = selected) -> words u32 [ceil(N / 32)]; one short launch. */
int skyemb_cosine_token_scores_sel(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn, int Q,
                                   int64_t N, int P, int D, int combine, int top_t, float eps, float *scores,
                                   const uint32_t *select, void *stream);
int skyemb_cosine_token_topk_sel(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn, int Q,
                                 int64_t N, int P, int D, int k, int combine, int top_t, float eps, int64_t idx_offset, int nlists,
                                 const float *thr0, float *part_s, int64_t *part_i, const uint32_t *select, void *stream);
int skyemb_pack_select(const uint8_t *flags, int64_t N, uint32_t *words, void *stream);

/* Weighted MSE / MAE patch-token search (additive to ABI version 111: nothing above changes): utils/similarity.py:174-212 scored
 * token by token and combined per image (214-268), for Q <= 16 queries t [Q, D] over a bank [N, P, D] of fp32, fp16 or bf16
 * (bank_dtype: SKYEMB_F32 / SKYEMB_F16 / SKYEMB_BF16).  c [D] = fp32(w / sum(w)), prepared by the caller (w = 1 without weights).
 *
 * Arithmetic contract (csrc/distance_tokens.hip and tests/token_distance_reference.py state the same, word for word):
 *   All arithmetic is fp32, every operation rounds to nearest even on its own, and there is no fused multiply-add anywhere in
 *   the score.  With x [D] a bank row (a 16-bit row is widened exactly on load):
 *     term[d] = c[d] * v[d],  v[d] = |x[d] - t[d]| for MAE,  v[d] = (x[d] - t[d]) * (x[d] - t[d]) for MSE;
 *     16 partial sums: p[j] = 0, then p[j] = p[j] + term[d] over the elements with (d >> 2) & 15 == j, in ascending d;
 *     four folds: p[j] = p[j] + p[j ^ 8], then p[j] = p[j] + p[j ^ 4], then p[j] = p[j] + p[j ^ 2], then p[j] = p[j] + p[j ^ 1]
 *     (every fold on all 16 partials at once; addition commutes, so afterwards all 16 are equal);
 *     dist = p[0] / (float)D, one IEEE division.
 *   The order does not depend on Q, launch geometry, wave, P, bank dtype, top_t or the selection.  A 16-bit bank gives the fp32
 *   call's result on the widened bank, bit for bit.
 *
 * Ordering and combine.  Smaller is better.  The kernels work on key = -dist, an exact negation, and a NaN token distance ranks
 * as key -inf, i.e. distance +inf (torch would propagate the NaN).  With a[0] <= a[1] <= ... the top_t smallest token distances
 * of an image (top_t == 0: all P of them):
 *   MIN   a[0], for every top_t;
 *   MAX   the largest of those used: a[top_t - 1], or the plain max for top_t == 0;
 *   MEAN  (((0 + a[0]) + a[1]) + ...) / (float)top_t, smallest first; top_t == 0: token order p = 0 .. P-1, divided by (float)P.
 * In key space these ARE the cosine search's MAX, MIN and MEAN (negation commutes with every rounding), so its combine code,
 * lists, thr0 floors, ties (key descending, image ascending), the (-inf, -1) terminator and skyemb_topk_merge serve unchanged.
 * A +inf token distance is ignored by MIN and makes MAX and MEAN +inf; under MAX and MEAN an image with fewer than top_t finite
 * token distances combines to +inf; an image whose combined distance is +inf is never returned.
 *
 *   skyemb_distance_token_scores  scores [Q, N]: every slot is written as a DISTANCE; a deselected image gets +inf.
 *   skyemb_distance_token_topk    part_s f32 / part_i i64 [Q, nlists, k] in KEY space (part_s = -distance, best first, ended by
 *                                 (-inf, -1)), nlists = skyemb_cosine_token_topk_chunks(N, P, Q, D, k); thr0 [Q] (or NULL):
 *                                 per-query key floors, only keys strictly above enter.  skyemb_topk_merge merges them as they are;
 *                                 the caller negates the merged keys.
 * metric: SKYEMB_METRIC_MSE | SKYEMB_METRIC_MAE; combine: SKYEMB_COMBINE_*; top_t: 0 (all tokens) or 1 .. min(P, 16); select: NULL
 * or the packed words of skyemb_pack_select (a deselected image costs no HBM bytes when 16 | P).  Shape limits: those of
 * skyemb_cosine_token_applicable (its LDS rule covers these kernels: t takes 4 Q D <= 64 D bytes, four waves' lists 32 Q k).
 * Refusals (return 1 before any launch, text in skyemb_last_error): a bad metric, combine, dtype, top_t or shape, N * P >= 2^31,
 * a wrong nlists, bank / c / t not 16-byte aligned, select not 4-byte aligned. */
#define SKYEMB_METRIC_MSE 1
#define SKYEMB_METRIC_MAE 2
int skyemb_distance_token_scores(const float *c, const float *t, const void *bank, int bank_dtype, int Q, int64_t N, int P, int D,
                                 int metric, int combine, int top_t, float *scores, const uint32_t *select, void *stream);
int skyemb_distance_token_topk(const float *c, const float *t, const void *bank, int bank_dtype, int Q, int64_t N, int P, int D,
                               int metric, int combine, int top_t, int k, int64_t idx_offset, int nlists, const float *thr0,
                               float *part_s, int64_t *part_i, const uint32_t *select, void *stream);

/* Per-query feature weights (additive to ABI version 111: nothing above changes).  The reference derives the weights from the
 * target (utils/similarity.py:134-147), so two targets never share them: here every query q of a call has its own row of
 * w [Q, D] (cosine) or c [Q, D] (distance), and one pass over the bank serves up to 16 targets with 16 weight vectors.
 *
 * Cosine (`skyemb_cosine_token_*_pq`): the `_sel` calls with `w` in place of `xn`; every other argument, select == NULL (every
 * image) included, as there.  tw [Q, D] and qn [Q] are prepared per query with that query's row (skyemb_weighted_norms).  The
 * bank norm is computed in the pass, per (query, row), and no norm array is read:
 *     x2[d] = x[d] * x[d], one fp32 rounding;  acc2 = 0, then acc2 = fma(w[q][d], x2[d], acc2) over d = 0, 1, 2, ... -- the
 *     contract's fma chain of the score with (w_q, x o x) as operands;  xn_q = sqrt(acc2), IEEE;
 *     score = dot / fma(qn[q], xn_q, eps), NaN -> -inf, as in every other call.
 *   This is NOT skyemb_weighted_norms' order (fma(w[d] * x[d], x[d], acc)), so the call with one shared weight vector and this
 *   call with Q identical rows may differ in the last bits of a score.  A 16-bit bank gives the fp32 result on the widened bank,
 *   bit for bit.  A negative acc2 (negative weights) gives a NaN norm and a NaN score, which ranks as -inf; an all-zero weight row
 *   gives the score 0 / eps = 0 for every token.  Combine, top_t, selection, lists, thr0, terminator and skyemb_topk_merge are
 *   those of the `_sel` calls.  Two operand images are resident in LDS, so the shape rule reads 128 D + 32 Q k <= 163840 where
 *   skyemb_cosine_token_applicable has 64 D: skyemb_cosine_token_pq_applicable(Q, P, D, k) says so without touching the device and
 *   on 0 leaves the limits and the refused shape as skyemb_last_error.  nlists is skyemb_cosine_token_topk_chunks', unchanged.
 *   Refusals before any launch: those of the `_sel` calls with this shape rule, and a `w` that is not 16-byte aligned.
 *
 * Distance (`skyemb_distance_token_*_pq`): the calls above with c [Q, D], row q = fp32(w_q / sum(w_q)); term[d] of query q is
 *   c[q][d] * v[d] and the arithmetic contract holds word for word, so query q's result is bit-identical to the single-c call
 *   with that row.  c sits in LDS beside t (8 Q D <= 128 D bytes together), so the shape rule is
 *   skyemb_cosine_token_pq_applicable's; the remaining refusals are those of the calls above.
 *
 * Per-query token-position masks and per-query selections remain out of scope: one `select` serves all queries of a call. */
int skyemb_cosine_token_pq_applicable(int Q, int P, int D, int k);
int skyemb_cosine_token_scores_pq(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *w, int Q,
                                  int64_t N, int P, int D, int combine, int top_t, float eps, float *scores,
                                  const uint32_t *select, void *stream);
int skyemb_cosine_token_topk_pq(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *w, int Q,
                                int64_t N, int P, int D, int k, int combine, int top_t, float eps, int64_t idx_offset, int nlists,
                                const float *thr0, float *part_s, int64_t *part_i, const uint32_t *select, void *stream);
int skyemb_distance_token_scores_pq(const float *c, const float *t, const void *bank, int bank_dtype, int Q, int64_t N, int P, int D,
                                    int metric, int combine, int top_t, float *scores, const uint32_t *select, void *stream);
int skyemb_distance_token_topk_pq(const float *c, const float *t, const void *bank, int bank_dtype, int Q, int64_t N, int P, int D,
                                  int metric, int combine, int top_t, int k, int64_t idx_offset, int nlists, const float *thr0,
                                  float *part_s, int64_t *part_i, const uint32_t *select, void *stream);

/* ------------------------------------------------------- linear-probe fits -
 * (additive to ABI version 111: nothing above changes.)  utils/pretrain_fns.py:52-159 fits two scikit-learn estimators on the
 * host every `verbose_iters` iterations: StandardScaler + LogisticRegression(lbfgs, C = 0.01) on `class` and
 * ElasticNet(alpha = 1e-4, l1_ratio = 0.9) on `zspec`.  These calls are the device side of the same fits
 * (sky_embeddings_amd/probe.py drives them; csrc/probe.hip).  No atomics: every sum has one order that the shapes alone fix
 * (SKYEMB_PROBE_CHUNKS row chunks added in chunk order, fixed trees, one thread per output), so results depend neither on
 * launch geometry nor on the row strides ldx / ldo (elements, >= F).  Bad shapes and null pointers return 1 before any launch.
 *
 *   skyemb_probe_colstats   X [n, F] fp32 -> mean, var (population), scale = sqrt(var), exactly 1 where var == 0
 *                           (StandardScaler's rule), all fp64 [F], two passes (sum, then sum of squared deviations).
 *                           ws: fp64 [SKYEMB_PROBE_CHUNKS * F].
 *   skyemb_probe_scale      out[i, f] = fp32((X[i, f] - mean[f]) / scale[f]) in fp64, one rounding; scale == NULL: centre only.
 *                           Any rows (the held-out split takes the fit split's mean / scale); out may be X.
 *   skyemb_probe_softmax_loss_grad   multinomial logistic regression, 3 <= K <= 16 classes, F <= SKYEMB_PROBE_MAX_F:
 *                           loss = (1 / m) sum_i CE_i + 0.5 l2 ||W||^2 (fp64, device), gW [K, F] = R^T X + l2 W, gb [K] = column
 *                           sums of R, R = (softmax - onehot) / m.  X [m, F], W [K, F], b [K] fp32, y int32 in [0, K).
 *                           Logits, max-subtracted softmax and R in fp32; row losses, the chunk sums of gW, gb and ||W||^2 are
 *                           added in fp64; gW, gb are stored as fp32.  ws: skyemb_probe_softmax_ws_bytes(m, F, K) bytes, 8-byte
 *                           aligned (-1 for a refused shape).
 *   skyemb_probe_gram       Xc [m, F] fp32 (centred), yc [m] fp32 -> G = Xc^T Xc fp64 [F, F] (symmetric bit for bit), q = Xc^T yc
 *                           fp64 [F], ynorm2 = ||yc||^2 (one fp64): inputs widened exactly, fp64 fma chains over the rows in
 *                           ascending order.  F <= SKYEMB_PROBE_MAX_F.
 *   skyemb_probe_enet_cd    cyclic coordinate descent (scikit-learn's selection = 'cyclic', Gram form) from w = 0 by ONE persistent
 *                           workgroup, w and H = G w fp64 in LDS: for j = 0 .. F-1 with G[j, j] != 0:
 *                             t = (q[j] - H[j]) + w[j] G[j, j];  w[j] = sign(t) max(|t| - a1, 0) / (G[j, j] + b2);  H += dw G[:, j].
 *                           After a sweep with max|dw| / max|w| < tol, or max|w| == 0, or the last one: the duality gap of
 *                           scikit-learn's enet_coordinate_descent_gram; stop when gap < tol * ynorm2.
 *                           a1 = alpha l1_ratio m, b2 = alpha (1 - l1_ratio) m.  -> w fp64 [F], status int32[2] = {sweeps run,
 *                           1 if the gap test passed else 0}, gap (the last one computed; tol + 1 if none). */
#define SKYEMB_PROBE_CHUNKS 32
#define SKYEMB_PROBE_MAX_F 4096
#define SKYEMB_PROBE_MIN_K 3
#define SKYEMB_PROBE_MAX_K 16
int skyemb_probe_colstats(const float *X, int64_t ldx, int n, int F, double *mean, double *var, double *scale, double *ws,
                          void *stream);
int skyemb_probe_scale(const float *X, int64_t ldx, int n, int F, const double *mean, const double *scale, float *out, int64_t ldo,
                       void *stream);
int64_t skyemb_probe_softmax_ws_bytes(int m, int F, int K);
int skyemb_probe_softmax_loss_grad(const float *X, int64_t ldx, const int32_t *y, int m, int F, int K, const float *W, const float *b,
                                   double l2, double *loss, float *gW, float *gb, void *ws, int64_t ws_bytes, void *stream);
int skyemb_probe_gram(const float *Xc, int64_t ldx, const float *yc, int m, int F, double *G, double *q, double *ynorm2, void *stream);
int skyemb_probe_enet_cd(const double *G, const double *q, const double *ynorm2, int F, double a1, double b2, int max_iter, double tol,
                         double *w, int32_t *status, double *gap, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SKYEMB_H */
