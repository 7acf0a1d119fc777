// Patch-token bank search for Q <= 16 queries: the bank holds P consecutive rows (patch tokens) per image, every token is
// scored with the contract's fp32 fma chain (same arithmetic as cosine_topk_stream_kernel: rows straight from HBM into
// registers, v_mfma_f32_16x16x4_f32), the P token scores of an image are combined in registers (min | mean | max,
// utils/similarity.py:262-267) and ONE candidate per image goes to the wave's private sorted lists.  The [Q, N * P] token score
// matrix never reaches memory.
//
// P divides 16 (an image is P neighbouring lanes of a 16-row tile) or is a multiple of 16 (an image is P / 16 consecutive tiles
// of ONE wave: rows per wave are a multiple of lcm(P, 16), so no image straddles two waves).
//
// Combine order (fp32): min and max are exact.  mean = (((0 + s[0]) + s[1]) + ... + s[P-1]) / (float)P: token order
// p = 0 .. P-1, one IEEE division; every lane of an image's lane group runs the same chain, tiles of a long image are folded in
// ascending order, so the result does not depend on the launch geometry, on the wave or on Q.  A -inf token score (NaN scores
// rank as -inf) gives -inf for min and mean and is ignored by max; an image whose combined score is -inf never enters a list.
//
// Bank element type T: float, or bf16_t / f16_t for a half-precision resident bank (the `_lp` entry points).  A 16-bit row is
// widened exactly on its way into the MFMA operands (mfma32_lp, topk_stream.h); everything after the load is the same code, so a
// 16-bit bank gives the fp32 kernel's result on the widened bank bit for bit, for half the bytes.
//
// Top-t combine (TOPT, the `_top` entry points; the reference's n_top_sims): only the top_t (1 .. min(P, 16)) best token scores
// of an image count.  d[0] >= d[1] >= ... the image's scores in descending order, -inf last: min = d[top_t-1],
// mean = (((0 + d[0]) + d[1]) + ... + d[top_t-1]) / (float)top_t, largest first (NOT the plain mean's token order, also for
// top_t == P); max is d[0], the plain max kernel.  The image's lane group sorts its scores with a bitonic network over
// DPP lane permutes; a long image keeps its 16 best as one float per lane in `carry` (the plain combine's registers): per tile
// max(carry[i], new[15 - i]) is the 16 largest of the union as a bitonic sequence, which a bitonic merge sorts again.  Equal
// values are interchangeable, so neither result depends on how the network orders ties.  An image with fewer than top_t
// scores above -inf gives -inf.  No LDS and no global scratch beyond the plain kernel's.
//
// Selection (SEL, the `_sel` entry points): a packed bitmask over the images (bit i & 31 of 32-bit word i >> 5 is image i,
// ceil(N / 32) words, padding bits zero; skyemb_pack_select builds it) restricts the search to the images whose bit is set: the
// result is that of the compacted bank, image indices mapped back.  The decision is per wave (a counter of images and the mask word of
// the current 32 images live in scalar registers; the word is loaded by every lane once per 32 images and made scalar with
// readfirstlane), so nothing diverges.  16 | P: an image whose bit is clear is passed over whole -- none of its
// P / 16 tiles, neither rows nor norms, is loaded.  P | 16: a tile holds the 16 / P neighbouring images n0 / P ..., whose bits lie
// in one word (n0 / P is a multiple of 16 / P, which divides 32); the tile is passed over when all are clear, else it is scored
// as ever and the lead lanes of the deselected images stay out of the candidate ballot.  Whole images are skipped, so `carry` and
// `tile_in_image` are untouched.  The !LISTS kernel writes -inf for every deselected image.  The mask is only read.
//
// Per-query feature weights (PQW, the `_pq` entry points): every query has its own weight vector w [Q, D] (the reference derives
// the weights from the target, utils/similarity.py:134-147), so the bank norm depends on the query and no precomputed xn serves.
// A second operand image of w sits in LDS beside the A image and a second accumulator chain runs over the fragments the wave
// already holds: acc2 = fma(w_q[d], x2[d], acc2), x2[d] = x[d] * x[d] rounded once, in the score chain's k-step order
// (stream_dot16_pq, topk_stream.h); xn_q = sqrtf(acc2), correctly rounded (sqrtf, not __fsqrt_rn: inside this kernel the compiler
// lowers the latter to the bare v_sqrt_f32 approximation).  From finish_score on the code is the shared one.  No norm array is
// read.  LDS: 128 D + 32 Q k bytes (skyemb_cosine_token_pq_applicable).
#include "topk_stream.h"
#include "token_combine.h"

namespace {

// LISTS: part_s / part_i [Q, nlists, k] as cosine_topk_stream_kernel writes them (idx = idx_offset + image).
// !LISTS: scores [Q, n_img] combined scores.
// TOPT: the top-t combine with 1 <= top_t <= min(P, 16) (MIN and MEAN only); !TOPT ignores top_t.
// SEL: only the images whose bit in `sel` is set take part; !SEL ignores sel.
// PQW: `xw` is w [Q, D], the per-query feature weights; !PQW: `xw` is xn [R], the bank norms under the call's one weight vector.
template <typename T, int WAVES, int COMBINE, bool LISTS, bool TOPT, bool SEL, bool PQW>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu((TOPT || SEL) && WAVES == 8 && !PQW ? 4 : 1)))
void cosine_token_kernel(const float *__restrict__ tw, const float *__restrict__ qn,
                                                                  const T *__restrict__ bank, const float *__restrict__ xw,
                                                                  int Q, int64_t R, int P, int D, int k, float eps,
                                                                  int64_t idx_offset, int64_t rows_per_wave,
                                                                  float *__restrict__ part_s, int64_t *__restrict__ part_i,
                                                                  const float *__restrict__ thr0, float *__restrict__ scores,
                                                                  int64_t n_img, int top_t, const uint32_t *__restrict__ sel) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nchunk = D >> 4;
    float4 *imgA = (float4 *)lds;                                   // [nchunk][64]: A fragments of every k-step
    float4 *imgW = imgA + (size_t)nchunk * 64;                      // PQW: [nchunk][64], the same fragments of w
    float *ls_all = lds + (size_t)nchunk * 64 * 4 * (PQW ? 2 : 1);  // [WAVES][Q][k]
    int *li_all = (int *)(ls_all + (size_t)WAVES * Q * k);         // [WAVES][Q][k]
    build_imgA<WAVES>(imgA, tw, Q, D, nchunk, tid);
    if (PQW) build_imgA<WAVES>(imgW, xw, Q, D, nchunk, tid);        // rows q >= Q are zero
    __syncthreads();
    float *ls = ls_all + (size_t)wave * Q * k;
    int *li = li_all + (size_t)wave * Q * k;
    const int wid = blockIdx.x * WAVES + wave;
    const int64_t r_begin = (int64_t)wid * rows_per_wave;           // a multiple of lcm(P, 16): the first row of an image
    int64_t r_end = r_begin + rows_per_wave;
    if (r_end > R) r_end = R;                                       // R = images x P: whole images only
    const int n_lane = lane & 15, g = lane >> 4;
    const int tp = P < 16 ? P : 16;                                 // lanes of one image in a tile
    const int tiles_per_image = P < 16 ? 1 : P >> 4;
    // per-query list sizes / thresholds live in registers of ALL lanes (wave-uniform arrays of 16)
    int n_in[16];
    float thr[16], floor_thr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        n_in[q] = 0;
        thr[q] = (LISTS && thr0 && q < Q) ? thr0[q] : -INFINITY;
        floor_thr[q] = thr[q];                                      // valid lower bound of the global k-th best (or -inf)
    }
    float qn4[4], carry[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        qn4[r] = (4 * g + r) < Q ? qn[4 * g + r] : 0.f;
        carry[r] = combine_start<COMBINE>();
    }
    const float fP = (float)P;
    int tile_in_image = 0;
    const int lg_tp = __builtin_ctz(tp);                            // SEL, P < 16: lane n of a tile belongs to its image n >> lg_tp
    // SEL: wave-uniform state in scalar registers -- the first image of the coming tile (counted, one division per wave), the
    // mask word of images 32 sel_word_at .. and which word that is
    unsigned sel_img = SEL ? (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)r_begin / (unsigned)P)) : 0u;
    unsigned sel_word = 0;
    int sel_word_at = -1;

    for (int64_t n0 = r_begin; n0 < r_end; n0 += 16) {
        bool on_lane = true;                                        // SEL: this lane's image is selected
        if (SEL && (P < 16 || tile_in_image == 0)) {                // 16 | P: the first tile of an image decides for all of them
            const unsigned img0 = sel_img;                          // the tile's first image (< n_img: n0 < r_end <= R), a scalar
            sel_img += P < 16 ? 16u >> lg_tp : 1u;                  // the first image of the next tile (P | 16) / the next image
            if ((int)(img0 >> 5) != sel_word_at) {                  // one load per 32 images, made scalar
                sel_word_at = (int)(img0 >> 5);
                sel_word = (unsigned)__builtin_amdgcn_readfirstlane((int)sel[sel_word_at]);
            }
            if (P >= 16) {
                if (!((sel_word >> (img0 & 31)) & 1u)) {            // the whole wave passes the image over
                    if (!LISTS && lane < Q) scores[(int64_t)lane * n_img + img0] = -INFINITY;
                    n0 += P - 16;
                    continue;
                }
            } else {
                const int ipt = 16 >> lg_tp;                        // images per tile; their bits lie in one word
                const unsigned bits = (sel_word >> (img0 & 31)) & (0xffffu >> (16 - ipt));   // padding bits are zero: images past n_img
                if (bits == 0) {                                    // no image of this tile is selected
                    if (!LISTS)
                        for (int e = lane; e < ipt * Q; e += 64) {
                            const int64_t img = (int64_t)img0 + (e & (ipt - 1));
                            if (img < n_img) scores[(int64_t)(e >> (4 - lg_tp)) * n_img + img] = -INFINITY;
                        }
                    continue;
                }
                on_lane = (bits >> (n_lane >> lg_tp)) & 1u;
            }
        }
        int64_t row = n0 + n_lane;
        const bool row_ok = row < r_end;
        if (!row_ok) row = r_end - 1;                                // clamp: masked below
        const T *src = bank + row * D + lane_elems<T>() * g;
        f32x4 acc, acc2 = {0.f, 0.f, 0.f, 0.f};
        if (PQW) acc = stream_dot16_pq(src, imgA, imgW, nchunk, lane, acc2);
        else acc = stream_dot16(src, imgA, nchunk, lane);
        // C/D: col = lane&15 -> bank row n0 + n_lane, row = 4g + r -> query
        const float xnv = PQW ? 0.f : xw[row];
        const bool first_tile = tile_in_image == 0;
        const bool last_tile = ++tile_in_image == tiles_per_image;
        if (last_tile) tile_in_image = 0;
        // the image's first lane speaks for it (a row past r_end belongs to an image past r_end)
        const bool lead = last_tile && (n_lane & (tp - 1)) == 0 && row_ok;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q_mine = 4 * g + r;
            const float s = (row_ok && q_mine < Q) ? finish_score(acc[r], qn4[r], PQW ? sqrtf(acc2[r]) : xnv, eps) : -INFINITY;
            float c;
            if (TOPT) {
                carry[r] = top_tile(s, carry[r], n_lane, tp, first_tile);
                c = last_tile ? top_finish<COMBINE>(carry[r], lane, tp, top_t) : -INFINITY;   // wave-uniform
            } else {
                c = combine_tile<COMBINE>(s, carry[r], lane, tp);
                carry[r] = last_tile ? combine_start<COMBINE>() : c;
                if (COMBINE == SKYEMB_COMBINE_MEAN && last_tile) {      // wave-uniform: the sum is complete
                    c = __fdiv_rn(c, fP);
                    c = c == c ? c : -INFINITY;
                }
            }
            if (!LISTS) {
                if (SEL && !on_lane) c = -INFINITY;
                if (lead && q_mine < Q) scores[(int64_t)q_mine * n_img + (int64_t)((unsigned)(n0 + n_lane) / (unsigned)P)] = c;
                continue;
            }
            // candidates of the 4 queries {r, 4+r, 8+r, 12+r} (one per lane group), images ascending within a group
            float my_thr = -INFINITY;
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) my_thr = (g == gg) ? thr[4 * gg + r] : my_thr;
            unsigned long long m = __ballot(lead && (!SEL || on_lane) && q_mine < Q && c > my_thr);
            while (m) {
                const int srcl = __builtin_ctzll(m);
                m &= m - 1;
                const float cv = __shfl(c, srcl, 64);
                const int q = 4 * (srcl >> 4) + r;
                float *lsq = ls + q * k;
                int *liq = li + q * k;
                // wave-uniform per-query state (static indexing through the unrolled select)
                int nq = 0;
                float tq = -INFINITY;
#pragma unroll
                for (int gg = 0; gg < 4; ++gg)
                    if (q == 4 * gg + r) { nq = n_in[4 * gg + r]; tq = thr[4 * gg + r]; }
                if (!(cv > tq)) continue;
                const int image = (int)((unsigned)(n0 + (srcl & 15)) / (unsigned)P);
                const int new_n = stream_list_insert(lsq, liq, nq, k, cv, image, lane);
                const float kth = new_n == k ? lsq[k - 1] : -INFINITY;
#pragma unroll
                for (int gg = 0; gg < 4; ++gg)
                    if (q == 4 * gg + r) {
                        n_in[4 * gg + r] = new_n;
                        thr[4 * gg + r] = new_n == k ? kth : floor_thr[4 * gg + r];
                    }
            }
        }
    }
    if (!LISTS) return;
    // write this wave's lists: part[q][wid][k], the entries and ONE terminator (-inf, -1) as cosine_topk_stream_kernel does
    const int nlists = gridDim.x * WAVES;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (q >= Q) continue;
        const int64_t o = ((int64_t)q * nlists + wid) * k;
        const int n_out = n_in[q] < k ? n_in[q] + 1 : k;
        for (int e = lane; e < n_out; e += 64) {
            const bool have = e < n_in[q];
            part_s[o + e] = have ? ls[q * k + e] : -INFINITY;
            part_i[o + e] = have ? idx_offset + (int64_t)li[q * k + e] : -1;
        }
    }
}

constexpr int LDS_BYTES = 160 * 1024;

size_t image_bytes(int D) { return (size_t)(D >> 4) * 64 * 16; }   // the A operand image: 64 D bytes

// 8 waves per workgroup when their private lists (Q x k entries of 8 bytes each) fit next to the A image, else 4
// (images: 1, or 2 with per-query weights -- the w image is as large as the A image)
int token_waves(int Q, int D, int k, int images = 1) {
    return images * image_bytes(D) + (size_t)8 * 8 * Q * k <= (size_t)LDS_BYTES ? 8 : 4;
}

// the shape limits of both predicates: k <= 512 is the list capacity skyemb_topk_merge sorts; four waves' lists sit next to the
// operand images (1, or 2 with per-query weights): images x 64 D + 32 Q k <= 160 KiB
bool token_shape_ok(int images, int Q, int P, int D, int k) {
    return Q >= 1 && Q <= 16 && D >= 64 && D % (16 * UNROLL) == 0 && D <= 1024 && P >= 1 && P <= 4096 && (16 % P == 0 || P % 16 == 0) &&
           k >= 1 && k <= 512 && images * image_bytes(D) + (size_t)4 * 8 * Q * k <= (size_t)LDS_BYTES;
}

// which bank_dtype codes an entry point takes
enum Dtypes { F32_ONLY, LP_ONLY, ANY_DTYPE };

// One call.  The entry points fill the first block; token_topk / token_scores add their own; token_call checks it all and
// works out the geometry.
struct Launch {
    const char *who;
    Dtypes dtypes;
    bool pq;                                                        // xw is w [Q, D] (the `_pq` calls), else xn [N * P]
    const float *tw, *qn;
    const void *bank;
    int bank_dtype;
    const float *xw;
    int Q;
    int64_t N;
    int P, D, combine, top_t;
    float eps;
    const uint32_t *sel;                                            // nullptr: the kernels without the selection switch
    hipStream_t st;
    // the top-k call: lists part_s / part_i [Q, nlists, k]; the scores call: scores [Q, N], at k = 1
    int k = 1, nlists = 0;
    int64_t idx_offset = 0, *part_i = nullptr;
    const float *thr0 = nullptr;
    float *part_s = nullptr, *scores = nullptr;
    // geometry
    int blocks = 0;
    size_t smem = 0;
    int64_t R = 0, rows_per_wave = 0;
};

template <typename T, int WAVES, int COMBINE, bool LISTS, bool TOPT, bool SEL, bool PQW>
int launch_kernel(const Launch &a, const T *bank) {
    const auto kern = cosine_token_kernel<T, WAVES, COMBINE, LISTS, TOPT, SEL, PQW>;
    if (a.smem > 64 * 1024) {
        const int rc = sky_set_lds_limit((const void *)kern, LDS_BYTES, a.who);
        if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)a.blocks), dim3(WAVES * 64), a.smem, a.st, a.tw, a.qn, bank, a.xw, a.Q, a.R, a.P, a.D, a.k, a.eps,
                       a.idx_offset, a.rows_per_wave, a.part_s, a.part_i, a.thr0, a.scores, a.N, a.top_t, a.sel);
    SKY_LAUNCH_CHECK(a.who);
    return 0;
}

// the choice of the instantiation: per-query weights, selection, then combine and top-t
template <typename T, int WAVES, bool LISTS, bool SEL, bool PQW>
int launch_combine(const Launch &a, const T *bank) {
    // top_t == 0: all tokens, the plain kernels; max is d[0] for every top_t, the plain max kernel
    if (a.top_t != 0 && a.combine == SKYEMB_COMBINE_MIN) return launch_kernel<T, WAVES, SKYEMB_COMBINE_MIN, LISTS, true, SEL, PQW>(a, bank);
    if (a.top_t != 0 && a.combine == SKYEMB_COMBINE_MEAN) return launch_kernel<T, WAVES, SKYEMB_COMBINE_MEAN, LISTS, true, SEL, PQW>(a, bank);
    if (a.combine == SKYEMB_COMBINE_MIN) return launch_kernel<T, WAVES, SKYEMB_COMBINE_MIN, LISTS, false, SEL, PQW>(a, bank);
    if (a.combine == SKYEMB_COMBINE_MEAN) return launch_kernel<T, WAVES, SKYEMB_COMBINE_MEAN, LISTS, false, SEL, PQW>(a, bank);
    return launch_kernel<T, WAVES, SKYEMB_COMBINE_MAX, LISTS, false, SEL, PQW>(a, bank);
}

template <typename T, int WAVES, bool LISTS, bool PQW>
int launch_sel(const Launch &a, const T *bank) {
    return a.sel ? launch_combine<T, WAVES, LISTS, true, PQW>(a, bank) : launch_combine<T, WAVES, LISTS, false, PQW>(a, bank);
}

template <int WAVES, bool LISTS, typename T>
int launch_tokens(const Launch &a, const T *bank) {
    return a.pq ? launch_sel<T, WAVES, LISTS, true>(a, bank) : launch_sel<T, WAVES, LISTS, false>(a, bank);
}

}  // namespace

#define TOKEN_LIMITS_MSG "needs Q <= 16, D %% 64 == 0, D <= 1024, 1 <= P <= 4096 with 16 %% P == 0 or P %% 16 == 0, 1 <= k <= 512 and "
#define TOKEN_SHAPE_MSG TOKEN_LIMITS_MSG "64 D + 32 Q k <= 163840 bytes of LDS (Q=%d P=%d D=%d k=%d)"
#define TOKEN_PQ_SHAPE_MSG TOKEN_LIMITS_MSG "128 D + 32 Q k <= 163840 bytes of LDS (Q=%d P=%d D=%d k=%d)"

// The one statement of the shape limits: a refusal leaves it as the library's error text (skyemb_last_error), which the callers
// -- the entry points below, distance_tokens.hip and the Python layer -- pass on instead of restating it.
extern "C" int skyemb_cosine_token_applicable(int Q, int P, int D, int k) {
    const bool ok = token_shape_ok(1, Q, P, D, k);
    if (!ok) skyemb_set_error("patch-token search " TOKEN_SHAPE_MSG, Q, P, D, k);
    return ok ? 1 : 0;
}

// The same for the calls with per-query weights: two operand images (tw and w) are resident, so 128 D takes the place of 64 D.
extern "C" int skyemb_cosine_token_pq_applicable(int Q, int P, int D, int k) {
    const bool ok = token_shape_ok(2, Q, P, D, k);
    if (!ok) skyemb_set_error("patch-token search with per-query weights " TOKEN_PQ_SHAPE_MSG, Q, P, D, k);
    return ok ? 1 : 0;
}

extern "C" int skyemb_cosine_token_topk_chunks(int64_t N, int P, int Q, int D, int k) {
    if (N < 1 || !skyemb_cosine_token_applicable(Q, P, D, k)) return 0;
    const int waves = token_waves(Q, D, k);
    const int64_t per_wave = image_unit(P) < 64 ? 64 : image_unit(P);   // at least 64 rows and one whole image per wave
    int64_t blocks = 256;
    while (blocks > 1 && blocks * waves * per_wave > N * P) blocks >>= 1;
    return (int)(blocks * waves);
}

// the texts an entry point refuses a bank_dtype code with -- before anything else, so a refused code never reaches a launch
#define LP_DTYPE_MSG "bank_dtype must be SKYEMB_BF16 (0) or SKYEMB_F16 (2), got %d (an fp32 bank takes the call without _lp)"
#define TOP_DTYPE_MSG "bank_dtype must be SKYEMB_BF16 (0), SKYEMB_F32 (1) or SKYEMB_F16 (2), got %d"

namespace {

// The argument checks of every call, in one order.  lists: the top-k call (part_i and nlists count), else the scores call.
int check_tokens(const Launch &a, bool lists) {
    const char *who = a.who;
    const int Q = a.Q, P = a.P, D = a.D, k = a.k;
    SKY_CHECK_ARG(a.tw && a.qn && a.bank && a.xw && (lists ? a.part_s && a.part_i : a.scores != nullptr) && a.N > 0, "%s: bad arguments",
                  who);
    if (a.pq) SKY_CHECK_ARG(skyemb_cosine_token_pq_applicable(Q, P, D, k), "%s: " TOKEN_PQ_SHAPE_MSG, who, Q, P, D, k);
    else SKY_CHECK_ARG(skyemb_cosine_token_applicable(Q, P, D, k), "%s: " TOKEN_SHAPE_MSG, who, Q, P, D, k);
    SKY_CHECK_ARG(a.combine == SKYEMB_COMBINE_MIN || a.combine == SKYEMB_COMBINE_MEAN || a.combine == SKYEMB_COMBINE_MAX,
                  "%s: unknown combine code %d", who, a.combine);
    SKY_CHECK_ARG(a.top_t >= 0 && a.top_t <= (P < 16 ? P : 16), "%s: top_t must be 0 (all tokens) or 1 .. min(P, 16) (top_t=%d P=%d)", who,
                  a.top_t, P);
    SKY_CHECK_ARG(a.N * P < (1ll << 31), "%s: %s too large (N * P < 2^31 rows per call)", who, lists ? "shard" : "bank");
    if (lists)
        SKY_CHECK_ARG(a.nlists == skyemb_cosine_token_topk_chunks(a.N, P, Q, D, k),
                      "%s: nlists must come from skyemb_cosine_token_topk_chunks", who);
    SKY_CHECK_ARG(aligned16(a.bank) && aligned16(a.tw), "%s: bank and tw must be 16-byte aligned", who);
    if (a.pq) SKY_CHECK_ARG(aligned16(a.xw), "%s: w must be 16-byte aligned", who);
    SKY_CHECK_ARG(((uintptr_t)a.sel & 3) == 0, "%s: select must be 4-byte aligned", who);
    return 0;
}

// Every call: the dtype refusal, the checks, the launch geometry, the launch.  lists: 8 or 4 waves per workgroup (nlists is a
// multiple of either) and their lists in LDS; else the scores call's 4 waves.
int token_call(Launch a, bool lists) {
    if (a.dtypes == LP_ONLY) SKY_CHECK_ARG(sky_is_lp(a.bank_dtype), "%s: " LP_DTYPE_MSG, a.who, a.bank_dtype);
    if (a.dtypes == ANY_DTYPE)
        SKY_CHECK_ARG(a.bank_dtype == SKYEMB_F32 || sky_is_lp(a.bank_dtype), "%s: " TOP_DTYPE_MSG, a.who, a.bank_dtype);
    if (check_tokens(a, lists)) return 1;
    const int images = a.pq ? 2 : 1;
    const int waves = lists ? token_waves(a.Q, a.D, a.k, images) : 4;
    a.R = a.N * a.P;
    a.blocks = (int)(lists ? a.nlists / waves : token_scores_blocks(a.R, a.P));
    a.smem = images * image_bytes(a.D) + (lists ? (size_t)2 * 4 * waves * a.Q * a.k : 0);
    a.rows_per_wave = token_rows_per_wave(a.R, (int64_t)a.blocks * waves, a.P);
    return with_bank_type(a.bank, a.bank_dtype, [&](auto *b) {
        if (!lists) return launch_tokens<4, false>(a, b);
        return waves == 8 ? launch_tokens<8, true>(a, b) : launch_tokens<4, true>(a, b);
    });
}

int token_topk(Launch a, int k, int64_t idx_offset, int nlists, const float *thr0, float *part_s, int64_t *part_i) {
    a.k = k, a.idx_offset = idx_offset, a.nlists = nlists, a.thr0 = thr0, a.part_s = part_s, a.part_i = part_i;
    return token_call(a, true);
}

int token_scores(Launch a, float *scores) {
    a.scores = scores;
    return token_call(a, false);
}

}  // namespace

extern "C" int skyemb_cosine_token_topk(const float *tw, const float *qn, const float *bank, const float *xn, int Q, int64_t N,
                                        int P, int D, int k, int combine, float eps, int64_t idx_offset, int nlists,
                                        const float *thr0, float *part_s, int64_t *part_i, void *stream) {
    return token_topk({"skyemb_cosine_token_topk", F32_ONLY, false, tw, qn, bank, SKYEMB_F32, xn, Q, N, P, D, combine, 0, eps, nullptr,
                       (hipStream_t)stream}, k, idx_offset, nlists, thr0, part_s, part_i);
}

extern "C" int skyemb_cosine_token_scores(const float *tw, const float *qn, const float *bank, const float *xn, int Q, int64_t N,
                                          int P, int D, int combine, float eps, float *scores, void *stream) {
    return token_scores({"skyemb_cosine_token_scores", F32_ONLY, false, tw, qn, bank, SKYEMB_F32, xn, Q, N, P, D, combine, 0, eps, nullptr,
                         (hipStream_t)stream}, scores);
}

// Half-precision resident banks: the same two calls on a bf16 / fp16 bank (include/skyemb.h).
extern "C" int skyemb_cosine_token_topk_lp(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn, int Q,
                                           int64_t N, int P, int D, int k, int combine, float eps, int64_t idx_offset, int nlists,
                                           const float *thr0, float *part_s, int64_t *part_i, void *stream) {
    return token_topk({"skyemb_cosine_token_topk_lp", LP_ONLY, false, tw, qn, bank, bank_dtype, xn, Q, N, P, D, combine, 0, eps, nullptr,
                       (hipStream_t)stream}, k, idx_offset, nlists, thr0, part_s, part_i);
}

extern "C" int skyemb_cosine_token_scores_lp(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn,
                                             int Q, int64_t N, int P, int D, int combine, float eps, float *scores, void *stream) {
    return token_scores({"skyemb_cosine_token_scores_lp", LP_ONLY, false, tw, qn, bank, bank_dtype, xn, Q, N, P, D, combine, 0, eps, nullptr,
                         (hipStream_t)stream}, scores);
}

// Top-t combine (include/skyemb.h): one pair of calls for the three bank element types.  top_t == 0 is the plain call of that
// type: the same checks, the same kernel, the same launch.
extern "C" int skyemb_cosine_token_topk_top(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn, int Q,
                                            int64_t N, int P, int D, int k, int combine, int top_t, float eps, int64_t idx_offset,
                                            int nlists, const float *thr0, float *part_s, int64_t *part_i, void *stream) {
    return token_topk({"skyemb_cosine_token_topk_top", ANY_DTYPE, false, tw, qn, bank, bank_dtype, xn, Q, N, P, D, combine, top_t, eps,
                       nullptr, (hipStream_t)stream}, k, idx_offset, nlists, thr0, part_s, part_i);
}

extern "C" int skyemb_cosine_token_scores_top(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn,
                                              int Q, int64_t N, int P, int D, int combine, int top_t, float eps, float *scores,
                                              void *stream) {
    return token_scores({"skyemb_cosine_token_scores_top", ANY_DTYPE, false, tw, qn, bank, bank_dtype, xn, Q, N, P, D, combine, top_t, eps,
                         nullptr, (hipStream_t)stream}, scores);
}

// Selection (include/skyemb.h): the `_top` calls restricted to the images whose bit is set in `select`.  select == NULL IS the
// `_top` call (one definition of the plain call: its checks, its kernels, its error texts).
extern "C" int skyemb_cosine_token_topk_sel(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn, int Q,
                                            int64_t N, int P, int D, int k, int combine, int top_t, float eps, int64_t idx_offset,
                                            int nlists, const float *thr0, float *part_s, int64_t *part_i, const uint32_t *select,
                                            void *stream) {
    return token_topk({select ? "skyemb_cosine_token_topk_sel" : "skyemb_cosine_token_topk_top", ANY_DTYPE, false, tw, qn, bank, bank_dtype,
                       xn, Q, N, P, D, combine, top_t, eps, select, (hipStream_t)stream}, k, idx_offset, nlists, thr0, part_s, part_i);
}

extern "C" int skyemb_cosine_token_scores_sel(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *xn,
                                              int Q, int64_t N, int P, int D, int combine, int top_t, float eps, float *scores,
                                              const uint32_t *select, void *stream) {
    return token_scores({select ? "skyemb_cosine_token_scores_sel" : "skyemb_cosine_token_scores_top", ANY_DTYPE, false, tw, qn, bank,
                         bank_dtype, xn, Q, N, P, D, combine, top_t, eps, select, (hipStream_t)stream}, scores);
}

// Per-query feature weights (include/skyemb.h): the `_sel` calls with w [Q, D] in place of xn.  select == NULL: every image.
extern "C" int skyemb_cosine_token_topk_pq(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *w, int Q,
                                           int64_t N, int P, int D, int k, int combine, int top_t, float eps, int64_t idx_offset,
                                           int nlists, const float *thr0, float *part_s, int64_t *part_i, const uint32_t *select,
                                           void *stream) {
    return token_topk({"skyemb_cosine_token_topk_pq", ANY_DTYPE, true, tw, qn, bank, bank_dtype, w, Q, N, P, D, combine, top_t, eps, select,
                       (hipStream_t)stream}, k, idx_offset, nlists, thr0, part_s, part_i);
}

extern "C" int skyemb_cosine_token_scores_pq(const float *tw, const float *qn, const void *bank, int bank_dtype, const float *w, int Q,
                                             int64_t N, int P, int D, int combine, int top_t, float eps, float *scores,
                                             const uint32_t *select, void *stream) {
    return token_scores({"skyemb_cosine_token_scores_pq", ANY_DTYPE, true, tw, qn, bank, bank_dtype, w, Q, N, P, D, combine, top_t, eps,
                         select, (hipStream_t)stream}, scores);
}

namespace {

// one byte per image -> the packed words: a wave's ballot is two words; images past N vote 0, which zeroes the padding bits
__global__ __launch_bounds__(256) void pack_select_kernel(const uint8_t *__restrict__ flags, int64_t N, uint32_t *__restrict__ words,
                                                          int64_t nwords) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long m = __ballot(i < N && flags[i] != 0);
    const int lane = threadIdx.x & 63;
    const int64_t w = i >> 5;
    if ((lane & 31) == 0 && w < nwords) words[w] = (uint32_t)(lane ? m >> 32 : m);
}

}  // namespace

extern "C" int skyemb_pack_select(const uint8_t *flags, int64_t N, uint32_t *words, void *stream) {
    SKY_CHECK_ARG(flags && words && N > 0, "skyemb_pack_select: bad arguments");
    SKY_CHECK_ARG(N < (1ll << 31), "skyemb_pack_select: N < 2^31 images");
    SKY_CHECK_ARG(((uintptr_t)words & 3) == 0, "skyemb_pack_select: words must be 4-byte aligned");
    const int64_t nwords = ceil_div64(N, 32);
    hipLaunchKernelGGL(pack_select_kernel, dim3((unsigned)ceil_div64(N, 256)), dim3(256), 0, (hipStream_t)stream, flags, N, words,
                       nwords);
    SKY_LAUNCH_CHECK("skyemb_pack_select");
    return 0;
}
