// Weighted MSE / MAE patch-token bank search for Q <= 16 queries (utils/similarity.py:174-212 + 214-268 with max_pool = False):
// the distance-metric twin of topk_tokens.hip.  Rows stream from HBM straight into registers, every token distance is a
// vector-ALU sum (|x - t| has no dot-product form, so no MFMA), the P token distances of an image are combined in registers and
// ONE candidate per image goes to the wave's private sorted lists.  No [Q, N * P] matrix reaches memory.
//
// Arithmetic contract (include/skyemb.h and tests/token_distance_reference.py state the same, word for word):
//   All arithmetic is fp32, every operation rounds to nearest even on its own, and there is no fused multiply-add anywhere in
//   the score (this file is compiled with floating-point contraction off).  With c = fp32(w / sum(w)) [D] prepared by the
//   caller, t [D] the query and x [D] a bank row (a 16-bit row is widened exactly on load):
//     term[d] = c[d] * v[d],  v[d] = |x[d] - t[d]| for MAE,  v[d] = (x[d] - t[d]) * (x[d] - t[d]) for MSE;
//     16 partial sums: p[j] = 0, then p[j] = p[j] + term[d] over the elements with (d >> 2) & 15 == j, in ascending d;
//     four folds: p[j] = p[j] + p[j ^ 8], then p[j] = p[j] + p[j ^ 4], then p[j] = p[j] + p[j ^ 2], then p[j] = p[j] + p[j ^ 1]
//     (every fold on all 16 partials at once; addition commutes, so afterwards all 16 are equal);
//     dist = p[0] / (float)D, one IEEE division.
//   The order does not depend on Q, launch geometry, wave, P, bank dtype, top_t or the selection.
//
// Layout: 16 lanes per bank row, lane j of a row loads the float4s 16 m + j (m = 0 .. D / 64 - 1) -- 256 contiguous bytes per row
// and step -- so lane j's running sum IS partial j and the folds are four DPP adds within a row of 16 lanes.  A wave holds four
// rows at a time (lane group h = lane >> 4); a 16-row tile is four such steps.  The row is loaded ONCE and scored against all Q
// queries (t [Q, D] sits in LDS, c comes through the vector cache: 4 D bytes that every wave re-reads), so HBM bytes per pass
// are the bank's, whatever Q is.  After the folds the tile's distances are moved to the cosine kernel's layout (lane (n, g) holds
// row n of the tile for the queries 4 g + r), and from there on the code is that kernel's.
//
// Ordering: smaller is better, so the kernel works on key = -dist (an exact negation; a NaN distance ranks as key -inf, i.e.
// distance +inf).  In key space the reference's combine of distances IS the cosine kernels' combine of scores, because negation
// commutes with every rounding: distance min = key MAX, distance max = key MIN, distance mean = key MEAN; "the top_t smallest
// distances" are the top_t largest keys.  So token_combine.h, the lists, thr0, ties (key desc, image asc), the (-inf, -1)
// terminator and skyemb_topk_merge apply unchanged.  The scores call writes -key: distances, +inf for a deselected image.
//
// Per-query feature weights (PQC, the `_pq` entry points): c is [Q, D], one row per query, staged in LDS behind t (another 4 Q D
// bytes); term[d] of query q takes c[q][d].  The contract above is otherwise untouched, so query q's result is bit-identical to
// the single-c call with that row.  LDS: 8 Q D <= 128 D for t and c, so these calls answer to skyemb_cosine_token_pq_applicable.
#include "topk_stream.h"
#include "token_combine.h"
#include "distance_chain.h"

#pragma clang fp contract(off)

namespace {

constexpr int DWAVES = 4;            // waves per workgroup: four waves' lists fit whenever skyemb_cosine_token_applicable says yes

// four consecutive elements of a bank row, widened exactly
template <typename T>
__device__ __forceinline__ float4 row4(const T *p);
template <>
__device__ __forceinline__ float4 row4<float>(const float *p) { return *(const float4 *)p; }
template <>
__device__ __forceinline__ float4 row4<bf16_t>(const bf16_t *p) {
    const uint2 w = *(const uint2 *)p;
    float4 v;
    widen2<bf16_t>(w.x, v.x, v.y);
    widen2<bf16_t>(w.y, v.z, v.w);
    return v;
}
template <>
__device__ __forceinline__ float4 row4<f16_t>(const f16_t *p) {
    const uint2 w = *(const uint2 *)p;
    float4 v;
    widen2<f16_t>(w.x, v.x, v.y);
    widen2<f16_t>(w.y, v.z, v.w);
    return v;
}

// (the chain's term, its folds and its division: distance_chain.h, shared with the two-stage MSE search's re-score)

// KCOMBINE is the combine in KEY space (see the head of this file); the other switches are cosine_token_kernel's.
// c [D] (PQC: [Q, D]), t [Q, D]; LDS: t, (PQC: c,) then [DWAVES][Q][k] list scores and [DWAVES][Q][k] list images.
template <typename T, int METRIC, int KCOMBINE, bool LISTS, bool TOPT, bool SEL, bool PQC>
__global__ __launch_bounds__(DWAVES * 64) void distance_token_kernel(const float *__restrict__ cw, const float *__restrict__ tq,
                                                                      const T *__restrict__ bank, int Q, int64_t R, int P, int D, int k,
                                                                      int64_t idx_offset, int64_t rows_per_wave,
                                                                      float *__restrict__ part_s, int64_t *__restrict__ part_i,
                                                                      const float *__restrict__ thr0, float *__restrict__ scores,
                                                                      int64_t n_img, int top_t, const uint32_t *__restrict__ sel) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nm = D >> 6, D4 = D >> 2;                             // float4 steps per lane and row; float4s per row
    float4 *t4 = (float4 *)lds;                                     // [Q][D / 4]
    const float4 *c4 = t4 + (size_t)Q * D4;                         // PQC: [Q][D / 4]
    float *ls_all = lds + (size_t)Q * D * (PQC ? 2 : 1);            // [DWAVES][Q][k]
    int *li_all = (int *)(ls_all + (size_t)DWAVES * Q * k);         // [DWAVES][Q][k]
    for (int e = tid; e < Q * D4; e += DWAVES * 64) t4[e] = ((const float4 *)tq)[e];
    if (PQC)
        for (int e = tid; e < Q * D4; e += DWAVES * 64) t4[Q * D4 + e] = ((const float4 *)cw)[e];
    __syncthreads();
    float *ls = ls_all + (size_t)wave * Q * k;
    int *li = li_all + (size_t)wave * Q * k;
    const int wid = blockIdx.x * DWAVES + wave;
    const int64_t r_begin = (int64_t)wid * rows_per_wave;           // a multiple of lcm(P, 16): the first row of an image
    int64_t r_end = r_begin + rows_per_wave;
    if (r_end > R) r_end = R;                                       // R = images x P: whole images only
    const int n_lane = lane & 15, g = lane >> 4;
    const int tp = P < 16 ? P : 16;                                 // lanes of one image in a tile
    const int tiles_per_image = P < 16 ? 1 : P >> 4;
    int n_in[16];
    float thr[16], floor_thr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        n_in[q] = 0;
        thr[q] = (LISTS && thr0 && q < Q) ? thr0[q] : -INFINITY;
        floor_thr[q] = thr[q];                                      // valid lower bound of the global k-th best key (or -inf)
    }
    float carry[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) carry[r] = combine_start<KCOMBINE>();
    const float fP = (float)P, fD = (float)D;
    int tile_in_image = 0;
    const int lg_tp = __builtin_ctz(tp);
    unsigned sel_img = SEL ? (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)r_begin / (unsigned)P)) : 0u;
    unsigned sel_word = 0;
    int sel_word_at = -1;
    const int from_lane = 16 * (n_lane & 3) + n_lane;               // a lane of the row group that scored this lane's row of the tile

    for (int64_t n0 = r_begin; n0 < r_end; n0 += 16) {
        bool on_lane = true;                                        // SEL: this lane's image is selected
        if (SEL && (P < 16 || tile_in_image == 0)) {                // 16 | P: the first tile of an image decides for all of them
            const unsigned img0 = sel_img;                          // the tile's first image (< n_img: n0 < r_end <= R), a scalar
            sel_img += P < 16 ? 16u >> lg_tp : 1u;
            if ((int)(img0 >> 5) != sel_word_at) {                  // one load per 32 images, made scalar
                sel_word_at = (int)(img0 >> 5);
                sel_word = (unsigned)__builtin_amdgcn_readfirstlane((int)sel[sel_word_at]);
            }
            if (P >= 16) {
                if (!((sel_word >> (img0 & 31)) & 1u)) {            // the whole wave passes the image over: no row of it is loaded
                    if (!LISTS && lane < Q) scores[(int64_t)lane * n_img + img0] = INFINITY;
                    n0 += P - 16;
                    continue;
                }
            } else {
                const int ipt = 16 >> lg_tp;                        // images per tile; their bits lie in one word
                const unsigned bits = (sel_word >> (img0 & 31)) & (0xffffu >> (16 - ipt));
                if (bits == 0) {                                    // no image of this tile is selected
                    if (!LISTS)
                        for (int e = lane; e < ipt * Q; e += 64) {
                            const int64_t img = (int64_t)img0 + (e & (ipt - 1));
                            if (img < n_img) scores[(int64_t)(e >> (4 - lg_tp)) * n_img + img] = INFINITY;
                        }
                    continue;
                }
                on_lane = (bits >> (n_lane >> lg_tp)) & 1u;
            }
        }
        // keys of the tile: key[r] of lane (n, g) = -dist(row n0 + n, query 4 g + r).  The tile's 4 nm float4 loads per lane run
        // as nm blocks of four (all four in flight before the first is used); (s, m) = (row step, float4 step) of an element.
        float key[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        float p[16];
        int s = 0, m = 0;
        for (int b = 0; b < nm; ++b) {
            float4 xv[4], cv4[4];
            int ls_ = s, lm = m;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int64_t row = n0 + 4 * ls_ + g;
                if (row >= r_end) row = r_end - 1;                  // clamp: masked below
                xv[u] = row4<T>(bank + row * D + 64 * lm + 4 * n_lane);
                if (!PQC) cv4[u] = *(const float4 *)(cw + 64 * lm + 4 * n_lane);
                if (++lm == nm) { lm = 0; ++ls_; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (m == 0) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) p[q] = 0.f;
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    if (q < Q) {                                    // wave-uniform
                        const float4 tv = t4[q * D4 + 16 * m + n_lane];
                        const float4 cv = PQC ? c4[q * D4 + 16 * m + n_lane] : cv4[u];
                        p[q] = dist_term<METRIC>(p[q], xv[u].x, tv.x, cv.x);
                        p[q] = dist_term<METRIC>(p[q], xv[u].y, tv.y, cv.y);
                        p[q] = dist_term<METRIC>(p[q], xv[u].z, tv.z, cv.z);
                        p[q] = dist_term<METRIC>(p[q], xv[u].w, tv.w, cv.w);
                    }
                }
                if (++m == nm) {                                    // rows n0 + 4 s + g are complete: fold, divide, hand over
                    m = 0;
                    const bool row_ok = n0 + 4 * s + g < r_end;
                    const bool mine = (n_lane >> 2) == s;           // this lane's row of the tile was scored in this step
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        if (q >= Q) continue;                       // wave-uniform
                        const float dist = dist_finish(dist_fold_lanes(p[q]), fD);
                        const float kq = (row_ok && dist == dist) ? -dist : -INFINITY;
                        const float got = __shfl(kq, from_lane, 64);
                        if (mine && g == (q >> 2)) key[q & 3] = got;
                    }
                    ++s;
                }
            }
        }
        const bool row_ok = n0 + n_lane < r_end;
        const bool first_tile = tile_in_image == 0;
        const bool last_tile = ++tile_in_image == tiles_per_image;
        if (last_tile) tile_in_image = 0;
        // the image's first lane speaks for it (a row past r_end belongs to an image past r_end)
        const bool lead = last_tile && (n_lane & (tp - 1)) == 0 && row_ok;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q_mine = 4 * g + r;
            const float sc = (row_ok && q_mine < Q) ? key[r] : -INFINITY;
            float c;
            if (TOPT) {
                carry[r] = top_tile(sc, carry[r], n_lane, tp, first_tile);
                c = last_tile ? top_finish<KCOMBINE>(carry[r], lane, tp, top_t) : -INFINITY;   // wave-uniform
            } else {
                c = combine_tile<KCOMBINE>(sc, carry[r], lane, tp);
                carry[r] = last_tile ? combine_start<KCOMBINE>() : c;
                if (KCOMBINE == SKYEMB_COMBINE_MEAN && last_tile) {      // wave-uniform: the sum is complete
                    c = __fdiv_rn(c, fP);
                    c = c == c ? c : -INFINITY;
                }
            }
            if (!LISTS) {
                if (SEL && !on_lane) c = -INFINITY;
                if (lead && q_mine < Q) scores[(int64_t)q_mine * n_img + (int64_t)((unsigned)(n0 + n_lane) / (unsigned)P)] = -c;
                continue;
            }
            // candidates of the 4 queries {r, 4+r, 8+r, 12+r} (one per lane group), images ascending within a group
            float my_thr = -INFINITY;
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) my_thr = (g == gg) ? thr[4 * gg + r] : my_thr;
            unsigned long long mk = __ballot(lead && (!SEL || on_lane) && q_mine < Q && c > my_thr);
            while (mk) {
                const int srcl = __builtin_ctzll(mk);
                mk &= mk - 1;
                const float cv = __shfl(c, srcl, 64);
                const int q = 4 * (srcl >> 4) + r;
                float *lsq = ls + q * k;
                int *liq = li + q * k;
                int nq = 0;
                float tqv = -INFINITY;
#pragma unroll
                for (int gg = 0; gg < 4; ++gg)
                    if (q == 4 * gg + r) { nq = n_in[4 * gg + r]; tqv = thr[4 * gg + r]; }
                if (!(cv > tqv)) continue;
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
    // this wave's lists: part[q][wid][k], the entries and ONE terminator (-inf, -1), as cosine_token_kernel writes them
    const int nlists = gridDim.x * DWAVES;
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

struct Launch {
    int blocks;
    size_t smem;
    hipStream_t st;
    const char *who;
    const float *cw, *tq;
    int Q;
    int64_t R;
    int P, D, k;
    int64_t idx_offset, rows_per_wave;
    float *part_s;
    int64_t *part_i;
    const float *thr0;
    float *scores;
    int64_t n_img;
    int top_t;
    const uint32_t *sel;
    bool pq;                                                        // c is [Q, D]
};

template <typename T, int METRIC, bool LISTS, bool SEL, bool PQC>
int launch_pq(const Launch &a, const T *bank, int combine) {
    auto go = [&](auto kern) {
        if (a.smem > 64 * 1024) {
            const int rc = sky_set_lds_limit((const void *)kern, LDS_BYTES, a.who);
            if (rc != 0) return rc;
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)a.blocks), dim3(DWAVES * 64), a.smem, a.st, a.cw, a.tq, bank, a.Q, a.R, a.P, a.D, a.k,
                           a.idx_offset, a.rows_per_wave, a.part_s, a.part_i, a.thr0, a.scores, a.n_img, a.top_t, a.sel);
        SKY_LAUNCH_CHECK(a.who);
        return 0;
    };
    // distance -> key space: min = key MAX (a[0] for every top_t: the plain kernel), max = key MIN, mean = key MEAN
    if (combine == SKYEMB_COMBINE_MIN) return go(distance_token_kernel<T, METRIC, SKYEMB_COMBINE_MAX, LISTS, false, SEL, PQC>);
    if (a.top_t != 0 && combine == SKYEMB_COMBINE_MAX) return go(distance_token_kernel<T, METRIC, SKYEMB_COMBINE_MIN, LISTS, true, SEL, PQC>);
    if (a.top_t != 0) return go(distance_token_kernel<T, METRIC, SKYEMB_COMBINE_MEAN, LISTS, true, SEL, PQC>);
    if (combine == SKYEMB_COMBINE_MAX) return go(distance_token_kernel<T, METRIC, SKYEMB_COMBINE_MIN, LISTS, false, SEL, PQC>);
    return go(distance_token_kernel<T, METRIC, SKYEMB_COMBINE_MEAN, LISTS, false, SEL, PQC>);
}

template <typename T, int METRIC, bool LISTS, bool SEL>
int launch_sel(const Launch &a, const T *bank, int combine) {
    return a.pq ? launch_pq<T, METRIC, LISTS, SEL, true>(a, bank, combine) : launch_pq<T, METRIC, LISTS, SEL, false>(a, bank, combine);
}

template <bool LISTS, typename T>
int launch_typed(const Launch &a, const T *bank, int metric, int combine) {
    if (metric == SKYEMB_METRIC_MSE)
        return a.sel ? launch_sel<T, SKYEMB_METRIC_MSE, LISTS, true>(a, bank, combine)
                     : launch_sel<T, SKYEMB_METRIC_MSE, LISTS, false>(a, bank, combine);
    return a.sel ? launch_sel<T, SKYEMB_METRIC_MAE, LISTS, true>(a, bank, combine)
                 : launch_sel<T, SKYEMB_METRIC_MAE, LISTS, false>(a, bank, combine);
}

// the refusals both calls share; every one of them comes before any launch
// (pq: c is [Q, D] and sits in LDS with t, which the rule with two images covers)
int check_common(const char *who, const void *c, const void *t, const void *bank, int bank_dtype, int Q, int64_t N, int P, int D, int k,
                 int metric, int combine, int top_t, const void *out, const uint32_t *select, bool pq = false) {
    SKY_CHECK_ARG(c && t && bank && out && N > 0, "%s: bad arguments", who);
    SKY_CHECK_ARG(bank_dtype == SKYEMB_F32 || sky_is_lp(bank_dtype),
                  "%s: bank_dtype must be SKYEMB_BF16 (0), SKYEMB_F32 (1) or SKYEMB_F16 (2), got %d", who, bank_dtype);
    SKY_CHECK_ARG(metric == SKYEMB_METRIC_MSE || metric == SKYEMB_METRIC_MAE,
                  "%s: metric must be SKYEMB_METRIC_MSE (1) or SKYEMB_METRIC_MAE (2), got %d", who, metric);
    SKY_CHECK_ARG(combine == SKYEMB_COMBINE_MIN || combine == SKYEMB_COMBINE_MEAN || combine == SKYEMB_COMBINE_MAX,
                  "%s: unknown combine code %d", who, combine);
    if (!(pq ? skyemb_cosine_token_pq_applicable(Q, P, D, k) : skyemb_cosine_token_applicable(Q, P, D, k))) {   // its text names the limits; prefix the caller
        char why[512];
        snprintf(why, sizeof why, "%s", skyemb_last_error());
        skyemb_set_error("%s: %s", who, why);
        return 1;
    }
    SKY_CHECK_ARG(top_t >= 0 && top_t <= (P < 16 ? P : 16), "%s: top_t must be 0 (all tokens) or 1 .. min(P, 16) (top_t=%d P=%d)", who,
                  top_t, P);
    SKY_CHECK_ARG(N * P < (1ll << 31), "%s: bank too large (N * P < 2^31 rows per call)", who);
    SKY_CHECK_ARG(aligned16(bank) && aligned16(c) && aligned16(t), "%s: bank, c and t must be 16-byte aligned", who);
    SKY_CHECK_ARG(((uintptr_t)select & 3) == 0, "%s: select must be 4-byte aligned", who);
    return 0;
}

// the two calls; pq: c is [Q, D] (the `_pq` entry points)
int distance_topk(const char *who, bool pq, const float *c, const float *t, const void *bank, int bank_dtype, int Q, int64_t N, int P, int D,
                  int metric, int combine, int top_t, int k, int64_t idx_offset, int nlists, const float *thr0, float *part_s,
                  int64_t *part_i, const uint32_t *select, void *stream) {
    if (check_common(who, c, t, bank, bank_dtype, Q, N, P, D, k, metric, combine, top_t, part_s, select, pq)) return 1;
    SKY_CHECK_ARG(part_i, "%s: bad arguments", who);
    SKY_CHECK_ARG(nlists == skyemb_cosine_token_topk_chunks(N, P, Q, D, k), "%s: nlists must come from skyemb_cosine_token_topk_chunks",
                  who);
    // nlists is a multiple of 4 (blocks x 4 or 8 waves); 4 Q D <= 64 D, so four waves' lists fit under the cosine search's LDS rule
    // (pq: 8 Q D <= 128 D under the rule with two images)
    const int64_t R = N * P;
    const Launch a = {nlists / DWAVES, (size_t)4 * Q * D * (pq ? 2 : 1) + (size_t)2 * 4 * DWAVES * Q * k, (hipStream_t)stream, who, c, t, Q, R,
                      P, D, k, idx_offset, token_rows_per_wave(R, nlists, P), part_s, part_i, thr0, nullptr, N, top_t, select, pq};
    return with_bank_type(bank, bank_dtype, [&](auto *b) { return launch_typed<true>(a, b, metric, combine); });
}

int distance_scores(const char *who, bool pq, const float *c, const float *t, const void *bank, int bank_dtype, int Q, int64_t N, int P,
                    int D, int metric, int combine, int top_t, float *scores, const uint32_t *select, void *stream) {
    if (check_common(who, c, t, bank, bank_dtype, Q, N, P, D, 1, metric, combine, top_t, scores, select, pq)) return 1;
    const int64_t R = N * P, blocks = token_scores_blocks(R, P);    // workgroups of DWAVES = 4 waves
    const Launch a = {(int)blocks, (size_t)4 * Q * D * (pq ? 2 : 1), (hipStream_t)stream, who, c, t, Q, R, P, D, 1, 0,
                      token_rows_per_wave(R, blocks * DWAVES, P), nullptr, nullptr, nullptr, scores, N, top_t, select, pq};
    return with_bank_type(bank, bank_dtype, [&](auto *b) { return launch_typed<false>(a, b, metric, combine); });
}

}  // namespace

extern "C" int skyemb_distance_token_topk(const float *c, const float *t, const void *bank, int bank_dtype, int Q, int64_t N, int P,
                                          int D, int metric, int combine, int top_t, int k, int64_t idx_offset, int nlists,
                                          const float *thr0, float *part_s, int64_t *part_i, const uint32_t *select, void *stream) {
    return distance_topk("skyemb_distance_token_topk", false, c, t, bank, bank_dtype, Q, N, P, D, metric, combine, top_t, k, idx_offset,
                         nlists, thr0, part_s, part_i, select, stream);
}

extern "C" int skyemb_distance_token_scores(const float *c, const float *t, const void *bank, int bank_dtype, int Q, int64_t N, int P,
                                            int D, int metric, int combine, int top_t, float *scores, const uint32_t *select,
                                            void *stream) {
    return distance_scores("skyemb_distance_token_scores", false, c, t, bank, bank_dtype, Q, N, P, D, metric, combine, top_t, scores, select,
                           stream);
}

// Per-query feature weights (include/skyemb.h): the same two calls with c [Q, D], row q for query q.
extern "C" int skyemb_distance_token_topk_pq(const float *c, const float *t, const void *bank, int bank_dtype, int Q, int64_t N, int P,
                                             int D, int metric, int combine, int top_t, int k, int64_t idx_offset, int nlists,
                                             const float *thr0, float *part_s, int64_t *part_i, const uint32_t *select, void *stream) {
    return distance_topk("skyemb_distance_token_topk_pq", true, c, t, bank, bank_dtype, Q, N, P, D, metric, combine, top_t, k, idx_offset,
                         nlists, thr0, part_s, part_i, select, stream);
}

extern "C" int skyemb_distance_token_scores_pq(const float *c, const float *t, const void *bank, int bank_dtype, int Q, int64_t N, int P,
                                               int D, int metric, int combine, int top_t, float *scores, const uint32_t *select,
                                               void *stream) {
    return distance_scores("skyemb_distance_token_scores_pq", true, c, t, bank, bank_dtype, Q, N, P, D, metric, combine, top_t, scores,
                           select, stream);
}
