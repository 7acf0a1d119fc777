// The arithmetic chain of the weighted MSE / MAE distance contract (include/skyemb.h, "weighted MSE / MAE"), stated once for the
// kernels that score by it: distance_tokens.hip (16 lanes per row, lane j holds partial j) and the two-stage MSE search's re-score
// in topk_prefilter.hip (one lane per row, all 16 partials in its registers).  The contract has no fused multiply-add: every
// function body here switches floating-point contraction off for itself (the setting travels with the instructions when they are
// inlined), so the including file's own setting does not matter.
#pragma once
#include "token_combine.h"

// p = p + c * v(x - t): sub, abs or square, times c, add -- four roundings (abs is exact), no fma
template <int METRIC>
__device__ __forceinline__ float dist_term(float p, float x, float t, float c) {
#pragma clang fp contract(off)
    const float d = __fsub_rn(x, t);
    const float v = METRIC == SKYEMB_METRIC_MSE ? __fmul_rn(d, d) : fabsf(d);
    return __fadd_rn(p, __fmul_rn(c, v));
}

// the four folds with partial j in lane j of a 16-lane row: afterwards every lane holds p[0]
__device__ __forceinline__ float dist_fold_lanes(float v) {
#pragma clang fp contract(off)
    v = __fadd_rn(v, lane_xor(v, 8));
    v = __fadd_rn(v, lane_xor(v, 4));
    v = __fadd_rn(v, lane_xor(v, 2));
    v = __fadd_rn(v, lane_xor(v, 1));
    return v;
}

// the one division
__device__ __forceinline__ float dist_finish(float p0, float fD) { return __fdiv_rn(p0, fD); }

// The whole chain in one lane: x4(d) -> the row's elements d .. d + 3 widened, t and c [D] (16-byte aligned, D % 4 == 0).  Partial j
// takes the elements with (d >> 2) & 15 == j in ascending d; a fold adds p[j ^ m] to p[j] for all j at once, so p[j] and p[j ^ m]
// end equal and only the lower half is carried on (addition commutes: lane j's p[j] + p[j ^ 8] is this p[j] + p[j + 8]).
template <int METRIC, typename Row4>
__device__ __forceinline__ float dist_row_serial(Row4 x4, const float *__restrict__ t, const float *__restrict__ c, int D) {
#pragma clang fp contract(off)
    float p[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) p[j] = 0.f;
    for (int d0 = 0; d0 < D; d0 += 64) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int d = d0 + 4 * j;
            if (d < D) {
                const float4 xv = x4(d), tv = *(const float4 *)(t + d), cv = *(const float4 *)(c + d);
                p[j] = dist_term<METRIC>(p[j], xv.x, tv.x, cv.x);
                p[j] = dist_term<METRIC>(p[j], xv.y, tv.y, cv.y);
                p[j] = dist_term<METRIC>(p[j], xv.z, tv.z, cv.z);
                p[j] = dist_term<METRIC>(p[j], xv.w, tv.w, cv.w);
            }
        }
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1)
#pragma unroll
        for (int j = 0; j < m; ++j) p[j] = __fadd_rn(p[j], p[j + m]);
    return dist_finish(p[0], (float)D);
}
