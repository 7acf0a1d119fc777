// Device pieces shared by the bank-streaming kernels (topk_stream.hip: one vector per row; topk_tokens.hip: P rows per image):
// the 16-row MFMA dot product fed straight from HBM, the A operand image, the score's last step and the wave-owned sorted list.
//
// Lane (n = lane&15, g = lane>>4) loads bank[row0+n][16c + 4g .. 4g+3]; the MFMA B operand of k-step m
// must hold bank[row0+n][16c + 4m + g], i.e. the 4x4 transpose of (lane group g) x (element s):
// two v_permlane32_swap (lanes +-32) and two v_permlane16_swap (lanes +-16) per float4.
#pragma once
#include "common.h"

constexpr int UNROLL = 4;   // float4 loads per register set (2 sets: up to 8 KiB per wave in flight)

__device__ __forceinline__ float finish_score(float dot, float qn, float xn, float eps) {
    const float den = fmaf(qn, xn, eps);
    const float s = __fdiv_rn(dot, den);
    return s == s ? s : -INFINITY;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void swap32(float &lo_half_src, float &hi_half_dst) {
    // lanes 32-63 of `hi_half_dst` <-> lanes 0-31 of `lo_half_src`
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(hi_half_dst), __float_as_uint(lo_half_src), false, false);
    hi_half_dst = __uint_as_float(r[0]);
    lo_half_src = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap16(float &even_src, float &odd_dst) {
    // odd 16-lane rows of `odd_dst` <-> even 16-lane rows of `even_src`
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(odd_dst), __float_as_uint(even_src), false, false);
    odd_dst = __uint_as_float(r[0]);
    even_src = __uint_as_float(r[1]);
}

// v[s] of lane group g  ->  v[g'] ... transpose so that afterwards v[m] (group g) == old v[g] of group m
__device__ __forceinline__ void transpose4(float4 &v) {
    swap32(v.z, v.x);   // upper half's x <-> lower half's z
    swap32(v.w, v.y);   // upper half's y <-> lower half's w
    swap16(v.y, v.x);   // odd rows' x <-> even rows' y
    swap16(v.w, v.z);   // odd rows' z <-> even rows' w
}

// A operand image in LDS: entry [c][l] (lane l = (q = l & 15, g = l >> 4)) holds tw[q][16c + 4m + g], m = 0..3.  Every load of
// a thread's (up to four) entries is issued before the first LDS write: a load that feeds an LDS store straight away is waited
// for on the spot, and the image of 16 x 768 queries was twelve dependent memory round trips per workgroup.
template <int WAVES>
__device__ __forceinline__ void build_imgA(float4 *imgA, const float *__restrict__ tw, int Q, int D, int nchunk, int tid) {
    const int total = nchunk * 64;
    for (int e0 = tid; e0 < total; e0 += 4 * WAVES * 64) {
        float4 a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * WAVES * 64 < total ? e0 + u * WAVES * 64 : total - 1;
            const int c = e >> 6, l = e & 63, q = l & 15, g = l >> 4;
            const float *src = tw + (int64_t)(q < Q ? q : 0) * D + 16 * c + g;
            a[u] = make_float4(src[0], src[4], src[8], src[12]);
            if (q >= Q) a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * WAVES * 64;
            if (e < total) imgA[e] = a[u];
        }
    }
}

// dot products of 16 queries (A image in LDS) with the 16 bank rows this wave's lanes point at (`src` = row + 4 g): the
// contract's fp32 fma chain over d = 0, 1, 2, ... on v_mfma_f32_16x16x4_f32.  Two register sets (nchunk % UNROLL == 0 is
// checked on the host): the next group's loads are in flight while the current group feeds the MFMAs.
__device__ __forceinline__ f32x4 stream_dot16(const float *__restrict__ src, const float4 *__restrict__ imgA, int nchunk, int lane) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float4 b0[UNROLL], b1[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) b0[u] = *(const float4 *)(src + 16 * u);
    for (int c0 = 0; c0 < nchunk; c0 += 2 * UNROLL) {
        const bool more1 = c0 + UNROLL < nchunk, more2 = c0 + 2 * UNROLL < nchunk;
        if (more1) {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) b1[u] = *(const float4 *)(src + 16 * (c0 + UNROLL + u));
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            transpose4(b0[u]);
            const float4 a = imgA[(c0 + u) * 64 + lane];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0[u].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b0[u].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b0[u].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b0[u].w, acc, 0, 0, 0);
        }
        if (more2) {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) b0[u] = *(const float4 *)(src + 16 * (c0 + 2 * UNROLL + u));
        }
        if (more1) {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                transpose4(b1[u]);
                const float4 a = imgA[(c0 + UNROLL + u) * 64 + lane];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b1[u].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1[u].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b1[u].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b1[u].w, acc, 0, 0, 0);
            }
        }
    }
    return acc;
}

// Insert (cv, cidx) into a sorted list (scores descending) of nq <= k entries that ONE wavefront owns in LDS; returns the new
// size.  Caller guarantees cv > (nq == k ? lsq[k-1] : -inf).  Candidates arrive in ascending index order, so among equal
// scores the earlier (lower index) entry stays in front: order = (score desc, index asc).
__device__ __forceinline__ int stream_list_insert(float *lsq, int *liq, int nq, int k, float cv, int cidx, int lane) {
    int pos = 0;
    for (int e = lane; e < nq; e += 64) pos += lsq[e] >= cv ? 1 : 0;
    pos = wave_sum_i(pos);
    const int new_n = nq < k ? nq + 1 : k;
    for (int e0 = ((new_n - 1) / 64) * 64; e0 >= 0; e0 -= 64) {
        const int e = e0 + lane;
        const bool mv = e >= pos && e < new_n - 1;
        float sv = 0.f;
        int iv = 0;
        if (mv) { sv = lsq[e]; iv = liq[e]; }
        __builtin_amdgcn_wave_barrier();
        if (mv) { lsq[e + 1] = sv; liq[e + 1] = iv; }
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) {
        lsq[pos] = cv;
        liq[pos] = cidx;
    }
    __builtin_amdgcn_wave_barrier();
    return new_n;
}
