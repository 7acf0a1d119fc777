// Device pieces shared by the bank-streaming kernels (topk_stream.hip: one vector per row; topk_tokens.hip: P rows per image):
// the 16-row MFMA dot product fed straight from HBM, the A operand image, the score's last step and the wave-owned sorted list.
//
// Lane (n = lane&15, g = lane>>4) loads bank[row0+n][16c + 4g .. 4g+3] (fp32 rows; 16-bit rows: BankSet); the MFMA B operand of k-step m
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

// ---- 16-bit bank rows (bf16_t | f16_t): a half-precision bank IS the fp32 bank its elements widen to, so the chain above is fed
// the same operands in the same order from half the bytes.

// the two floats a 32-bit word of a 16-bit row widens to, exactly (lower address first)
template <typename T>
__device__ __forceinline__ void widen2(unsigned w, float &a, float &b);
template <>
__device__ __forceinline__ void widen2<bf16_t>(unsigned w, float &a, float &b) {
    a = __uint_as_float(w << 16);                 // bf16 is the upper half of the fp32 with the same value
    b = __uint_as_float(w & 0xffff0000u);
}
template <>
__device__ __forceinline__ void widen2<f16_t>(unsigned w, float &a, float &b) {
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
    const f16x2 h = __builtin_bit_cast(f16x2, w);
    a = (float)h[0];                              // v_cvt_f32_f16: exact, subnormals included, inf stays inf
    b = (float)h[1];
}

// elements of a row that one lane's 16-byte load covers: `src` of stream_dot16 = row + lane_elems<T>() * g
template <typename T>
__host__ __device__ constexpr int lane_elems() { return 16 / (int)sizeof(T); }

// One 16-byte load `r` of lane (n, g) = elements 32 c' + 8 g .. 8 g + 7 -> the MFMAs of the 32 elements 32 c' .. 32 c' + 31
// (A fragments a0 = imgA[2 c'], a1 = imgA[2 c' + 1]).  Widened, lo = elements 8 g .. 8 g + 3 and hi = 8 g + 4 .. 8 g + 7; after
// transpose4 component m of lo / hi is element 8 m + g / 8 m + 4 + g, so the order lo.x hi.x lo.y hi.y | lo.z hi.z lo.w hi.w
// walks the k-steps 4 m' + g, m' = 0 .. 7: the fp32 rows' d-ascending chain, A image unchanged, the same permlane swaps per
// element.
template <typename T>
__device__ __forceinline__ f32x4 mfma32_lp(f32x4 acc, const uint4 r, const float4 a0, const float4 a1) {
    float4 lo, hi;
    widen2<T>(r.x, lo.x, lo.y);
    widen2<T>(r.y, lo.z, lo.w);
    widen2<T>(r.z, hi.x, hi.y);
    widen2<T>(r.w, hi.z, hi.w);
    transpose4(lo);
    transpose4(hi);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, lo.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, hi.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, lo.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, hi.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, lo.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, hi.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, lo.w, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, hi.w, acc, 0, 0, 0);
    return acc;
}

// stream_dot16 for 16-bit rows (`src` = row + 8 g).  The same two register sets of 16 UNROLL = 64 elements each, i.e. LP_LOADS
// 16-byte loads per set (nchunk % UNROLL == 0 as above, so D = 64 and D = 192 work).
constexpr int LP_LOADS = UNROLL / 2;

template <typename T>
__device__ __forceinline__ f32x4 stream_dot16(const T *__restrict__ src, const float4 *__restrict__ imgA, int nchunk, int lane) {
    static_assert(sizeof(T) == 2, "16-bit bank rows");
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    uint4 b0[LP_LOADS], b1[LP_LOADS];
#pragma unroll
    for (int j = 0; j < LP_LOADS; ++j) b0[j] = *(const uint4 *)(src + 32 * j);
    for (int c0 = 0; c0 < nchunk; c0 += 2 * UNROLL) {
        const bool more1 = c0 + UNROLL < nchunk, more2 = c0 + 2 * UNROLL < nchunk;
        if (more1) {
#pragma unroll
            for (int j = 0; j < LP_LOADS; ++j) b1[j] = *(const uint4 *)(src + 16 * (c0 + UNROLL) + 32 * j);
        }
#pragma unroll
        for (int j = 0; j < LP_LOADS; ++j)
            acc = mfma32_lp<T>(acc, b0[j], imgA[(c0 + 2 * j) * 64 + lane], imgA[(c0 + 2 * j + 1) * 64 + lane]);
        if (more2) {
#pragma unroll
            for (int j = 0; j < LP_LOADS; ++j) b0[j] = *(const uint4 *)(src + 16 * (c0 + 2 * UNROLL) + 32 * j);
        }
        if (more1) {
#pragma unroll
            for (int j = 0; j < LP_LOADS; ++j)
                acc = mfma32_lp<T>(acc, b1[j], imgA[(c0 + UNROLL + 2 * j) * 64 + lane], imgA[(c0 + UNROLL + 2 * j + 1) * 64 + lane]);
        }
    }
    return acc;
}

// ---- per-query feature weights (PQW, the `_pq` entry points): next to the score chain a second chain over the same fragments,
// acc2[q][n] = fma(w[q][d], x2[n][d], acc2), x2[d] = x[d] * x[d] rounded once, same k-step order -- the squared weighted norm of
// bank row n under query q's own weights, in the score's C/D layout (lane (n, g) holds the queries 4 g + r).  imgW: the image of
// w [Q, D] in build_imgA's layout.

// one k-group of four MFMA steps on both chains; b is a transposed fragment (the score chain's B operand)
__device__ __forceinline__ void mfma4_pq(f32x4 &acc, f32x4 &acc2, const float4 a, const float4 w, const float4 b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, __fmul_rn(b.x, b.x), acc2, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, __fmul_rn(b.y, b.y), acc2, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, __fmul_rn(b.z, b.z), acc2, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, __fmul_rn(b.w, b.w), acc2, 0, 0, 0);
}

// stream_dot16 with the norm chain: the same loads, register sets and k-step order; returns the score chain, acc2 by reference
__device__ __forceinline__ f32x4 stream_dot16_pq(const float *__restrict__ src, const float4 *__restrict__ imgA,
                                                 const float4 *__restrict__ imgW, int nchunk, int lane, f32x4 &acc2) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc2 = acc;
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
            mfma4_pq(acc, acc2, imgA[(c0 + u) * 64 + lane], imgW[(c0 + u) * 64 + lane], b0[u]);
        }
        if (more2) {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) b0[u] = *(const float4 *)(src + 16 * (c0 + 2 * UNROLL + u));
        }
        if (more1) {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                transpose4(b1[u]);
                mfma4_pq(acc, acc2, imgA[(c0 + UNROLL + u) * 64 + lane], imgW[(c0 + UNROLL + u) * 64 + lane], b1[u]);
            }
        }
    }
    return acc;
}

// mfma32_lp with the norm chain: the widened, transposed halves in mfma32_lp's order lo.x hi.x lo.y hi.y | lo.z hi.z lo.w hi.w
template <typename T>
__device__ __forceinline__ void mfma32_lp_pq(f32x4 &acc, f32x4 &acc2, const uint4 r, const float4 a0, const float4 a1, const float4 w0,
                                             const float4 w1) {
    float4 lo, hi;
    widen2<T>(r.x, lo.x, lo.y);
    widen2<T>(r.y, lo.z, lo.w);
    widen2<T>(r.z, hi.x, hi.y);
    widen2<T>(r.w, hi.z, hi.w);
    transpose4(lo);
    transpose4(hi);
    mfma4_pq(acc, acc2, a0, w0, make_float4(lo.x, hi.x, lo.y, hi.y));
    mfma4_pq(acc, acc2, a1, w1, make_float4(lo.z, hi.z, lo.w, hi.w));
}

template <typename T>
__device__ __forceinline__ f32x4 stream_dot16_pq(const T *__restrict__ src, const float4 *__restrict__ imgA,
                                                 const float4 *__restrict__ imgW, int nchunk, int lane, f32x4 &acc2) {
    static_assert(sizeof(T) == 2, "16-bit bank rows");
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc2 = acc;
    uint4 b0[LP_LOADS], b1[LP_LOADS];
#pragma unroll
    for (int j = 0; j < LP_LOADS; ++j) b0[j] = *(const uint4 *)(src + 32 * j);
    for (int c0 = 0; c0 < nchunk; c0 += 2 * UNROLL) {
        const bool more1 = c0 + UNROLL < nchunk, more2 = c0 + 2 * UNROLL < nchunk;
        if (more1) {
#pragma unroll
            for (int j = 0; j < LP_LOADS; ++j) b1[j] = *(const uint4 *)(src + 16 * (c0 + UNROLL) + 32 * j);
        }
#pragma unroll
        for (int j = 0; j < LP_LOADS; ++j) {
            const int c = (c0 + 2 * j) * 64 + lane;
            mfma32_lp_pq<T>(acc, acc2, b0[j], imgA[c], imgA[c + 64], imgW[c], imgW[c + 64]);
        }
        if (more2) {
#pragma unroll
            for (int j = 0; j < LP_LOADS; ++j) b0[j] = *(const uint4 *)(src + 16 * (c0 + 2 * UNROLL) + 32 * j);
        }
        if (more1) {
#pragma unroll
            for (int j = 0; j < LP_LOADS; ++j) {
                const int c = (c0 + UNROLL + 2 * j) * 64 + lane;
                mfma32_lp_pq<T>(acc, acc2, b1[j], imgA[c], imgA[c + 64], imgW[c], imgW[c + 64]);
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
