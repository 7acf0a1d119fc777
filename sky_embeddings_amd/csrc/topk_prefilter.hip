// Many-query weighted-cosine top-k in two stages (utils/similarity.py:18-35,149-172; contract: oracle/topk_oracle.c):
//
//   stage 1 (prefilter)  approximate dot products on the fp16 matrix cores with a PROVEN error bound,
//                        every (query, row) pair whose score could still reach the query's top-k is appended to
//                        the query's candidate list;
//   stage 2 (exact)      the few survivors are re-scored with the contract's fp32 fma chain and ordered
//                        (score desc, index asc): the result is bit-identical to the exact kernel's.
//
// The exact-fp32 kernel (topk.hip) is bound by the fp32 matrix rate (157 TFLOP/s: 15.4 TFLOP at Q = 10k over 1M x 768);
// fp16 operands run 16x faster per MFMA and halve the bank bytes.
//
// Arithmetic of stage 1.  Row i of the bank is stored as x^_i = fp16(x_i * 2^-e_i) (e_i puts the row maximum in
// [2^13, 2^14)); the weighted query tw_q = w * t_q as q' = tw_q * 2^-f_q split into qh = fp16(q'), ql = fp16(q' - qh).
//   dot^ = sum_d (qh_d + ql_d) * x^_d          two v_mfma_f32_16x16x32_f16 passes into one fp32 accumulator
// Products of two fp16 numbers are exact in fp32.  Against the contract's chain dot' = chain(tw, x) * 2^-(e+f):
//   |dot^ - dot'| <= eps_a * ||q'||_2 * ||x'||_2,
//   eps_a = 2^-11 (fp16 rounding of x', relative) + 2^-21 (residual of the query split and the cross term)
//         + 6.06 * D * 2^-24 (fp32 accumulation of 2D products in any order, priced at one ulp each in case the matrix
//           core truncates, + the chain's own D roundings)
//         + 2 * sqrt(D) * 2^-27 (fp16 subnormals of either operand, even if the matrix core flushes them to zero: absolute
//           errors <= 2^-14 per element, expressed through the row / query maxima >= 2^13).
// With den = fmaf(qn, xn, eps) > 0 the exact score e = dot' * 2^(e+f) / den therefore lies in
//   [L, U] = (dot^ -+ eps_a ||q'|| ||x'||) * 2^(e+f) / den   (widened by 2^-22 relative for the divisions).
// A threshold tau_q that is a lower bound of the query's true k-th best exact score makes "U >= tau_q" a necessary
// condition for membership in the top-k.  tau_q is the k-th largest L over the candidates found so far -- real rows, so
// always a valid bound -- and is refreshed between the phases of the pass (bank slices of 1/32, 3/32, 12/32, 16/32 of
// the tiles after a first slice that takes everything): the candidate lists stay at a few hundred entries per query.
// At the end the K' candidates with the largest U are re-scored exactly; the answer is accepted when its k-th best
// exact score beats the U of every candidate that was NOT re-scored, otherwise the query is flagged and the caller
// runs it through the exact kernel (never observed on embedding-like data; forced in the tests).
//
// Resident fp16 bank (skyemb_bank16_rowp_lp / skyemb_cosine_topk_prefiltered_lp).  The bank IS the fp32 bank its elements
// widen to, so stage 1 multiplies the stored rows themselves: x^_i = x_i exactly, e_i = 0, no image is written.  Against
// dot' = chain(tw, x) * 2^-f the bound keeps its shape, |dot^ - dot'| <= eps_a * ||q'||_2 * ||x||_2 + s_i, with
//   eps_a = 2^-11 + 2^-21 (hi only: the query's own fp16 rounding, relative; no cross term -- the other factor is exact)
//           or 2^-21 (hi + lo: the residual q' - qh - ql is <= 2^-22 |q'| per element)
//         + 6.06 * D * 2^-24 (accumulation, as above: no more products, no more roundings)
//         + sqrt(D) * 2^-27 (fp16 subnormals of the QUERY operand, absolute <= 2^-14 per element against a query maximum
//           >= 2^13; the row side's share of that term is gone with the scaling it relied on)
//   s_i   = ||q'||_2 * sqrt(nsub_i) * 2^-14: row i has nsub_i fp16-subnormal elements (0 < |x| < 2^-14, not rescaled any
//           more).  If the matrix core flushes them the products q'_d x_d of those d are lost: Cauchy-Schwarz over them.
//           Nothing is assumed about whether it does.
// s_i rides in the row's norm slot: rowp[i] = {xn_i, nx_i, 1, 0} with nx_i = ||x_i||_2 (1 + D 2^-22) + sqrt(nsub_i) 2^-14 /
// eps_a, rounded up -- the slot multiplies eps_a ||q'||.  The row constants are built once and serve both variants, so
// the division uses the SMALLER eps_a (hi + lo): under hi only the term comes out larger than needed, never smaller.
// Whole tiles of BT rows are read straight from the bank; the last N % BT rows are served from a zero-padded copy of one
// tile (a launch of its own, so no read ever passes the bank's N * D elements).  Stage 2 widens the selected rows
// element by element into the same fma chain: the scores are those of the fp32 kernel on the widened bank, bit for bit.
//
// Resident bf16 bank (skyemb_resident_rowp / skyemb_cosine_topk_prefiltered_resident with SKYEMB_BF16).  The same construction on
// v_mfma_f32_16x16x32_bf16: x^_i = x_i exactly, e_i = 0, and the query split is qh = bf16(q'), ql = bf16(q' - qh).  The product of
// two bf16 numbers (8-bit significands) is exact in fp32 whenever it is a normal number.  bf16 has fp32's exponent range, so the
// query's scale is chosen for the fp32 ACCUMULATOR, not for the operand format: q' = tw_q 2^-f with the largest |q'_d| in
// [2^-21, 2^-20).  Overflow: |qh_d + ql_d| < 2^-20 (1 + 2^-8) and |x_d| < 2^128, so the 2 D <= 2^13 products and every partial sum of
// them stay below 2^121.1 -- no finite row overflows the accumulator, and a row the bound gives up on still has a finite dot^ (its
// test below then passes for every query; a NaN dot^ would drop it).  Against dot' = chain(tw, x) 2^-f:
//   |dot^ - dot'| <= eps_a ||q'||_2 ||x||_2,     eps_a = 2^-9 (hi only) or 2^-18 (hi + lo) + 6.06 D 2^-24 + D 2^-38
//   2^-9 / 2^-18   bf16 rounds to nearest even with 8 significant bits: |q'_d - qh_d| <= 2^-9 |q'_d|; r_d = q'_d - qh_d is exact in fp32
//                  (a multiple of ulp(q'_d) below 2^24 of them) and |r_d - ql_d| <= 2^-9 |r_d| <= 2^-18 |q'_d|.  Cauchy-Schwarz over d.
//                  (fp16's hi only: 2^-11, hi + lo: 2^-22.  At D = 768: 2.23e-3 and 2.81e-4, against 7.7e-4 for resident fp16 hi only.)
//   6.06 D 2^-24   the accumulation of the 2 D products in any order at one ulp each, the chain's own D roundings, and the factor
//                  1 + 2^-8 by which sum |qh_d + ql_d| |x_d| may exceed sum |q'_d| |x_d|: 5.02 D 2^-24 before the second-order terms.
//   D 2^-38        everything that happens below 2^-126, where nothing is assumed about the matrix core -- it may flush bf16-subnormal
//                  operands, products and partial sums to zero or round them -- under TWO conditions that the kernels enforce:
//                    (R) every nonzero element of the row has 2^-60 <= |x_d|, so ||x|| >= 2^-60 (or the row is zero: dot^ = dot' = 0);
//                    (Q) the query's scale 2^-f is below 2^30 (largest |tw_d| >= 2^-50), and ||q'|| >= 2^-21 by construction.
//                  (a) a product or a partial sum below 2^-126 lost or rounded: <= 2^-126 each, 4 D of them: D 2^-124 <=
//                      D 2^-43 ||q'|| ||x||.  (b) a query operand below 2^-126 flushed, or q'_d itself an fp32 subnormal after the
//                      scaling: <= 2^-126 |x_d| per product, in all <= 2^-125 sqrt(D) ||x|| <= sqrt(D) 2^-104 ||q'|| ||x|| -- the
//                      counterpart of the fp16 bound's query-subnormal term sqrt(D) 2^-27, 2^77 times smaller because bf16 operands
//                      underflow at 2^-126, not at 2^-24: it is kept, and it vanishes in the sum.  Row operands are never subnormal: (R).
//                      (c) the contract's chain rounds a subnormal partial sum by <= 2^-150, D times, and dot' carries that times
//                      2^-f: <= D 2^-120 <= D 2^-39 ||q'|| ||x||.  (a) + (b) + (c) < D 2^-38.
// There is NO additive row term: what the fp16 bound carries in the norm slot is kept out by (R) instead.  Row constants
// (bankbf16_rowp_kernel): rowp[i] = {xn_i, nx_i, 1, 0}, nx_i = ||x_i||_2 (1 + D 2^-22) rounded up, taken of the row scaled by a power
// of two (the squares leave fp32's range on both sides).  A row is UNBOUNDABLE and takes {0, inf, 1, 0} -- a candidate of every
// query, decided by stage 2 -- when it has an inf / NaN element (as ever), a nonzero element below 2^-60 (R), an element at or
// above 2^120 (nx and eps_a ||q'|| nx must stay finite; far below that, from about 2^64 on, the next rule has already caught it), or
// a weighted norm xn_i that is not finite: then a xn_i of the test is inf or NaN whatever tau is, while the row's exact score is
// +-0 and can belong to a top-k that reaches down to zero.  A query outside (Q), or whose scale had to be clamped at 2^-100 (largest
// |tw_d| >= 2^79), is flagged by init_state_kernel and re-run by the caller; its dot^ are never trusted.  Nothing else changes:
// same bytes, same tiles, ring, swizzle, candidate test, lists, phases, selection handling, tail tile; stage 2 widens bf16 rows.
#include "common.h"
#include "prefilter_plan.h"
#include "token_combine.h"
#include "distance_chain.h"
#include <array>
#include <math.h>
#include <stdlib.h>
#include <utility>

namespace {

typedef _Float16 half_t;
typedef __attribute__((ext_vector_type(8))) _Float16 half8;
typedef __attribute__((address_space(1))) const void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;

constexpr int BT = 256, BK = 32, NW = 8, NT = NW * 64;   // bank rows per tile, k-step, waves
// queries per tile: 256 with one fp16 pass (hi), 128 with two (hi + lo) -- 16 KiB of query rows per k-step either way, but the
// 256 x 256 tile does twice the products per byte brought into LDS (the LDS-DMA rate, not the matrix cores, bounds the kernel)
constexpr int qtile(bool lo) { return lo ? 128 : 256; }
constexpr int QPAD = 256;                                // every per-query array is padded to this many rows
constexpr int B_BYTES = BT * BK * 2, Q_BYTES = 256 * BK * 2;
constexpr int stage_bytes(bool) { return Q_BYTES + B_BYTES; }            // query rows (hi, or hi + lo) + bank rows = 32 KiB
constexpr int pieces(bool) { return (Q_BYTES + B_BYTES) / 1024 / NW; }   // LDS-DMA instructions per wave per stage (one = 16 rows x 64 B)
constexpr int NSTAGE = 4, AHEAD = NSTAGE - 1;   // 96 KiB of LDS-DMA in flight per CU: one workgroup per CU has to cover the
                                                 // L2 latency alone (a 2 x 64 KiB ring ran at 23 GB/s per CU: 2.8 us per k-step);
                                                 // NSTAGE is a power of two: stage s lives in buffer s & (NSTAGE - 1)
constexpr int GQ = 5;                     // query tiles (hi + lo = 384 KiB each at D = 768) kept hot in an XCD's L2
constexpr int RESCORE_MAX = 256;          // K': candidates re-scored exactly per query
constexpr int SCAP = 2048;                // candidates of one item staged in LDS (8 bytes each)
constexpr int PF_GRID = 256;              // persistent workgroups of the stage-1 launch (one per CU)

__device__ __forceinline__ void glds16(const void *src, char *lds_wave_base) {
    __builtin_amdgcn_global_load_lds((gvoid_t *)src, (lvoid_t *)lds_wave_base, 16, 0, 0);
}

// lo: the query enters as hi + lo (see the header); without lo its own fp16 rounding (2^-11 relative, + the cross term) joins
// the row's
// resident: the rows are a resident fp16 bank, exact in stage 1 (file header): their 2^-11 and their half of the subnormal term go
// (prefilter_plan.h's eps_of restates this, eps_a_bf16_of and eps_m_of for the searches: they MOVE TOGETHER; test_prefilter_plan_cpu.py compares)
__host__ __device__ inline double eps_a_of(int D, bool lo, bool resident = false) {
    if (resident) return (lo ? 0x1p-21 : 0x1p-11 + 0x1p-21) + 6.06 * D * 0x1p-24 + sqrt((double)D) * 0x1p-27;
    return (lo ? 0x1p-11 + 0x1p-21 : 0x1p-10 + 0x1p-21) + 6.06 * D * 0x1p-24 + 2.0 * sqrt((double)D) * 0x1p-27;
}

// the same bound for a resident bf16 bank multiplied by v_mfma_f32_16x16x32_bf16 (file header, "Resident bf16 bank")
__host__ __device__ inline double eps_a_bf16_of(int D, bool lo) {
    return (lo ? 0x1p-18 : 0x1p-9) + 6.06 * D * 0x1p-24 + D * 0x1p-38;
}
// what a bf16 search asks of its operands: every nonzero row element in [2^-BF_ROW_LO, 2^BF_ROW_HI) and a finite weighted norm --
// any other row takes the {0, inf, 1, 0} constants --, the query's scale 2^-f in (2^-BF_SCALE_LO, 2^BF_SCALE_HI) -- any other
// query is flagged for the exact route (init_state_kernel)
constexpr int BF_QMAX_EXP = -20;          // the largest |q'| of a query lies in [2^(BF_QMAX_EXP - 1), 2^BF_QMAX_EXP)
constexpr int BF_ROW_LO = 60, BF_ROW_HI = 120, BF_SCALE_LO = 100, BF_SCALE_HI = 30;

// ---- preparation --------------------------------------------------------------------------------------------------
// one wave per row: scale exponent, fp16 image, ||x'||_2 (rounded up), scaled weighted norm.
// rowp[i] = {xn * 2^-e, ||x'||_2 (1 + D 2^-22), 2^-e, 0}; rows N .. rows_padded-1 (whole tiles of BT rows) hold a sentinel.
// The four components are the row's B operand of the candidate test's v_mfma_f32_16x16x4_f32 (prefilter_kernel, item epilogue):
// the last one multiplies the queries' 0 and must stay finite.
__global__ __launch_bounds__(256) void bank16_kernel(const float *__restrict__ bank, const float *__restrict__ xn, int64_t N, int D,
                                                      half_t *__restrict__ bank16, float4 *__restrict__ rowp, int64_t rows_padded) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) {
        // padding up to a whole bank tile: zeros, and ||x'|| = NaN makes the candidate test fail for every query
        if (row < rows_padded) {
            for (int d = lane * 4; d < D; d += 256) *(uint2 *)(bank16 + row * D + d) = make_uint2(0u, 0u);
            if (lane == 0) rowp[row] = make_float4(0.f, NAN, 0.f, 0.f);
        }
        return;
    }
    const float *x = bank + row * D;
    float mx = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4 *)(x + d);
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    mx = wave_max(mx);
    half_t *o = bank16 + row * D;
    int e = 0;
    if (mx > 0.f && mx < INFINITY) {
        (void)frexpf(mx, &e);            // mx = m * 2^e, m in [0.5, 1)
        e -= 14;                         // mx * 2^-e in [2^13, 2^14)
    }
    if (!(mx < INFINITY) || e < -126) {
        // a row with an infinite element cannot be bounded, and neither can one so small that its scale 2^-e would
        // overflow (largest |x| below ~2^-113: the fp16 image would be inf / NaN and the row silently lost): fp16 zeros
        // + ||x'|| = inf make every query keep it as a candidate (U = inf), so the exact stage decides
        for (int d = lane * 4; d < D; d += 256) *(uint2 *)(o + d) = make_uint2(0u, 0u);
        // (the weighted-norm slot is 0, not the row's -- possibly infinite -- norm: the test's fma chain must not meet inf - inf)
        if (lane == 0) rowp[row] = make_float4(0.f, INFINITY, 1.0f, 0.f);
        return;
    }
    const float s = ldexpf(1.0f, -e);
    float ss = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4 *)(x + d);
        const float a = v.x * s, b = v.y * s, c = v.z * s, dd = v.w * s;
        ss = fmaf(a, a, fmaf(b, b, fmaf(c, c, fmaf(dd, dd, ss))));
        typedef __attribute__((ext_vector_type(4))) _Float16 half4;
        half4 h;
        h[0] = (half_t)a; h[1] = (half_t)b; h[2] = (half_t)c; h[3] = (half_t)dd;
        *(half4 *)(o + d) = h;
    }
    ss = wave_sum(ss);
    if (lane == 0) {
        const float nx = sqrtf(ss) * (1.0f + (float)D * 0x1p-22f);
        const float xnv = xn[row];
        rowp[row] = make_float4(xnv * s, nx, s, 0.f);
    }
}

// the same for a resident fp16 bank (file header): one wave per row, NO image -- rowp[i] = {xn, nx, 1, 0} with
// nx = ||x||_2 (1 + D 2^-22) + sqrt(nsub) * sub_scale, rounded up (sub_scale = 2^-14 / eps_a, raised, from the host); the same
// sentinel for rows N .. rows_padded-1.  tail (NULL when N is a whole number of tiles): one tile [BT, D] that receives rows
// tail_first .. N-1 (tail_first = N rounded down to whole tiles) and zeros behind them.
__global__ __launch_bounds__(256) void bank16_rowp_lp_kernel(const half_t *__restrict__ bank, const float *__restrict__ xn, int64_t N,
                                                              int D, float4 *__restrict__ rowp, int64_t rows_padded,
                                                              half_t *__restrict__ tail, int64_t tail_first, float sub_scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_padded) return;
    half_t *t = tail && row >= tail_first ? tail + (row - tail_first) * D : nullptr;
    if (row >= N) {
        if (t)
            for (int d = lane * 4; d < D; d += 256) *(uint2 *)(t + d) = make_uint2(0u, 0u);
        if (lane == 0) rowp[row] = make_float4(0.f, NAN, 0.f, 0.f);
        return;
    }
    const half_t *x = bank + row * D;
    float ss = 0.f, nsub = 0.f, bad = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const uint2 raw = *(const uint2 *)(x + d);
        if (t) *(uint2 *)(t + d) = raw;
        typedef __attribute__((ext_vector_type(4))) _Float16 half4;
        const half4 h = __builtin_bit_cast(half4, raw);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = (float)h[j];                 // exact
            const float m = fabsf(a);
            ss = fmaf(a, a, ss);
            nsub += (m > 0.f && m < 0x1p-14f) ? 1.f : 0.f;
            bad = !(m < INFINITY) ? 1.f : bad;           // inf or NaN
        }
    }
    ss = wave_sum(ss);
    nsub = wave_sum(nsub);                               // <= D <= 4096: exact
    bad = wave_max(bad);
    if (lane == 0) {
        // a row with an inf / NaN element cannot be bounded: ||x|| = inf makes every query keep it (bank16_kernel's rule)
        const float nx = fmaf(sqrtf(nsub), sub_scale, sqrtf(ss) * (1.0f + (float)D * 0x1p-22f)) * (1.0f + 0x1p-21f);
        rowp[row] = bad != 0.f ? make_float4(0.f, INFINITY, 1.0f, 0.f) : make_float4(xn[row], nx, 1.0f, 0.f);
    }
}

// the same for a resident bf16 bank (file header, "Resident bf16 bank"): rowp[i] = {xn, nx, 1, 0} with nx = ||x||_2 (1 + D 2^-22),
// rounded up -- no additive term: a row that could need one is outside the window and takes {0, inf, 1, 0}.  The squares of
// bf16 elements leave fp32's range on both sides, so the norm is taken of the row scaled by a power of two (second pass over
// the row: it is in L2).  Same sentinel, same tail tile.
__global__ __launch_bounds__(256) void bankbf16_rowp_kernel(const unsigned short *__restrict__ bank, const float *__restrict__ xn, int64_t N,
                                                             int D, float4 *__restrict__ rowp, int64_t rows_padded,
                                                             unsigned short *__restrict__ tail, int64_t tail_first) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_padded) return;
    unsigned short *t = tail && row >= tail_first ? tail + (row - tail_first) * D : nullptr;
    if (row >= N) {
        if (t)
            for (int d = lane * 4; d < D; d += 256) *(uint2 *)(t + d) = make_uint2(0u, 0u);
        if (lane == 0) rowp[row] = make_float4(0.f, NAN, 0.f, 0.f);
        return;
    }
    const unsigned short *x = bank + row * D;
    float mx = 0.f, bad = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const uint2 raw = *(const uint2 *)(x + d);
        if (t) *(uint2 *)(t + d) = raw;
        const unsigned int u[4] = {raw.x << 16, raw.x & 0xFFFF0000u, raw.y << 16, raw.y & 0xFFFF0000u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float m = fabsf(__uint_as_float(u[j]));                  // exact
            bad = (!(m < ldexpf(1.0f, BF_ROW_HI)) || (m > 0.f && m < ldexpf(1.0f, -BF_ROW_LO))) ? 1.f : bad;   // inf / NaN / outside the window
            mx = fmaxf(mx, m);
        }
    }
    mx = wave_max(mx);
    bad = wave_max(bad);
    const float xnv = xn[row];
    if (!(xnv < INFINITY)) bad = 1.f;                        // the weighted norm overflowed (or is NaN): a * xn of the test is not a number
    if (bad != 0.f) {
        if (lane == 0) rowp[row] = make_float4(0.f, INFINITY, 1.0f, 0.f);
        return;
    }
    int e = 0;
    if (mx > 0.f) (void)frexpf(mx, &e);                      // mx 2^-e in [0.5, 1); e in (-BF_ROW_LO, BF_ROW_HI]
    const float s = ldexpf(1.0f, -e);
    float ss = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const uint2 raw = *(const uint2 *)(x + d);
        const float a = __uint_as_float(raw.x << 16) * s, b = __uint_as_float(raw.x & 0xFFFF0000u) * s;
        const float c = __uint_as_float(raw.y << 16) * s, dd = __uint_as_float(raw.y & 0xFFFF0000u) * s;
        ss = fmaf(a, a, fmaf(b, b, fmaf(c, c, fmaf(dd, dd, ss))));
    }
    ss = wave_sum(ss);
    if (lane == 0) {
        // (an element 2^-126 of the row maximum or less loses its square: below 2^-250 of ss, inside the factor's slack)
        const float nx = ldexpf(sqrtf(ss) * (1.0f + (float)D * 0x1p-22f) * (1.0f + 0x1p-21f), e);
        rowp[row] = make_float4(xnv, nx, 1.0f, 0.f);
    }
}

// queries: tw[q] -> qh, ql (fp16, scaled by 2^-f); qbase[q] = {qn * 2^-f, eps_a * ||q'|| (1 + D 2^-22), 2^-f, qn}
// BF: the bf16 form -- qh = bf16(q'), ql = bf16(q' - qh), the largest |q'| in [2^(BF_QMAX_EXP - 1), 2^BF_QMAX_EXP): bf16 has fp32's
// exponent range, so the scale is chosen for the fp32 ACCUMULATOR, which must hold 2 D products against any finite row
template <bool BF>
__global__ __launch_bounds__(256) void query16_kernel(const float *__restrict__ tw, const float *__restrict__ qn, int Q, int D,
                                                       half_t *__restrict__ qh, half_t *__restrict__ ql, float4 *__restrict__ qbase,
                                                       float eps_a) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) {
        // rows up to a whole query tile (the grid covers them): zeros; their test parameters let no pair pass
        if (q < (Q + QPAD - 1) / QPAD * QPAD)
            for (int d = lane * 4; d < D; d += 256) {
                *(uint2 *)(qh + (int64_t)q * D + d) = make_uint2(0u, 0u);
                *(uint2 *)(ql + (int64_t)q * D + d) = make_uint2(0u, 0u);
            }
        return;
    }
    const float *x = tw + (int64_t)q * D;
    float mx = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4 *)(x + d);
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    mx = wave_max(mx);
    int e = 0;
    if (mx > 0.f && mx < INFINITY) {
        (void)frexpf(mx, &e);
        e -= BF ? BF_QMAX_EXP : 14;
    }
    if (e < -126) e = -126;             // keep 2^-e finite; such a query (scale == 2^126) is flagged for the exact path by init_state_kernel
    if (BF && e > BF_SCALE_LO) e = BF_SCALE_LO;   // (keeps 2^e finite too; flagged likewise)
    const float s = ldexpf(1.0f, -e);
    float ss = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4 *)(x + d);
        const float a[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
        if (BF) {
            // (the squares of elements below 2^-43 of the maximum underflow: below 2^-86 of ss, inside the slack of nq's factor)
            bf16x4 h, l;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ss = fmaf(a[j], a[j], ss);
                h[j] = (bf16_t)a[j];
                l[j] = (bf16_t)(a[j] - (float)h[j]);  // exact difference in fp32, then one bf16 rounding
            }
            *(bf16x4 *)(qh + (int64_t)q * D + d) = h;
            *(bf16x4 *)(ql + (int64_t)q * D + d) = l;
            continue;
        }
        typedef __attribute__((ext_vector_type(4))) _Float16 half4;
        half4 h, l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ss = fmaf(a[j], a[j], ss);
            h[j] = (half_t)a[j];
            l[j] = (half_t)(a[j] - (float)h[j]);      // exact difference in fp32, then one fp16 rounding
        }
        *(half4 *)(qh + (int64_t)q * D + d) = h;
        *(half4 *)(ql + (int64_t)q * D + d) = l;
    }
    ss = wave_sum(ss);
    if (lane == 0) {
        const float nq = sqrtf(ss) * (1.0f + (float)D * 0x1p-22f);
        qbase[q] = make_float4(qn[q] * s, eps_a * nq, s, qn[q]);
    }
}

// ---- a selection of the bank's rows (skyemb_prefilter_select_prepare) ----------------------------------------------------------
// words: bit i & 31 of word i >> 5 is row i, padding bits zero (skyemb_pack_select).  The masked copy of the row constants: a
// deselected row -- whatever it held, the {0, inf, 1, 0} "keep for every query" of an unboundable row included -- and every row
// past N gets the padding sentinel, whose NaN fails the candidate test for every query.
__global__ __launch_bounds__(256) void select_rowp_kernel(const unsigned int *__restrict__ words, const float4 *__restrict__ rowp,
                                                           int64_t N, int64_t rows_padded, float4 *__restrict__ rowp_sel) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows_padded) return;
    const bool on = i < N && ((words[i >> 5] >> (i & 31)) & 1u) != 0u;
    rowp_sel[i] = on ? rowp[i] : make_float4(0.f, NAN, 0.f, 0.f);
}
// the live tiles -- those of the ceil(N / BT) bank tiles with a selected row: a popcount over the BT / 32 words of each -- in
// ascending order; info = {their number, 1 if the last bank tile is one of them}.  One workgroup, 1024 tiles per round.
__global__ __launch_bounds__(1024) void select_tiles_kernel(const unsigned int *__restrict__ words, int64_t nwords, int tiles_all,
                                                             int *__restrict__ tiles, int *__restrict__ info) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int r0 = 0; r0 < tiles_all; r0 += 1024) {
        const int t = r0 + tid;
        int pc = 0;
        if (t < tiles_all)
            for (int j = 0; j < BT / 32; ++j) {
                const int64_t wi = (int64_t)t * (BT / 32) + j;
                if (wi < nwords) pc += __popc(words[wi]);
            }
        const bool live = pc > 0;
        const unsigned long long m = __ballot(live);
        if (lane == 0) wsum[wave] = __builtin_popcountll(m);
        __syncthreads();
        int off = base, tot = 0;
        for (int w = 0; w < 16; ++w) {
            off += w < wave ? wsum[w] : 0;
            tot += wsum[w];
        }
        off += __builtin_popcountll(m & ((1ull << lane) - 1));
        if (live) tiles[off] = t;                              // off < the number of live tiles <= tiles_all
        if (t == tiles_all - 1) info[1] = live ? 1 : 0;
        base += tot;
        __syncthreads();
    }
    if (tid == 0) info[0] = base;
}

// ---- stage 1 ------------------------------------------------------------------------------------------------------
// Operand tile (rows x 32 k, fp16): 64-byte rows; 16-byte chunk c of row r is stored at chunk c ^ swz(r), the XOR applied
// to the per-lane SOURCE address (the LDS-DMA destination is wave base + lane * 16).  One instruction = 16 rows.
// swz makes the four 16-lane groups of a ds_read_b128 fragment read ({rows 0-3, 12-15 of chunk c, rows 4-11 of chunk c+1}
// and the like, MI355X_MICROARCH.md LDS table) hit 16 distinct 16-byte slots of the 256-byte bank row.
__device__ __forceinline__ int swz(int r) {
    const int g = (r >> 2) & 3;
    return (((g ^ (g >> 1)) & 1) << 1) | (g >> 1);          // g = 0,1,2,3 -> 0,2,3,1
}
// All three operand arrays are padded to whole tiles (query16_kernel / bank16_kernel), so a piece's address is a
// workgroup-uniform base (tile row, k-step: scalar registers) plus ONE per-lane 32-bit offset that never changes.  The
// instruction is written out (SGPR-base form, LDS destination in M0): left to the compiler, every piece's 64-bit vector
// address was hoisted out of the loop into registers the accumulators and fragments need (spills inside the k-loop).
// the lane index, recomputed where it is used (volatile asm: neither hoisted nor spilled).  In the k-loop's once-per-item paths
// a value kept alive from the kernel's entry gets spilled, and its reload -- a scratch load the compiler waits for with
// vmcnt(0) -- drains the LDS-DMA ring.
__device__ __forceinline__ int lane_now() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
__device__ __forceinline__ void glds16_sbase(const void *base_uniform, unsigned int lane_off, char *lds_wave_base) {
    const unsigned int dst = (unsigned int)(uintptr_t)(lvoid_t *)lds_wave_base;
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                 :
                 : "v"(lane_off), "s"(base_uniform), "s"(dst)
                 : "memory", "m0");
}
// fragment of 16 rows from row `rbase` (a multiple of 16: swz(rbase + l) == swz(l)): every fragment of a lane sits at
// rbase * 64 + ONE per-lane constant, frag_lane(lane) -- an immediate offset on a single address register
__device__ __forceinline__ int frag_lane(int lane) { return (lane & 15) * 64 + ((((lane >> 4) ^ swz(lane & 15))) << 4); }
__device__ __forceinline__ half8 frag(const char *sbase, int rbase, int lane_c) {
    return *(const half8 *)(sbase + rbase * 64 + lane_c);
}
// ---- the counting fold of a token search under top_t (prefilter_kernel<.., TOK, CNT>) ------------------------------------------------
// The pass bits of a lane are 32 independent columns (one per query block and row fragment).  The count of passed rows of an image
// is kept BIT-SLICED: plane c[b] holds bit b of the count of every column, so one half / full adder over whole words adds 32 counts
// at once.  Same tree as the AND / OR fold: four DPP row shifts (lane l takes lane l + o; the first lane of an aligned group ends
// with the group's count -- a lane whose source lies outside its row adds its own value and is cleared at the end), then, for
// P = 32 / 64, the neighbouring bits of each nibble.  Counts reach 2, 4, 8, 16, 32, 64: at most 7 planes.  No LDS, no per-lane
// branch; lgp and t are wave-uniform.
template <int NPL>
__device__ __forceinline__ void planes_add(unsigned int (&c)[7], const unsigned int (&y)[7]) {   // c[0 .. NPL] = c[0 .. NPL) + y[0 .. NPL)
    unsigned int carry = 0u;
#pragma unroll
    for (int b = 0; b < NPL; ++b) {
        const unsigned int x = c[b] ^ y[b], g = c[b] & y[b];
        c[b] = x ^ carry;
        carry = g | (carry & x);
    }
    c[NPL] = carry;
}
template <int NPL, int CTRL>
__device__ __forceinline__ void planes_add_dpp(unsigned int (&c)[7]) {
    unsigned int y[7];
#pragma unroll
    for (int b = 0; b < NPL; ++b) y[b] = (unsigned int)__builtin_amdgcn_update_dpp((int)c[b], (int)c[b], CTRL, 0xF, 0xF, false);
    planes_add<NPL>(c, y);
}
template <int NPL>
__device__ __forceinline__ void planes_add_shr(unsigned int (&c)[7], int sh) {
    unsigned int y[7];
#pragma unroll
    for (int b = 0; b < NPL; ++b) y[b] = c[b] >> sh;
    planes_add<NPL>(c, y);
}
// m: the lane's pass bits -> the bit of an image's first row (first lane of its aligned group of 2^min(lgp, 4) lanes; P = 32 / 64:
// bit 0 / 2 resp. bit 0 of each nibble) is set iff at least t of its 2^lgp rows passed; every other lane and bit is cleared
__device__ __forceinline__ unsigned int count_fold(unsigned int m, int lgp, int t, int l16) {
    const int lg16 = lgp < 4 ? lgp : 4;
    unsigned int c[7] = {m, 0u, 0u, 0u, 0u, 0u, 0u};
    if (lg16 >= 1) planes_add_dpp<1, 0x101>(c);              // row_shl:1
    if (lg16 >= 2) planes_add_dpp<2, 0x102>(c);              // row_shl:2
    if (lg16 >= 3) planes_add_dpp<3, 0x104>(c);              // row_shl:4
    if (lg16 >= 4) planes_add_dpp<4, 0x108>(c);              // row_shl:8
    if (lgp >= 5) planes_add_shr<5>(c, 1);                   // blocks (0, 1) -> bit 0, (2, 3) -> bit 2
    if (lgp >= 6) planes_add_shr<6>(c, 2);                   // all four blocks -> bit 0
    // count >= t, from the lowest plane up: a higher plane overrules what the lower ones said, equal bits keep it (count == t: yes)
    unsigned int ge = ~0u;
#pragma unroll
    for (int b = 0; b < 7; ++b) ge = ((t >> b) & 1) ? (c[b] & ge) : (c[b] | ge);
    if (lgp >= 5) ge &= 0x55555555u;
    if (lgp >= 6) ge &= 0x11111111u;
    return (l16 & ((1 << lg16) - 1)) == 0 ? ge : 0u;
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// The pair (q, i) is a candidate iff  dot^ + c * nx'_i >= a * xn'_i + b * se_i  with
//   a = tau * qn'   b = tau * eps * 2^-f   c = eps_a ||q'||     (a, b lowered and c raised by 2^-19 relative, see below).
// Round 4: the test is ONE matrix instruction per 16 x 16 block of pairs.  qpar[q] = {-a, c, -b, 0} is the query's row of an
// A operand, rowp[i] = {xn', nx', se, 0} the row's column of a B operand, and
//   t = v_mfma_f32_16x16x4_f32(qpar rows, rowp columns, C = dot^ block)  =  dot^ - a xn' + c nx' - b se   (fp32 fma chain)
// lands in scratch registers (the accumulators keep dot^ for the candidate lists); the pair passes iff t >= 0 (NaN fails), one
// compare + one add-with-carry per pair into the lane's bit mask.  Before, every pair cost two fmas, a multiply, a compare and
// the mask update on the vector ALU: 128 pairs per lane and item = 31 % of the pass.
// Roundings: the chain rounds four times, each by <= 2^-24 of a partial sum bounded by S = |dot^| + |a xn'| + |c nx'| + |b se|, and
// a, b carry one or two roundings of their own.  The slack 2^-19 (|a xn'| + |b se| + |c nx'|) =: 2^-19 T1 built into the constants
// covers them: if |dot^| <= 2 T1 the chain's error is <= 2^-22 * 3.01 T1 < 2^-19 T1; if |dot^| > 2 T1 the exact value has the
// sign of dot^ and magnitude > |dot^| / 2, far above the error.  So every pair that satisfies the inequality in exact arithmetic
// (the condition the proof of the file header needs) passes.
// Work items: bank tile t of [t0, t1) x query tile; bank tiles are dealt to the XCDs (t - t0) % 8 == blockIdx.x % 8, and an
// XCD walks its items group-of-GQ-query-tiles outermost, then bank tile, then query tile: the GQ query tiles stay in its
// L2 while its bank tiles stream through once per group.  The LDS ring never drains between items.
// MODE 0: first slice, every pair is stored (slot = row)   1: candidates appended to the per-query lists directly (returning
// global atomics: the short early phases, whose loose thresholds pass several per cent of the pairs)   2: candidates staged
// in LDS and flushed to the workgroup's own region (the long late phases)
// SEL (a search under a selection, select_tiles_kernel): [t0, t1) are POSITIONS in the ascending list `tiles` of the live bank
// tiles -- position p stands for bank tile tiles[p], whose rows, row constants (the masked copy: a deselected row fails every test)
// and row numbers the item uses; only the take-all slots are counted by position.  Without SEL `tiles` is not read (NULL) and a
// position is its own tile: the instruction stream of the unselected search.
// BF: the operands are bf16 (a resident bf16 bank, query16_kernel<true>'s images): the same bytes through the same ring and fragments,
// multiplied by v_mfma_f32_16x16x32_bf16 -- the one difference.  Without BF: the instruction stream it has always been.
// TOK (a resident token bank, "Patch-token banks" below; MODE 1 and 2 only): the rows are the N * P token rows of N images, P = 2^lgp
// a divisor of 64 (tok = lgp | is_max << 8), and the candidates are IMAGES: between the masks and the appends the pass bits of an
// image's P rows are folded -- AND under 'min', OR under 'max' -- into the image's first row, whose lane appends the image number.
// Without TOK `tok` is not read: the instruction stream of the row search.
// CNT (with TOK; 'min' under top_t = t, 1 < t < P: tok = lgp | t << 16): the fold COUNTS -- an image is a candidate iff at least t of its
// P rows passed (count_fold below).  AND is the case t = P and OR the case t = 1: those keep the fold above and its instances.
template <int MODE, bool LO, bool SEL, bool BF = false, bool TOK = false, bool CNT = false>
__global__ __launch_bounds__(NT) void prefilter_kernel(const half_t *__restrict__ qh, const half_t *__restrict__ ql,
                                                       const half_t *__restrict__ bank16, const float4 *__restrict__ rowp,
                                                       const int *__restrict__ tiles,
                                                       const float4 *__restrict__ qpar, int Q, int64_t N, int D, int t0, int t1,
                                                       int cap, int *__restrict__ cnt, int *__restrict__ cand_i, float *__restrict__ cand_d,
                                                       uint4 *__restrict__ wg_list, int *__restrict__ wg_count, int capw,
                                                       int *__restrict__ overflow, int tok
#if defined(PF_STAMP) || defined(PF_CLOCK)
                                                       , unsigned long long *__restrict__ dbg
#endif
                                                       ) {
    constexpr bool TAKE_ALL = MODE == 0, STAGED = MODE == 2;
    constexpr int QT = qtile(LO), MI = QT / 2 / 16;        // queries per tile; 16-row query fragments per wave (the wave's half of the tile)
    constexpr int STAGE = stage_bytes(LO), NI = pieces(LO), A_BYTES = QT * BK * 2, B_OFF = Q_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef PF_STAMP
    unsigned int seg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev;
    auto stamp = [&](int which) {
        unsigned long long t;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
        __builtin_amdgcn_sched_barrier(0);
        if (which >= 0) seg[which] += (unsigned int)(t - tprev);
        tprev = t;
    };
#define STAMP(w) stamp(w)
#else
#define STAMP(w)
#endif
    float4 *spar = (float4 *)(smem + NSTAGE * STAGE);        // [QT] test parameters of the item's queries
    float4 *srow = spar + QT;                                 // [BT] constants of the item's bank rows
    uint2 *stg = (uint2 *)(srow + BT);                        // [SCAP] candidates of the item being finished: {q_local << 8 | row_local, dot^}
    int *stg_n = (int *)(stg + SCAP);                         // their number (may exceed SCAP: the excess was flagged, not stored)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;                 // 2 x 4 waves: QT / 2 queries x 64 rows each
    const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3, nlocal = gridDim.x >> 3;
    const int T = t1 - t0, Tx = xcd < T ? (T - xcd + 7) / 8 : 0;
    const int nqt = (Q + QT - 1) / QT;
    const int full = nqt / GQ, last = nqt % GQ;
    const int items = Tx * nqt;                               // items * KT < 2^31: checked on the host (topk_prefiltered)
    const int KT = D / BK;
    // this workgroup's items: local, local + nlocal, ...
    const int my_items = items > local ? (items - local + nlocal - 1) / nlocal : 0;
    if (my_items == 0) {
        if (MODE == 2 && threadIdx.x == 0) wg_count[blockIdx.x] = 0;
        return;
    }

    auto item_of = [&](int n, int &qt, int &t, int &p) {    // n-th item of this workgroup -> (query tile, bank tile, its position)
        const int idx = local + n * nlocal;
        const int per_full = GQ * Tx;
        int g, within, tt;
        if (idx < per_full * full) {
            g = idx / per_full;
            const int rem = idx - g * per_full;
            tt = rem / GQ;
            within = rem - tt * GQ;
        } else {
            g = full;
            const int rem = idx - per_full * full;
            tt = rem / last;
            within = rem - tt * last;
        }
        qt = __builtin_amdgcn_readfirstlane(g * GQ + within);
        p = __builtin_amdgcn_readfirstlane(t0 + tt * 8 + xcd);
        if (SEL) {
            // one scalar load per item, written out: a vector load here would be waited for with vmcnt(0), which drains the ring
            asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "s"(tiles + p) : "memory");
        } else {
            t = p;
        }
    };
    // ---- issue cursor: the stage being requested runs AHEAD k-steps in front of the one being read, across item boundaries.
    // Each wave owns four 1 KiB pieces of a stage: rows [16 wave, +16) of the hi and of the lo query image, rows
    // [32 wave, +32) of the bank tile.  Their addresses are three running scalar pointers (64 bytes further per k-step,
    // re-based when the cursor enters a new item) plus one per-lane offset that never changes: a k-step's address work is a
    // handful of scalar adds (recomputing bases from the tile numbers cost ~80 scalar instructions per k-step and wave).
    static_assert(BT / 16 / NW == 2 && Q_BYTES / 1024 / NW == 2, "piece ownership below: two query and two bank pieces per wave");
    const unsigned int lane_off = (unsigned int)((lane >> 2) * D * 2 + (((lane & 3) ^ swz(lane >> 2)) << 4));
    int n_iss = 0, kt_iss = 0;
    int qt_cur, t_cur, p_cur, qt_nxt = 0, t_nxt = 0, p_nxt = 0;   // the item being multiplied / the one the issue cursor has entered
    item_of(0, qt_cur, t_cur, p_cur);
    const char *ph, *pl, *pb;
    auto rebase = [&](int qt, int t) {
        const int64_t qoff = ((int64_t)qt * QT + wave * (QT / NW)) * D * 2;   // LO: 16 rows of hi and of lo; else 32 rows of hi
        ph = (const char *)qh + qoff;
        pl = (const char *)ql + qoff;
        pb = (const char *)bank16 + ((int64_t)t * BT + wave * 32) * D * 2;
    };
    rebase(qt_cur, t_cur);
    const int bank_piece2 = 16 * D * 2;                      // second bank piece: 16 rows further
    // half 0: the two query pieces; half 1: the two bank pieces, then the cursor moves on
    auto issue_half = [&](int buf, int half) {
        char *st = smem + buf * STAGE;
        if (half == 0) {
            glds16_sbase(ph, lane_off, st + wave * (QT / NW) * 64);
            if (LO) glds16_sbase(pl, lane_off, st + A_BYTES + wave * 1024);
            else glds16_sbase(ph + bank_piece2, lane_off, st + wave * 2048 + 1024);      // rows 16..31 of the wave's 32
        } else {
            glds16_sbase(pb, lane_off, st + B_OFF + wave * 2048);
            glds16_sbase(pb + bank_piece2, lane_off, st + B_OFF + wave * 2048 + 1024);
            ph += BK * 2; pl += BK * 2; pb += BK * 2;
            if (++kt_iss == KT) {
                kt_iss = 0;
                if (++n_iss < my_items) {
                    item_of(n_iss, qt_nxt, t_nxt, p_nxt);
                    rebase(qt_nxt, t_nxt);
                }
            }
        }
    };

    f32x4 acc[MI][4];
    half8 fh[MI], fl[LO ? MI : 1], fb[4];
    const bool late = wave >= 4;                             // wave-uniform (SGPR)
    const int steps = my_items * KT;
#pragma unroll
    for (int p = 0; p < AHEAD; ++p)
        if (p < steps) {
            issue_half(p, 0);
            issue_half(p, 1);
        }

    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    };
    const int flane = frag_lane(lane);
    auto read_frags = [&](int b) {
#ifdef PF_NOREAD
        return;
#endif
        // one address register per operand: stage base + the wave's first row + the lane's constant; the rest are immediates
        const char *sa = smem + b * STAGE + wm * (QT / 2) * 64 + flane, *sb = smem + b * STAGE + B_OFF + wn * 64 * 64 + flane;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            fh[i] = frag(sa, i * 16, 0);
            if (LO) fl[i] = frag(sa + A_BYTES, i * 16, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = frag(sb, j * 16, 0);
    };
    // the four LDS-DMA instructions of the next stage cost ~100+ issue cycles each: they go BETWEEN the MFMAs (whose execution
    // covers them), not in front of them
    // two of the wave's four LDS-DMA pieces of a k-step are requested between the MFMAs (whose execution covers their
    // issue cost), the other two in the wave's read phase
    auto multiply = [&](bool issue, int ibuf, int half) {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            if (i == 1) {
                __builtin_amdgcn_sched_barrier(0);
#ifndef PF_NODMA
                if (issue) issue_half(ibuf, half);
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
#ifndef PF_NOMFMA
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (BF) {      // (the fragments are 16 bytes of LDS either way: the bits are handed over as they are)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fh[i]), __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
                    if (LO) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fl[i]), __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
                } else {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh[i], fb[j], acc[i][j], 0, 0, 0);
                    if (LO) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fl[i], fb[j], acc[i][j], 0, 0, 0);
                }
            }
#else
            acc[i][0][0] += (float)fh[i][0] + (float)fb[i & 3][2];
#endif
        }
    };
    auto item_epilogue = [&](int qt, int t, int p) {
        // ---- epilogue of the item: per 16x16 block a lane holds queries 4*(lane>>4)+r (r = 0..3) x bank row (lane & 15).
        // All 16 MI tests of the lane are branch-free (bit masks mr[r]); only waves that found something enter the append path.
        // (the lane coordinates go through an empty asm: everything addressed from them is then computed HERE, once per item,
        // instead of being hoisted out of the k-loop into registers that the accumulators and fragments need)
        const int ln = lane_now();
        const int l16 = ln & 15, l4 = ln >> 4;
        // B operand of the test: component (lane >> 4) of the constants of bank row (lane & 15) of each 16-row block
        float tb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) tb[j] = ((const float *)srow)[(wn * 64 + j * 16 + l16) * 4 + l4];
        // mr[r]: the lane's tests of query 4 * (lane >> 4) + r, one bit per (block i, row fragment j): bit (MI - 1 - i) * 4 + j
        unsigned int mr[4] = {0u, 0u, 0u, 0u};
#ifdef PF_NOTEST   // experiment build: the accumulators are consumed, no pair is tested (what the 128 tests per lane and item cost)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(acc[i][j]));
#else
        // A operands: component (lane >> 4) of the parameters of query (lane & 15) of each block
        float ta[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) ta[i] = ((const float *)spar)[(wm * (QT / 2) + i * 16 + l16) * 4 + l4];
        // Software pipeline, written out: one group = the matrix instruction of fragment j of block i + 1, then the eight vector
        // instructions that fold fragment j of block i into the four masks (mr[r] = 2 mr[r] + (t >= 0): compare into a scalar
        // pair, add-with-carry; NaN compares false).  An 8-pass matrix instruction occupies its pipe for the 32 cycles the eight
        // vector instructions take to issue, so both run all the time; the four masks are four independent chains (one mask
        // register for all sixteen pairs of a block was a chain of 32 dependent instructions: 375 cycles per block, stamped).
        // The compiler does not see the matrix instruction inside the asm: the distance from it to the first read of its result
        // (three more groups = 27 instructions) is kept by construction.
        f32x4 tst[2][4];
#pragma unroll
        for (int j = 3; j >= 0; --j) tst[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ta[0], tb[j], acc[0][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                unsigned long long c0, c1, c2, c3;
                if (i + 1 < MI)
                    asm volatile("v_mfma_f32_16x16x4_f32 %0, %9, %10, %11\n\t"
                                 "v_cmp_le_f32_e64 %5, 0, %12\n\tv_cmp_le_f32_e64 %6, 0, %13\n\t"
                                 "v_cmp_le_f32_e64 %7, 0, %14\n\tv_cmp_le_f32_e64 %8, 0, %15\n\t"
                                 "v_addc_co_u32_e64 %1, %5, %1, %1, %5\n\tv_addc_co_u32_e64 %2, %6, %2, %2, %6\n\t"
                                 "v_addc_co_u32_e64 %3, %7, %3, %3, %7\n\tv_addc_co_u32_e64 %4, %8, %4, %4, %8"
                                 : "=&v"(tst[(i + 1) & 1][j]), "+v"(mr[0]), "+v"(mr[1]), "+v"(mr[2]), "+v"(mr[3]), "=&s"(c0), "=&s"(c1),
                                   "=&s"(c2), "=&s"(c3)
                                 : "v"(ta[(i + 1) % MI]), "v"(tb[j]), "v"(acc[(i + 1) % MI][j]), "v"(tst[i & 1][j][0]), "v"(tst[i & 1][j][1]),
                                   "v"(tst[i & 1][j][2]), "v"(tst[i & 1][j][3]));
                else
                    asm volatile("v_cmp_le_f32_e64 %4, 0, %8\n\tv_cmp_le_f32_e64 %5, 0, %9\n\t"
                                 "v_cmp_le_f32_e64 %6, 0, %10\n\tv_cmp_le_f32_e64 %7, 0, %11\n\t"
                                 "v_addc_co_u32_e64 %0, %4, %0, %0, %4\n\tv_addc_co_u32_e64 %1, %5, %1, %1, %5\n\t"
                                 "v_addc_co_u32_e64 %2, %6, %2, %2, %6\n\tv_addc_co_u32_e64 %3, %7, %3, %3, %7"
                                 : "+v"(mr[0]), "+v"(mr[1]), "+v"(mr[2]), "+v"(mr[3]), "=&s"(c0), "=&s"(c1), "=&s"(c2), "=&s"(c3)
                                 : "v"(tst[i & 1][j][0]), "v"(tst[i & 1][j][1]), "v"(tst[i & 1][j][2]), "v"(tst[i & 1][j][3]));
            }
        }
#endif
        STAMP(5);
#if defined(PF_NOMFMA) || defined(PF_NOREAD) || defined(PF_NODMA) || defined(PF_NOAPPEND)
#pragma unroll
        for (int r = 0; r < 4; ++r) {                // experiment builds: the tests are computed, nothing is appended
            asm volatile("" ::"v"(mr[r]));
            mr[r] = 0;
        }
#endif
        if constexpr (TOK && CNT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) mr[r] = count_fold(mr[r], tok & 255, tok >> 16, l16);
        } else if constexpr (TOK) {
            // Rows of a 16-row block lie across the 16 lanes l16; the four blocks of the wave's strip are bit j of each nibble.  An
            // image is 2^lgp neighbouring rows of the strip.  Up to 16 rows: a tree over the lane bits with DPP row shifts (lane l
            // takes lane l + o of its 16-lane row; the first lane of an aligned group ends with the fold of the whole group, the
            // other lanes are cleared).  No LDS traffic.  32 / 64 rows: bit pairs / all four bits of each nibble besides.
            const int lgp = tok & 255;
            const bool is_max = (tok >> 8) != 0;                 // wave-uniform, like lgp
            const int lg16 = lgp < 4 ? lgp : 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                unsigned int m = mr[r], u;
                if (lg16 >= 1) { u = (unsigned int)__builtin_amdgcn_update_dpp((int)m, (int)m, 0x101, 0xF, 0xF, false); m = is_max ? (m | u) : (m & u); }   // row_shl:1
                if (lg16 >= 2) { u = (unsigned int)__builtin_amdgcn_update_dpp((int)m, (int)m, 0x102, 0xF, 0xF, false); m = is_max ? (m | u) : (m & u); }   // row_shl:2
                if (lg16 >= 3) { u = (unsigned int)__builtin_amdgcn_update_dpp((int)m, (int)m, 0x104, 0xF, 0xF, false); m = is_max ? (m | u) : (m & u); }   // row_shl:4
                if (lg16 >= 4) { u = (unsigned int)__builtin_amdgcn_update_dpp((int)m, (int)m, 0x108, 0xF, 0xF, false); m = is_max ? (m | u) : (m & u); }   // row_shl:8
                if (lgp >= 5) { u = m >> 1; m = (is_max ? (m | u) : (m & u)) & 0x55555555u; }    // blocks (0, 1) -> bit 0, (2, 3) -> bit 2
                if (lgp >= 6) { u = m >> 2; m = (is_max ? (m | u) : (m & u)) & 0x11111111u; }    // all four blocks -> bit 0
                mr[r] = (l16 & ((1 << lg16) - 1)) == 0 ? m : 0u;
            }
        }
        auto passed = [&](int i, int r, int j) -> bool { return (mr[r] >> ((MI - 1 - i) * 4 + j)) & 1u; };
        // Appends are rare (a few per wave and item): the walk over the lane's 128 bits is pruned by WAVE-UNIFORM branches (a
        // ballot per block, then per query row of a flagged block); per-lane branches only below those.  (Thirty-two per-lane
        // branches per item, taken or not, cost 2.7 k cycles per item and wave group, stamped.)
        const unsigned int anyr = mr[0] | mr[1] | mr[2] | mr[3];
        auto block_flagged = [&](int i) -> bool { return __builtin_amdgcn_ballot_w64(((anyr >> ((MI - 1 - i) * 4)) & 15u) != 0u) != 0ull; };
        auto row_flagged = [&](int i, int r) -> bool { return __builtin_amdgcn_ballot_w64(((mr[r] >> ((MI - 1 - i) * 4)) & 15u) != 0u) != 0ull; };
        if (TAKE_ALL) {
            // first slice: every (query, row) pair of the slice is a candidate, slot = row within the slice (no counters);
            // pairs that fail even the open test (NaN) are stored as -inf and dropped by the select step
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = qt * QT + wm * (QT / 2) + i * 16 + 4 * l4 + r;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int64_t row = (int64_t)t * BT + wn * 64 + j * 16 + l16;
                        // SEL: slot = position in the list x BT + row in tile; every slot of the slice is written (the host counts
                        // first * BT of them), rows past N too -- their sentinel constants mark them for select_kernel
                        if (q < Q && (SEL || row < N)) {
                            const int64_t o = (int64_t)q * cap + (SEL ? (int64_t)(p - t0) * BT + (wn * 64 + j * 16 + l16) : row - (int64_t)t0 * BT);
                            cand_i[o] = (int)row;
                            cand_d[o] = passed(i, r, j) ? acc[i][j][r] : -INFINITY;
                        }
                    }
                }
        } else if (!STAGED) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
                if (block_flagged(i)) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (row_flagged(i, r)) {
                            const int q = qt * QT + wm * (QT / 2) + i * 16 + 4 * l4 + r;
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (passed(i, r, j)) {
                                    const int pos = atomicAdd(cnt + q, 1);
                                    if (pos < cap) {
                                        cand_i[(int64_t)q * cap + pos] = (t * BT + wn * 64 + j * 16 + l16) >> (TOK ? (tok & 255) : 0);
                                        cand_d[(int64_t)q * cap + pos] = acc[i][j][r];
                                    }
                                }
                        }
                }
        } else {
            // Candidates go to a list in LDS (slot from an LDS counter: no global atomic, no wait on the vector-memory
            // counter that the LDS-DMA ring lives on -- a returning global atomic per candidate cost ~750 cycles per k-step).
            // The workgroup flushes the list to its OWN region of wg_list with plain stores (flush_item); bucket_kernel sorts
            // the regions into the per-query lists afterwards.
            const int kbase = ((wm * (QT / 2) + 4 * l4) << 8) | (wn * 64 + l16);
#pragma unroll
            for (int i = 0; i < MI; ++i)
                if (block_flagged(i)) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (row_flagged(i, r)) {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (passed(i, r, j)) {
                                    const int key = kbase + (((i * 16 + r) << 8) | (j * 16));      // q_local << 8 | row_local
                                    const int slot = atomicAdd(stg_n, 1);
                                    if (slot < SCAP) stg[slot] = make_uint2((unsigned int)key, __float_as_uint(acc[i][j][r]));
                                    else overflow[qt * QT + (key >> 8)] = 1;     // more than the staging list holds: the query is re-run exactly
                                }
                        }
                }
        }
        STAMP(6);
    };
    // the staged candidates of item (qt, t) -> this workgroup's region of wg_list (16 bytes each: query, row, dot^)
    int wpos = 0;
    auto flush_item = [&](int qt, int t) {
        const int tid = wave * 64 + lane_now();
        int n = *stg_n;      // (a plain LDS read: a volatile one became a FLAT load, whose vmcnt(0) drained the LDS-DMA ring once per item)
        // More candidates than the staging list holds: WHICH pairs found no slot depends on the order the waves appended in, so
        // flagging only their queries made the set of re-run queries a matter of timing (a query whose pairs all came first kept
        // a complete list).  The item hands back ALL its queries: the flags depend on the data alone.  (Workgroup-uniform, once
        // per item; the answers were exact either way.)
        if (__builtin_amdgcn_readfirstlane(n) > SCAP && tid < QT && qt * QT + tid < Q) overflow[qt * QT + tid] = 1;
        n = __builtin_amdgcn_readfirstlane(n < SCAP ? n : SCAP);
        uint4 *dst = wg_list + (int64_t)blockIdx.x * capw;
        for (int e = tid; e < n; e += NT) {
            const uint2 c = stg[e];
            const int q = qt * QT + (int)(c.x >> 8), row = (t * BT + (int)(c.x & 255u)) >> (TOK ? (tok & 255) : 0);   // TOK: the image
#ifdef PF_NOFLUSHSTORE
            asm volatile("" ::"v"(q), "v"(row), "v"(c.y));
            continue;
#endif
            if (wpos + e < capw) dst[wpos + e] = make_uint4((unsigned int)q, (unsigned int)row, c.y, 0u);
            else overflow[q] = 1;                                          // region full: the query is re-run exactly
        }
        wpos = wpos + n < capw ? wpos + n : capw;
    };
    // the k-step of its item that this wave multiplies next / that the current step reads
    int kt_c = 0, kt_s = 0, qt_done = 0, t_done = 0;
    zero_acc();
    if (tid == 0) *stg_n = 0;                                 // (the first append is many barriers away)
    auto multiply_stage = [&](bool issue, int ibuf, int half) {
        multiply(issue, ibuf, half);
        if (++kt_c == KT) {
            STAMP(4);
            item_epilogue(qt_cur, t_cur, p_cur);
            zero_acc();
            STAMP(7);
            kt_c = 0;
            qt_done = qt_cur;         // (flushed after the next P1, when both groups have finished the item)
            t_done = t_cur;
            qt_cur = qt_nxt;          // (the issue cursor entered the next item AHEAD steps ago, and enters the one after it only later: KT > AHEAD)
            t_cur = t_nxt;
            p_cur = p_nxt;
        }
    };
    auto landed = [&](int s) {
        // stage s has landed (this wave's pieces); up to AHEAD - 1 younger stages stay in flight.  (The LDS-DMA of the per-item
        // constants is younger still: it can only make this wait stricter, never weaker.)
        const int rem = steps - 1 - s;
        if (rem >= 2) wait_vmcnt<2 * NI>();
        else if (rem == 1) wait_vmcnt<NI>();
        else wait_vmcnt<0>();
    };
    auto item_constants = [&](int s_now) {
        // after P1 of an item's first step: test parameters of its 128 queries (2 KiB) and constants of its 256 rows (4 KiB) go
        // to LDS by the same DMA path (by then every wave's current item is this one).  The late group's epilogue of the
        // PREVIOUS item (which reads spar / srow) ran between P0 and P1.  Three steps on they are older than everything a
        // counted wait leaves in flight, so they have landed before the item's epilogue (KT >= 4).  Both arrays are padded
        // to whole tiles with entries no pair can pass (init_state_kernel / bank16_kernel).  (Written-out DMA like the stages:
        // the compiler, seeing an LDS-DMA it cannot tell apart from the ring's, would drain the whole ring with vmcnt(0) in
        // front of the epilogue's reads of spar / srow.)
        if (kt_s == 0) {
            constexpr int QW = QT * 16 / 1024;           // waves that fetch the queries' parameters (1 KiB each); four more fetch the rows'
            const unsigned int l16b = (unsigned int)lane_now() * 16u;
            if (wave < QW) glds16_sbase((const char *)(qpar + (int64_t)qt_cur * QT) + wave * 1024, l16b, (char *)spar + wave * 1024);
            else if (wave < QW + 4) glds16_sbase((const char *)(rowp + (int64_t)t_cur * BT) + (wave - QW) * 1024, l16b, (char *)srow + (wave - QW) * 1024);
            // ... and the item finished one step ago (early group) / in this step's first phase (late group) is flushed
            if (STAGED && s_now > 0) flush_item(qt_done, t_done);
        } else if (kt_s == 1) {
            if (STAGED && tid == 0) *stg_n = 0;         // a barrier after the flush's reads, two before the next item's first append
        }
        kt_s = kt_s + 1 < KT ? kt_s + 1 : 0;
    };
    STAMP(-1);
#ifdef PF_CLOCK
    // -DPF_CLOCK (a diagnostic build of its own, no per-segment stamps): the clock the chip holds inside THIS kernel's loop =
    // delta s_memtime / delta s_memrealtime x 100 MHz, stamped once around the whole pass (MI355X_MICROARCH.md, DVFS item 6)
    const unsigned long long pfc_t0 = __builtin_amdgcn_s_memtime(), pfc_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    if (!late) {
        for (int s = 0; s < steps; ++s) {
            const bool issue = s + AHEAD < steps;
            const int ibuf = (s + AHEAD) & (NSTAGE - 1);
            landed(s);
            STAMP(0);
            __builtin_amdgcn_s_barrier();                                  // P0(s)
            STAMP(1);
            read_frags(s & (NSTAGE - 1));
            if (issue) {
                issue_half(ibuf, 0);
                issue_half(ibuf, 1);
            }
            STAMP(2);
            __builtin_amdgcn_s_barrier();                                  // P1(s)
            STAMP(3);
            item_constants(s);
            multiply_stage(false, 0, 0);
            STAMP(4);
        }
    } else {
        for (int s = 0; s < steps; ++s) {
            const bool issue = s + AHEAD < steps;
            const int ibuf = (s + AHEAD) & (NSTAGE - 1);
            landed(s);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // the fragment reads of stage s-1 are out of its buffer
            STAMP(0);
            __builtin_amdgcn_s_barrier();                                  // P0(s)
            STAMP(1);
            if (s > 0) multiply_stage(false, 0, 0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // staged candidates of a finished item are in LDS
            STAMP(4);
            __builtin_amdgcn_s_barrier();                                  // P1(s)
            STAMP(3);
            item_constants(s);
            read_frags(s & (NSTAGE - 1));
            if (issue) {
                issue_half(ibuf, 0);
                issue_half(ibuf, 1);
            }
            STAMP(2);
        }
        multiply_stage(false, 0, 0);                                       // the last stage (+ its item epilogue)
    }
    if (STAGED) {
        __syncthreads();                                                    // both groups are done with the last item
        flush_item(qt_done, t_done);
        if (tid == 0) wg_count[blockIdx.x] = wpos;
    }
#ifdef PF_CLOCK
    {
        const unsigned long long pfc_t1 = __builtin_amdgcn_s_memtime(), pfc_r1 = __builtin_amdgcn_s_memrealtime();
        if (tid == 0) {
            atomicAdd(dbg + 20, pfc_t1 - pfc_t0);
            atomicAdd(dbg + 21, pfc_r1 - pfc_r0);
            atomicAdd(dbg + 22, (unsigned long long)steps);
            atomicAdd(dbg + 23, 1ull);
        }
    }
#endif
#ifdef PF_STAMP
    if (lane == 0)
        for (int i = 0; i < 8; ++i) atomicAdd(dbg + (late ? 8 : 0) + i, (unsigned long long)seg[i]);
    if (lane == 0 && wave == 0) atomicAdd(dbg + 16, (unsigned long long)steps);
    if (lane == 0 && wave == 0) atomicAdd(dbg + 17, (unsigned long long)my_items);
#endif
}

// ---- the workgroups' candidate regions -> the per-query lists (slot from the query's counter; a count past `cap` marks the
// query as overflowed in select_kernel).  grid = (chunks, PF_GRID)
__global__ __launch_bounds__(256) void bucket_kernel(const uint4 *__restrict__ wg_list, const int *__restrict__ wg_count, int capw,
                                                     int cap, int *__restrict__ cnt, int *__restrict__ cand_i,
                                                     float *__restrict__ cand_d) {
    const int n = wg_count[blockIdx.y];
    const uint4 *src = wg_list + (int64_t)blockIdx.y * capw;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const uint4 c = src[e];
        const int q = (int)c.x;
        const int pos = atomicAdd(cnt + q, 1);
        if (pos < cap) {
            cand_i[(int64_t)q * cap + pos] = (int)c.y;
            cand_d[(int64_t)q * cap + pos] = __uint_as_float(c.z);
        }
    }
}

// the query's row of the candidate test's A operand (see prefilter_kernel): {-a, c (raised), -b, 0}
__device__ __forceinline__ float4 test_row(float a, float b, float c) { return make_float4(-a, c * (1.0f + 0x1p-19f), -b, 0.f); }

// ---- between phases: new threshold, compaction; last phase: pick the candidates to re-score ---------------------------------
__device__ __forceinline__ unsigned int orderable(float f) {
    const unsigned int u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float unorderable(unsigned int o) { return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// key of the kth largest (1-based, kth <= n) among keys[0..n) (LDS); 4 radix passes of 8 bits.  All threads return it.
__device__ unsigned int radix_kth_largest(const unsigned int *keys, int n, int kth, int *hist, int tid, int nthreads) {
    unsigned int prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = tid; b < 256; b += nthreads) hist[b] = 0;
        __syncthreads();
        for (int e = tid; e < n; e += nthreads) {
            const unsigned int kx = keys[e];
            if ((kx & mask) == prefix) atomicAdd(&hist[(kx >> shift) & 255], 1);
        }
        __syncthreads();
        radix_pick_bin(hist, kth, tid);
        __syncthreads();
        const int b = hist[256];
        kth = hist[257];
        prefix |= (unsigned int)b << shift;
        mask |= 255u << shift;
        __syncthreads();
    }
    return prefix;
}

// one workgroup (256 threads) per query.  state[q] = {tau (current threshold), overflow flag as float, -, -}
// final == 0: tau <- max(tau, k-th largest L); keep the candidates with U >= tau; write the test parameters of the next phase.
// final == 1: sel_i[q][0..nsel) <- the (up to) RESCORE_MAX candidates with the largest U; bound[q] = largest U NOT selected
//             (-inf when every candidate is selected).
// SEL (a search under a selection): rowp is the masked copy, and a take-all slice stores pairs of deselected rows -- they are told by
// the sentinel's third component, 0 where every row that counts holds a power of two, so a selected row whose constants hold a NaN
// keeps the treatment it has without a selection.  Without SEL none of this is compiled: the unselected search's kernel.
template <bool SEL>
__global__ __launch_bounds__(256) void select_kernel(int Q, int k, int cap, float eps, const float4 *__restrict__ qbase,
                                                     const float4 *__restrict__ rowp, const float *__restrict__ xn, int *__restrict__ cnt,
                                                     int *__restrict__ cand_i, float *__restrict__ cand_d,
                                                     float4 *__restrict__ qpar, float *__restrict__ tau_q, int *__restrict__ overflow,
                                                     int final, int *__restrict__ sel_i, int *__restrict__ nsel,
                                                     float *__restrict__ bound) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned int *kL = (unsigned int *)smem;                  // [cap] orderable(L)
    unsigned int *kU = kL + cap;                              // [cap] orderable(U)
    int *hist = (int *)(kU + cap);                            // [258]
    int *scan = hist + 260;                                   // [8]
    const int tid = threadIdx.x, q = blockIdx.x;
    const int raw = cnt[q];
    if (raw > cap && tid == 0) overflow[q] = 1;
    const int n = raw < cap ? raw : cap;
    const float4 qb = qbase[q];                               // {qn', eps_a ||q'||, 2^-f, qn}
    int *ci = cand_i + (int64_t)q * cap;
    float *cd = cand_d + (int64_t)q * cap;
    const float inv_sf = 1.0f / qb.z;                         // 2^f (exact)
    for (int e = tid; e < n; e += 256) {
        const float4 rp = rowp[ci[e]];                        // {xn', ||x'||, 2^-e, 0}
        if (SEL && rp.z == 0.f) {
            // the sentinel of a deselected row (or of a padding row of the last tile): only a take-all slice stores such pairs.
            // Key 0 is below orderable(-inf) = 0x007fffff, the least key a row that counts can have: never kept, never counted
            // (and xn is not read: it ends at row N)
            kL[e] = 0u;
            kU[e] = 0u;
            continue;
        }
        const float den = fmaf(qb.w, xn[ci[e]], eps);
        const float sc = inv_sf * (1.0f / rp.z);              // 2^(e+f), exact
        const float err = qb.y * rp.y;
        const float hi = (cd[e] + err) * sc, lo = (cd[e] - err) * sc;
        float U = hi / den, L = lo / den;
        U = U >= 0.f ? U * (1.0f + 0x1p-21f) : U * (1.0f - 0x1p-21f);
        L = L >= 0.f ? L * (1.0f - 0x1p-21f) : L * (1.0f + 0x1p-21f);
        if (!(U == U)) U = INFINITY;                          // never drop what cannot be bounded
        if (!(L == L)) L = -INFINITY;
        kL[e] = orderable(L);
        kU[e] = orderable(U);
    }
    __syncthreads();
    float tau = tau_q[q];
    if (!final) {
        if (n >= k) {
            const unsigned int kth = radix_kth_largest(kL, n, k, hist, tid, 256);
            if (!SEL || kth != 0u) tau = fmaxf(tau, unorderable(kth));   // (key 0: fewer than k rows that count -- no k-th lower bound yet)
        }
        // compaction: survivors keep their relative order (deterministic lists)
        const unsigned int tk = orderable(tau);
        int kept = 0;
        for (int base = 0; base < n; base += 256) {
            const int e = base + tid;
            const bool keep = e < n && kU[e] >= tk;
            int idx_v = 0;
            float d_v = 0.f;
            if (keep) { idx_v = ci[e]; d_v = cd[e]; }
            const unsigned long long m = __ballot(keep);
            if ((tid & 63) == 0) scan[tid >> 6] = __builtin_popcountll(m);
            __syncthreads();
            int off = kept;
            for (int w = 0; w < (tid >> 6); ++w) off += scan[w];
            const int tot = scan[0] + scan[1] + scan[2] + scan[3];
            off += __builtin_popcountll(m & ((1ull << (tid & 63)) - 1));
            __syncthreads();                                   // reads of this batch precede writes (off <= e)
            if (keep) { ci[off] = idx_v; cd[off] = d_v; }
            kept += tot;
            __syncthreads();
        }
        if (tid == 0) {
            cnt[q] = kept;
            tau_q[q] = tau;
            // test parameters of the next phase (see prefilter_kernel); tau = -inf -> everything passes
            const float t = tau > -3.0e38f ? tau : -3.0e38f;
            float a = t * qb.x, b = t * eps * qb.z;
            a -= fabsf(a) * 0x1p-19f;
            b -= fabsf(b) * 0x1p-19f;
            if (!(a > -3.0e38f)) a = -3.0e38f;
            qpar[q] = test_row(a, b, qb.y);
        }
        return;
    }
    // ---- final.  Only candidates whose interval reaches the k-th largest LOWER bound L_k can be among the k best: at least k
    // candidates have an exact score >= L_k (each score is >= its own L), so the k-th best exact score is >= L_k, and whoever
    // has U < L_k is out.  When those needed fit the re-score quota (the rule on embedding-like data: k plus a few dozen), only
    // they are re-scored and the answer is certified by construction (bound = -inf) -- half the exact stage's HBM traffic.
    int *so = sel_i + (int64_t)q * RESCORE_MAX;
    // rows that count (a take-all slice that is also the last one leaves the sentinel rows in the list, see above)
    int live = n;
    if (SEL) {
        if (tid == 0) hist[0] = 0;
        __syncthreads();
        int mine = 0;
        for (int e = tid; e < n; e += 256) mine += kU[e] != 0u ? 1 : 0;
        if (mine) atomicAdd(&hist[0], mine);
        __syncthreads();
        live = hist[0];
        __syncthreads();
    }
    if (live >= k && live > 0) {
        const unsigned int lk = radix_kth_largest(kL, n, k, hist, tid, 256);
        if (unorderable(lk) > -INFINITY) {            // (k finite lower bounds exist; U = +inf / NaN-turned-inf rows always qualify)
            if (tid == 0) hist[0] = 0;
            __syncthreads();
            int mine = 0;
            for (int e = tid; e < n; e += 256) mine += kU[e] >= lk ? 1 : 0;
            if (mine) atomicAdd(&hist[0], mine);
            __syncthreads();
            const int need = hist[0];
            __syncthreads();
            if (need <= RESCORE_MAX) {
                if (tid == 0) hist[0] = 0;
                __syncthreads();
                for (int e = tid; e < n; e += 256)
                    if (kU[e] >= lk) so[atomicAdd(&hist[0], 1)] = ci[e];
                if (tid == 0) { nsel[q] = need; bound[q] = -INFINITY; }
                return;
            }
        }
    }
    // ---- otherwise: the RESCORE_MAX largest U
    if (live <= RESCORE_MAX) {
        if (!SEL || live == n) {
            for (int e = tid; e < n; e += 256) so[e] = ci[e];
        } else {
            if (tid == 0) hist[0] = 0;
            __syncthreads();
            for (int e = tid; e < n; e += 256)
                if (kU[e] != 0u) so[atomicAdd(&hist[0], 1)] = ci[e];
        }
        if (tid == 0) { nsel[q] = live; bound[q] = -INFINITY; }
        return;
    }
    const unsigned int uk = radix_kth_largest(kU, n, RESCORE_MAX, hist, tid, 256);   // RESCORE_MAX-th largest U (live > RESCORE_MAX: uk != 0)
    // strictly larger first, then ties of uk in list order until the quota is full; bound = uk if anything with U <= uk is left
    if (tid == 0) { hist[0] = 0; hist[1] = 0; }
    __syncthreads();
    for (int e = tid; e < n; e += 256)
        if (kU[e] > uk) so[atomicAdd(&hist[0], 1)] = ci[e];
    __syncthreads();
    const int above = hist[0];
    for (int e = tid; e < n; e += 256)
        if (kU[e] == uk) {
            const int p = atomicAdd(&hist[1], 1);
            if (above + p < RESCORE_MAX) so[above + p] = ci[e];
        }
    __syncthreads();
    if (tid == 0) {
        nsel[q] = RESCORE_MAX;
        bound[q] = unorderable(uk);                            // every candidate left out has U <= uk
    }
}

// ---- stage 2: exact scores of the selected candidates, final order, acceptance test ------------------------------------------
__device__ __forceinline__ float finish_score(float dot, float qn, float xn, float eps) {
    const float den = fmaf(qn, xn, eps);
    const float s = __fdiv_rn(dot, den);
    return s == s ? s : -INFINITY;
}

// four consecutive elements of a bank row as fp32: the fp32 bank's own, or a resident fp16 bank's widened exactly
__device__ __forceinline__ float4 row4(const float *x) { return *(const float4 *)x; }
__device__ __forceinline__ float4 row4(const half_t *x) {
    typedef __attribute__((ext_vector_type(4))) _Float16 half4;
    const half4 h = *(const half4 *)x;
    return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
}

__device__ __forceinline__ float4 row4(const bf16_t *x) {
    const uint2 raw = *(const uint2 *)x;
    return make_float4(__uint_as_float(raw.x << 16), __uint_as_float(raw.x & 0xFFFF0000u), __uint_as_float(raw.y << 16),
                       __uint_as_float(raw.y & 0xFFFF0000u));
}

// one workgroup (256 threads) per query; thread c owns candidate c: the contract's fma chain over d = 0..D-1
// FEW (a search under a selection, which may hold fewer than k rows): fewer than k candidates are an answer, not a reason to re-run
template <typename X, bool FEW>
__device__ __forceinline__ void rescore_body(const float *__restrict__ tw, const float *__restrict__ qn,
                                             const X *__restrict__ bank, const float *__restrict__ xn, int Q, int D,
                                             int k, float eps, int64_t idx_offset, const int *__restrict__ sel_i,
                                             const int *__restrict__ nsel, const float *__restrict__ bound,
                                             const int *__restrict__ overflow, float *__restrict__ out_s,
                                             int64_t *__restrict__ out_i, int *__restrict__ redo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sq = (float *)smem;                                // [D] weighted query
    float *ss = sq + D;                                       // [RESCORE_MAX] exact scores
    int *si = (int *)(ss + RESCORE_MAX);                      // [RESCORE_MAX] rows
    const int tid = threadIdx.x, q = blockIdx.x;
    const int n = nsel[q];
    for (int d = tid; d < D; d += 256) sq[d] = tw[(int64_t)q * D + d];
    __syncthreads();
    float sc = -INFINITY;
    int row = 0x7fffffff;
    if (tid < n) {
        row = sel_i[(int64_t)q * RESCORE_MAX + tid];
        const X *x = bank + (int64_t)row * D;
        float acc = 0.f;
        for (int d = 0; d < D; d += 4) {      // explicit fmaf only: nothing here for the compiler to contract
            const float4 v = row4(x + d);
            acc = fmaf(sq[d], v.x, acc);
            acc = fmaf(sq[d + 1], v.y, acc);
            acc = fmaf(sq[d + 2], v.z, acc);
            acc = fmaf(sq[d + 3], v.w, acc);
        }
        sc = finish_score(acc, qn[q], xn[row], eps);
    }
    ss[tid] = sc;
    si[tid] = row;
    __syncthreads();
    // rank by counting: (score desc, row asc)
    int rank = 0;
    if (tid < n) {
        for (int e = 0; e < n; ++e) {
            const float s2 = ss[e];
            const int r2 = si[e];
            rank += (s2 > sc || (s2 == sc && r2 < row)) ? 1 : 0;
        }
        if (rank < k && !(FEW && n < k && !(sc > -INFINITY))) {
            out_s[(int64_t)q * k + rank] = sc;
            out_i[(int64_t)q * k + rank] = idx_offset + row;
        }
        if (rank == k - 1) {
            // accepted iff the k-th best exact score beats (strictly) the upper bound of everything that was not re-scored
            redo[q] = (overflow[q] || !(sc > bound[q])) ? 1 : 0;
        }
    }
    if (n < k) {                                              // fewer candidates than k (tiny shard, NaN rows): the exact kernel decides
        // FEW: the answer stands when every candidate was re-scored -- the rows that score above -inf in order, then the (-inf, -1)
        // tail.  A row that scores -inf (a NaN in it) is not returned, as in the token search that serves the other selections: stage 1
        // does not keep every such row of an fp32 bank, so returning those it happens to keep would depend on the schedule.
        const int have = FEW ? __syncthreads_count(tid < n && sc > -INFINITY) : n;
        if (tid == 0) redo[q] = !FEW || overflow[q] || bound[q] > -INFINITY ? 1 : 0;
        for (int e = have + tid; e < k; e += 256) {
            out_s[(int64_t)q * k + e] = -INFINITY;
            out_i[(int64_t)q * k + e] = -1;
        }
    }
}

#define RESCORE_PARAMS(X)                                                                                                     \
    const float *__restrict__ tw, const float *__restrict__ qn, const X *__restrict__ bank, const float *__restrict__ xn, int Q,   \
        int D, int k, float eps, int64_t idx_offset, const int *__restrict__ sel_i, const int *__restrict__ nsel,                  \
        const float *__restrict__ bound, const int *__restrict__ overflow, float *__restrict__ out_s, int64_t *__restrict__ out_i, \
        int *__restrict__ redo
template <bool FEW>
__global__ __launch_bounds__(256) void rescore_kernel(RESCORE_PARAMS(float)) {
    rescore_body<float, FEW>(tw, qn, bank, xn, Q, D, k, eps, idx_offset, sel_i, nsel, bound, overflow, out_s, out_i, redo);
}
// the resident fp16 bank's rows, widened element by element: same chain, same bits as rescore_kernel on the widened bank
template <bool FEW>
__global__ __launch_bounds__(256) void rescore_lp_kernel(RESCORE_PARAMS(half_t)) {
    rescore_body<half_t, FEW>(tw, qn, bank, xn, Q, D, k, eps, idx_offset, sel_i, nsel, bound, overflow, out_s, out_i, redo);
}
// ... and a resident bf16 bank's
template <bool FEW>
__global__ __launch_bounds__(256) void rescore_bf_kernel(RESCORE_PARAMS(bf16_t)) {
    rescore_body<bf16_t, FEW>(tw, qn, bank, xn, Q, D, k, eps, idx_offset, sel_i, nsel, bound, overflow, out_s, out_i, redo);
}
#undef RESCORE_PARAMS

__global__ void init_state_kernel(int Q, int Q_padded, const float *__restrict__ thr0, const float4 *__restrict__ qbase, float eps,
                                  float4 *__restrict__ qpar, float *__restrict__ tau_q, int *__restrict__ cnt,
                                  int *__restrict__ overflow, int first_rows, float scale_lo, float scale_hi) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) {
        if (q < Q_padded) qpar[q] = make_float4(NAN, NAN, NAN, NAN);   // padding of the last query tile: t = NaN, no pair passes
        return;
    }
    const float tau = thr0 ? thr0[q] : -INFINITY;
    tau_q[q] = tau;
    cnt[q] = thr0 ? 0 : first_rows;          // without a floor the first slice is taken whole: slot = row (prefilter_kernel<true>)
    const float4 qb = qbase[q];
    // a query whose scale hit the clamp (largest |t w| below ~2^-112) has an fp16 image outside the error bound's
    // assumptions: answered by the exact kernel (redo), never silently by this path
    // (scale_lo = 0, scale_hi = 2^126: that rule.  The bf16 search's bound asks more of the scale: file header)
    overflow[q] = qb.z >= scale_hi || qb.z <= scale_lo ? 1 : 0;
    const float t = tau > -3.0e38f ? tau : -3.0e38f;
    float a = t * qb.x, b = t * eps * qb.z;
    a -= fabsf(a) * 0x1p-19f;
    b -= fabsf(b) * 0x1p-19f;
    if (!(a > -3.0e38f)) a = -3.0e38f;
    qpar[q] = test_row(a, b, qb.y);
}

struct Workspace {
    half_t *qh, *ql;
    float4 *qbase, *qpar;
    float *tau, *bound, *cand_d;
    int *cnt, *overflow, *cand_i, *sel_i, *nsel, *wg_count;
    uint4 *wg_list;
    int capw;
};
inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }
int64_t carve(char *base, int Q, int D, int cap, Workspace *w) {
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        char *p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    };
    char *p;
    const int64_t Qp = (Q + QPAD - 1) / QPAD * QPAD;          // the fp16 query images are padded to whole tiles
    p = take(Qp * D * 2); if (w) w->qh = (half_t *)p;
    p = take(Qp * D * 2); if (w) w->ql = (half_t *)p;
    p = take((int64_t)Q * 16); if (w) w->qbase = (float4 *)p;
    p = take(Qp * 16); if (w) w->qpar = (float4 *)p;
    p = take((int64_t)Q * 4); if (w) w->tau = (float *)p;
    p = take((int64_t)Q * 4); if (w) w->bound = (float *)p;
    p = take((int64_t)Q * 4); if (w) w->cnt = (int *)p;
    p = take((int64_t)Q * 4); if (w) w->overflow = (int *)p;
    p = take((int64_t)Q * 4); if (w) w->nsel = (int *)p;
    p = take((int64_t)Q * RESCORE_MAX * 4); if (w) w->sel_i = (int *)p;
    p = take((int64_t)Q * cap * 4); if (w) w->cand_i = (int *)p;
    p = take((int64_t)Q * cap * 4); if (w) w->cand_d = (float *)p;
    // stage 1 writes each workgroup's candidates to a region of its own: a few hundred candidates per query and phase in all,
    // dealt evenly over the workgroups; a full region flags the queries it had to drop
    const int capw = Q * 4 > 8192 ? Q * 4 : 8192;
    p = take((int64_t)PF_GRID * capw * 16); if (w) { w->wg_list = (uint4 *)p; w->capw = capw; }
    p = take((int64_t)PF_GRID * 4); if (w) w->wg_count = (int *)p;
    return off;
}

}  // namespace

extern "C" int skyemb_topk_prefilter_applicable(int Q, int64_t N, int D, int k) { return pfplan::rows_shape_ok(Q, N, D, k); }

extern "C" int64_t skyemb_bank16_bytes(int64_t N, int D) { return ceil_div64(N, BT) * BT * D * 2; }   // whole tiles of BT rows

extern "C" int64_t skyemb_bank16_rowp_rows(int64_t N) { return ceil_div64(N, BT) * BT; }

extern "C" int skyemb_bank16_prepare(const float *bank, const float *xn, int64_t N, int D, void *bank16, float *rowp, void *stream) {
    SKY_CHECK_ARG(bank && xn && bank16 && rowp && N > 0 && D > 0 && D % 4 == 0, "skyemb_bank16_prepare: bad arguments");
    const int64_t padded = skyemb_bank16_rowp_rows(N);
    hipLaunchKernelGGL(bank16_kernel, dim3((unsigned)ceil_div64(padded, 4)), dim3(256), 0, (hipStream_t)stream, bank, xn, N, D,
                       (half_t *)bank16, (float4 *)rowp, padded);
    SKY_LAUNCH_CHECK("skyemb_bank16_prepare");
    return 0;
}

extern "C" double skyemb_topk_prefilter_eps_a(int D, int lo, int resident) { return eps_a_of(D, lo != 0, resident != 0); }

#define RESIDENT_DTYPE_MSG "must be SKYEMB_BF16 (0) or SKYEMB_F16 (2), got %d"
extern "C" double skyemb_topk_prefilter_eps_a_resident(int D, int lo, int dtype) {
    return dtype == SKYEMB_BF16 ? eps_a_bf16_of(D, lo != 0) : eps_a_of(D, lo != 0, true);
}

static int resident_rowp(const char *who, bool bf, const void *bank16, const float *xn, int64_t N, int D, float *rowp, void *tail, void *stream) {
    SKY_CHECK_ARG(bank16 && xn && rowp && N > 0 && D > 0 && D % BK == 0, "%s: bad arguments", who);
    SKY_CHECK_ARG(N % BT == 0 || tail, "%s: N = %lld is no whole number of %d-row tiles: a tail tile [%d, D] is needed", who, (long long)N, BT, BT);
    SKY_CHECK_ARG(aligned16(bank16) && aligned16(tail), "%s: the bank and the tail tile must be 16-byte aligned", who);
    const int64_t padded = skyemb_bank16_rowp_rows(N);
    const dim3 grid((unsigned)ceil_div64(padded, 4));
    // fp16: one set of row constants serves both variants: the smaller eps_a (hi + lo) gives the larger, always valid, term
    const float sub_scale = (float)(0x1p-14 / eps_a_of(D, true, true) * (1.0 + 1e-6));
    if (bf) hipLaunchKernelGGL(bankbf16_rowp_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short *)bank16, xn, N, D,
                               (float4 *)rowp, padded, N % BT ? (unsigned short *)tail : nullptr, N / BT * BT);
    else hipLaunchKernelGGL(bank16_rowp_lp_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const half_t *)bank16, xn, N, D, (float4 *)rowp,
                            padded, N % BT ? (half_t *)tail : nullptr, N / BT * BT, sub_scale);
    SKY_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int skyemb_bank16_rowp_lp(const void *bank16, const float *xn, int64_t N, int D, float *rowp, void *tail, void *stream) {
    return resident_rowp("skyemb_bank16_rowp_lp", false, bank16, xn, N, D, rowp, tail, stream);
}

extern "C" int skyemb_resident_rowp(const void *bank16, int dtype, const float *xn, int64_t N, int D, float *rowp, void *tail, void *stream) {
    SKY_CHECK_ARG(sky_is_lp(dtype), "skyemb_resident_rowp: dtype " RESIDENT_DTYPE_MSG, dtype);
    return resident_rowp(dtype == SKYEMB_F16 ? "skyemb_bank16_rowp_lp" : "skyemb_resident_rowp", dtype == SKYEMB_BF16, bank16, xn, N, D, rowp, tail,
                         stream);
}

extern "C" int64_t skyemb_topk_prefilter_ws_bytes(int Q, int D, int k) { return carve(nullptr, Q, D, pfplan::cap_of(k), nullptr); }

// Test and diagnostic hook (host arithmetic only, nothing is launched): where carve puts each array of the workspace.  carve
// itself is run over a base that is only ever subtracted again -- never read or written -- so the two cannot drift.
// out[0 .. 13]: byte offsets of qh, ql, qbase, qpar, tau, bound, cnt, overflow, nsel, sel_i, cand_i, cand_d, wg_list, wg_count
// (carve's order); out[14] = cap (slots of a query's candidate list), out[15] = capw (entries of a workgroup's region).
extern "C" int skyemb_topk_prefilter_ws_layout(int Q, int D, int k, int64_t *out, int n) {
    constexpr int FIELDS = 14;
    SKY_CHECK_ARG(out && n == FIELDS + 2, "skyemb_topk_prefilter_ws_layout: out must hold %d values (14 offsets, cap, capw), got n = %d",
                  FIELDS + 2, n);
    SKY_CHECK_ARG(Q >= 1 && D >= 1 && k >= 1, "skyemb_topk_prefilter_ws_layout: bad shape (Q=%d D=%d k=%d)", Q, D, k);
    const int cap = pfplan::cap_of(k);
    alignas(256) static char anchor[256];                      // an address to count from: carve adds offsets to it, nothing more
    Workspace w;
    carve(anchor, Q, D, cap, &w);
    const char *at[FIELDS] = {(const char *)w.qh,    (const char *)w.ql,       (const char *)w.qbase, (const char *)w.qpar,   (const char *)w.tau,
                              (const char *)w.bound, (const char *)w.cnt,      (const char *)w.overflow, (const char *)w.nsel, (const char *)w.sel_i,
                              (const char *)w.cand_i, (const char *)w.cand_d,  (const char *)w.wg_list, (const char *)w.wg_count};
    for (int i = 0; i < FIELDS; ++i) out[i] = (int64_t)((uintptr_t)at[i] - (uintptr_t)anchor);
    out[FIELDS] = cap;
    out[FIELDS + 1] = w.capw;
    return 0;
}

// ---- the same searches under a selection of the bank's rows ---------------------------------------------------------------------
extern "C" int skyemb_prefilter_select_prepare(const uint32_t *words, int64_t N, const float *rowp, float *rowp_sel, int *tiles,
                                               int *info, void *stream) {
    SKY_CHECK_ARG(words && rowp && rowp_sel && tiles && info, "skyemb_prefilter_select_prepare: null argument");
    SKY_CHECK_ARG(N > 0 && N < (1ll << 31), "skyemb_prefilter_select_prepare: N = %lld, expected 1 .. 2^31 - 1 rows", (long long)N);
    const int64_t padded = skyemb_bank16_rowp_rows(N);
    hipLaunchKernelGGL(select_rowp_kernel, dim3((unsigned)(padded / 256)), dim3(256), 0, (hipStream_t)stream, words, (const float4 *)rowp,
                       N, padded, (float4 *)rowp_sel);
    hipLaunchKernelGGL(select_tiles_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, words, ceil_div64(N, 32), (int)(padded / BT), tiles,
                       info);
    SKY_LAUNCH_CHECK("skyemb_prefilter_select_prepare");
    return 0;
}

// ---- Patch-token banks: the same two stages over a resident 16-bit token bank [N, P, D], per-image combine min | max -------------------
// (skyemb_cosine_topk_tokens_prefiltered).  Stage 1 is prefilter_kernel<.., TOK> over the flat [N P, D] rows with the row constants of
// skyemb_resident_rowp: an image can reach a query's top-k under 'min' only if EVERY one of its P rows passes the row test
// (min_i e_i >= tau implies U_i >= tau for every i), under 'max' only if SOME row passes -- the fold of the pass bits in the item
// epilogue.  P divides 64, so an image never leaves one wave's 64-row strip, and the N P rows are whole images: the tail tile's
// padding rows belong to none.  A row the bound gives up on passes every test, so its image is decided by stage 2 under both
// combines (under 'min' when its other rows pass too -- and if they do not, the image is out whatever that row scores).
// tau_q is EXACT at all times: the k-th best exact combined score over the images decided so far (or the caller's floor, itself the
// k-th best of a sample).  After every slice of tiles token_rescore_kernel re-scores each candidate image of the slice -- P token
// scores by the contract's chain on the widened rows, finish_score, then fminf / fmaxf over the tokens (-inf for a NaN score, as the
// grouped search combines them) --, merges them into the query's running list of at most k (score desc, image asc: one 64-bit key,
// so ties need no second rule) and publishes the new tau_q into qpar.  Every image that passes stage 1 is re-scored, so nothing is
// left to certify: the only failure is a full candidate list or staging region, which flags the query (redo) for the grouped search.
// A query whose eps_a ||q'|| is 0 or not finite (a zero query: 0 * inf in the test of an unboundable row) is flagged as well.
//
// ---- combine 'mean' (skyemb_token_mean_pool / skyemb_cosine_topk_tokens_mean_prefiltered) ---------------------------------------------
// The mean of an image's P token cosines is, up to eps and fp32 rounding, ONE dot product with the image's pooled unit tokens, so
// stage 1 is the ROW search's pass (prefilter_kernel without TOK: a row is an image) over a derived 16-bit image [N, D], P times
// fewer rows than the bank; stage 2 is token_rescore_kernel with the mean fold, and the threshold and list discipline is that of
// min / max above.  Notation, per image i and query q (reals unless fl() is written): x_p the widened token rows, n_p = xn[i P + p],
// u_p = x_p / n_p, m = (1/P) sum_p u_p, r_p = tw . x_p, N_q = ||q'||_2 with q' = tw 2^-f, qn' = qn 2^-f, and the per-image constants
//   c1 = mean_p ||u_p||_2        c2 = mean_p ||u_p||_2 / n_p         (c1 = 1 under unit weights)
// Only the plain Cauchy-Schwarz |r_p| <= ||tw||_2 ||x_p||_2 is used, never |r_p| <= qn n_p: nothing is assumed of the weights (they
// may be negative or zero) beyond what makes n_p a positive finite number -- point (e) of the design is met by not needing it.
//  (d) contract score of a token  s_p = fl(chain_p / fl(qn n_p + eps)), eps >= 0:  |chain_p - r_p| <= 1.01 D 2^-24 ||tw|| ||x_p||, the fma
//      and the division round once each, so  |s_p - r_p / (qn n_p + eps)| <= (1.02 D + 2.02) 2^-24 rho_p,  rho_p = ||tw|| ||u_p|| / qn.
//      The eps term: r_p / (qn n_p + eps) = r_p / (qn n_p) (1 - eps / (qn n_p + eps)) <= r_p / (qn n_p) + rho_p eps / (qn n_p).
//      The combine's P - 1 adds (the first, 0 + s_0, is exact) err by <= 1.01 (P - 1) 2^-24 sum |s_p|, |s_p| <= rho_p (1 + 2^-20); the
//      division by float(P), a power of two, is exact.  Together
//        qn' mean <= q' . m + N_q c1 (1.02 D + 1.02 P + 2) 2^-24 + N_q c2 eps / qn.
//  (c) the kernel forms m_fl = fl(fl(sum_p fl(x_p / n_p)) / P): P divisions, P - 1 adds in token order, one exact scale per element:
//      ||m_fl - m|| <= 1.01 P 2^-24 c1 (triangle inequality over the tokens).
//  (b) + (a) m' = m_fl 2^-e with the largest element in [2^13, 2^14) is rounded to 16 bits and multiplied by the matrix cores: this is
//      the situation of the fp32 bank's fp16 image, |dot^ - q' . m'| <= eps_m N_q ||m'||,
//        fp16: eps_m = eps_a_of(D, lo, resident = false)  (row rounding 2^-11 and both operands' subnormals included)
//        bf16: eps_m = (lo ? 2^-9 + 2^-17 : 2^-8 + 2^-17) + 6.06 D 2^-24 + D 2^-37 -- the resident bf16 bound with the row's own rounding
//              2^-9 and its cross terms added; elements of m' below 2^-40 are stored as zero (<= sqrt(D) 2^-53 ||m'||, in the last term,
//              which has doubled), so every nonzero element is >= 2^-40: condition (R).
// Hence, with kappa = (1.02 D + 2.03 P + 4) 2^-24 (the +2 on top: subnormal roundings of chain, score and mean, <= 2^-100 of the rest
// under the windows below),
//     qn' 2^-e mean  <=  dot^ + eps_m N_q [ ||m'|| + (kappa / eps_m) c1 2^-e ] + (N_q eps / qn) c2 2^-e      =: qn' 2^-e U
// and the image is a candidate iff  t = dot^ - a R0 + c R1 + g R2 >= 0  -- the test instruction of prefilter_kernel as it stands, with
//     rowp[i] = {R0, R1, R2, 0} = {2^-e, ||m'|| + (kappa / eps_m) c1 2^-e, c2 2^-e, 0}  (norms and constants rounded up)
//     qpar[q] = {-a, c, g, 0},  a = tau qn' (lowered),  c = eps_m N_q (raised),  g = N_q eps / qn (raised)
// (kappa / eps_m uses the SMALLER eps_m, hi + lo, so one set of row constants serves both variants.)  U - mean is eps_m c1-ish in
// cosine units under unit weights: of the order of eps_a, as for the row search.
// An image is UNBOUNDABLE -- zeros in the pooled row and the constants {0, inf, 1, 0}: a candidate of every query, decided by stage
// 2 -- when a token has an inf / NaN element (bf16: a nonzero element outside [2^-60, 2^120)), a norm n_p outside [2^-40, 2^40] (zero,
// inf and NaN included), ||u_p|| outside [2^-20, 2^20]; when 0 < max |m_fl| < 2^-40; or when R1 or R2 reach 2^60.  Inside these windows
// no intermediate of the kernel overflows or underflows, and c R1, g R2 stay finite, so t is never NaN for a boundable image.
// A query is flagged (redo: the grouped search answers it) by the rules of min / max and also when qn is outside [2^-20, 2^20], its
// scale 2^-f outside [2^-34, 2^34], eps is negative or not finite, c or g reach 2^60, or a = tau qn' is not finite.
namespace {

constexpr int TOK_KMAX = RESCORE_MAX;      // the running list of a query: at most k <= TOK_KMAX images
constexpr int TOK_MIN = 0, TOK_MAX = 1, TOK_MEAN = 2;      // the fold of token_rescore_kernel

__host__ __device__ inline double eps_m_of(int D, bool lo, bool bf) {
    if (bf) return (lo ? 0x1p-9 + 0x1p-17 : 0x1p-8 + 0x1p-17) + 6.06 * D * 0x1p-24 + D * 0x1p-37;
    return eps_a_of(D, lo, false);
}
inline double kappa_of(int D, int P) { return (1.02 * D + 2.03 * P + 4.0) * 0x1p-24; }

// the query's row of the test's A operand under 'mean' (see above); *bad: the query leaves the bound's windows
__device__ __forceinline__ float4 mean_test_row(float tau, float4 qb, float gfac, bool *bad) {
    const float t = tau > -3.0e38f ? tau : -3.0e38f;
    float a = t * qb.x;
    a -= fabsf(a) * 0x1p-19f;
    if (!(a > -3.0e38f)) a = -3.0e38f;
    const float g = __fdiv_rn(qb.y * gfac, qb.w) * (1.0f + 0x1p-19f);      // N_q eps / qn: gfac = eps / eps_m, raised on the host
    *bad = !(a < INFINITY) || !(g >= 0.f && g < 0x1p60f) || !(qb.y < 0x1p60f);
    return test_row(a, -g, qb.y);
}

// ---- Weighted MSE (skyemb_token_mse_rowp / skyemb_distance_topk_tokens_prefiltered): the distance contract's MSE over the same bank ----
// Contract (include/skyemb.h, distance_chain.h): dist = (1/D) sum_d c_d (x_d - t_d)^2, c = fp32(w / sum w) shared by all queries, every
// operation rounded on its own, 16 partial sums / 4 folds / one division; keys are key = -dist, so distance 'min' is the key-space
// MAX fold (an image is a candidate when SOME token can reach the threshold) and distance 'max' the MIN fold (EVERY token must).
// In real arithmetic  D dist = A_q + B_r - 2 G,  A_q = sum c_d t_d^2,  B_r = sum c_d x_d^2,  G = sum (c_d t_d) x_d: ONE dot product of the
// row with tw = fl(c o t), the operand shape of the cosine search.  Stage 1 multiplies q' = tw 2^-f, split hi / lo exactly as
// query16_kernel splits it, by the stored rows; the file header's bound holds against the real sum, |dot^ - 2^-f sum tw_d x_d| <=
// eps_a ||q'|| ||x|| (its accumulation term prices dot^ against the real sum and then adds the chain's own roundings), and
//   eps_mse = eps_a (resident fp16 / bf16, hi or hi + lo) + 2^-22
// pays for tw itself: tw_d = c_d t_d (1 + d), |d| <= 2^-24, or an absolute 2^-150 where the product is subnormal -- against ||tw|| >=
// 2^-77 (fp16, scale below 2^90) or 2^-51 (bf16, scale below 2^30) that is below sqrt(D) 2^-73 ||tw|| ||x||.  Hence
//   D dist_real >= A_dn + B_dn - 2 2^f (dot^ + eps_mse ||q'|| nx) =: L,    nx the row's norm slot (>= ||x||, with the fp16 subnormal term)
// with A_dn <= A_q and B_dn <= B_r: the fp32 sums of D non-negative terms (c >= 0) are within (D + 3) 2^-24 of the real ones in any
// order, so A_dn = A^ (1 - D 2^-22) and B_dn = B^ (1 - D 2^-22), and 0 when the sum is below 2^-100 (where subnormal terms could have
// rounded UP by an absolute D 2^-150).
// The contract's own roundings: with c >= 0 every term and every partial sum is non-negative, so each of the chain's roundings moves
// the value by at most 2^-24 relative.  Counted along the longest path to the result: the subtraction, whose error is squared (2), the
// square (1), the product with c (1); the additions into a partial -- partial j takes EVERY element with (d >> 2) & 15 == j, four per
// 64-element step, so m = 4 ceil(D / 64) terms (D / 16 when 64 | D) and at most m rounded additions; four folds; one division:
// n = m + 9 = 4 ceil(D / 64) + 9 (17 at D = 128, 57 at D = 768), dist^ >= dist_real (1 - 2^-24)^n -- and squares or products that
// underflow lose at most (1 + c_d) 2^-149 each, in all below 2^-126 for c_d <= 2^10.  A token can reach the distance threshold
// theta = -tau only if dist^ <= theta, hence only if  L <= D theta (1 + gamma) + 2^-126,  gamma = (4 ceil(D / 64) + 12) 2^-24  (raised):
// (1 - 2^-24)^-n <= 1 + (n + 3) 2^-24 for every n <= 265, i.e. D <= 4096.
// The test is the instruction of prefilter_kernel as it stands, t = dot^ - a R0 + c R1 + g R2 >= 0 with
//     rowp[i] = {B_dn, nx, 1, 0}      qpar[q] = {-a, c, g, 0},  a = 2^-(f+1) (lowered),  c = eps_mse ||q'|| (raised),
//                                                              g = 2^-(f+1) (D theta (1 + gamma) + 2^-126 - A_dn) (raised)
// each by 2^-19 relative for the instruction's own fp32 chain (prefilter_kernel's argument: the slack covers it term by term).  So
// stage 1 runs the TOK instances unchanged; only the constants differ.
// A row is UNBOUNDABLE -- {0, inf, 1, 0}: a candidate of every query, decided by stage 2 -- when it has an inf / NaN element (bf16: a
// nonzero element outside [2^-60, 2^120)), or when B^ is not a finite number below 2^36 (fp16) / 2^96 (bf16) or is negative: with
// the query windows below a R0 then stays finite.  A query is flagged (redo: the grouped search answers it) when tw is zero, its
// scale 2^-f is outside (0, 2^90) (fp16) / (2^-100, 2^30) (bf16), A^ is not finite, g is not finite, or ANY c_d is negative, NaN or
// above 2^10 -- then every query is flagged, since no row constant is a bound.
__host__ __device__ inline double eps_mse_of(int D, bool lo, bool bf) { return (bf ? eps_a_bf16_of(D, lo) : eps_a_of(D, lo, true)) + 0x1p-22; }
__host__ __device__ inline double gamma_mse_of(int D) { return (4 * ((D + 63) / 64) + 12) * 0x1p-24; }
constexpr int MSE_SCALE_HI_F16 = 90, MSE_B_HI_F16 = 36, MSE_B_HI_BF16 = 96;

// the query's row of the test's A operand under MSE (see above); qb = {A_dn, eps_mse ||q'||, 2^-f, flag}; *bad: g left fp32's range
__device__ __forceinline__ float4 mse_test_row(float tau, float4 qb, float fD, float gamma, bool *bad) {
    const float theta = tau > -3.0e38f ? -tau : 3.0e38f;       // the distance threshold; no threshold yet: everything passes
    float T = theta * fD;
    T = fmaf(fabsf(T), gamma, T) + 0x1p-126f;                  // D theta (1 + gamma) + 2^-126 (the slack below covers these roundings)
    if (T > 3.0e38f) T = 3.0e38f;                              // (a floor of +inf: theta = -inf, T = inf - inf stays NaN -> g NaN -> *bad)
    const float h = 0.5f * qb.z;                              // 2^-(f+1), exact
    float g = h * (T - qb.x);
    g += fabsf(g) * 0x1p-19f;
    if (g > 3.0e38f) g = 3.0e38f;                              // no threshold yet (or a loose one times a large scale): a R0 < 2^125, all pass
    *bad = !(g >= -3.0e38f);                                   // -inf or NaN: the test of an unboundable row would not be a number
    return make_float4(-(h - h * 0x1p-19f), qb.y * (1.0f + 0x1p-19f), g, 0.f);
}

// eight consecutive elements of a 16-bit row as fp32 (exact)
template <bool BF>
__device__ __forceinline__ void widen8(const uint4 raw, float (&a)[8]) {
    const unsigned int u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (BF) {
            a[2 * j] = __uint_as_float(u[j] << 16);
            a[2 * j + 1] = __uint_as_float(u[j] & 0xFFFF0000u);
        } else {
            typedef __attribute__((ext_vector_type(2))) _Float16 half2_t;
            const half2_t h = __builtin_bit_cast(half2_t, u[j]);
            a[2 * j] = (float)h[0];
            a[2 * j + 1] = (float)h[1];
        }
    }
}

// Row constants under MSE: one wave per row, 16 bytes per lane and load.  rowp[i] = {B_dn, nx, 1, 0}; nx, the tail tile and the
// padding sentinel are those of bank16_rowp_lp_kernel (fp16: sub_scale = 2^-14 / eps_mse(hi + lo), raised) and bankbf16_rowp_kernel
// (bf16: the norm of the row scaled by a power of two, a second pass over the row in L2).  D % 8 == 0.
template <bool BF>
__global__ __launch_bounds__(256) void mse_rowp_kernel(const unsigned short *__restrict__ bank, const float *__restrict__ cw, int64_t N, int D,
                                                        float4 *__restrict__ rowp, int64_t rows_padded, unsigned short *__restrict__ tail,
                                                        int64_t tail_first, float sub_scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_padded) return;
    unsigned short *t = tail && row >= tail_first ? tail + (row - tail_first) * D : nullptr;
    if (row >= N) {
        if (t)
            for (int d = lane * 8; d < D; d += 512) *(uint4 *)(t + d) = make_uint4(0u, 0u, 0u, 0u);
        if (lane == 0) rowp[row] = make_float4(0.f, NAN, 0.f, 0.f);
        return;
    }
    const unsigned short *x = bank + row * D;
    float B = 0.f, ss = 0.f, nsub = 0.f, bad = 0.f, mx = 0.f;
    for (int d = lane * 8; d < D; d += 512) {
        const uint4 raw = *(const uint4 *)(x + d);
        if (t) *(uint4 *)(t + d) = raw;
        float a[8];
        widen8<BF>(raw, a);
        const float4 c0 = *(const float4 *)(cw + d), c1 = *(const float4 *)(cw + d + 4);
        const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float m = fabsf(a[j]);
            if (BF) bad = (!(m < ldexpf(1.0f, BF_ROW_HI)) || (m > 0.f && m < ldexpf(1.0f, -BF_ROW_LO))) ? 1.f : bad;
            else bad = !(m < INFINITY) ? 1.f : bad;
            const float sq = a[j] * a[j];                      // exact where it neither overflows nor underflows (window / B^ rule)
            B = fmaf(c[j], sq, B);
            if (!BF) {
                ss += sq;
                nsub += (m > 0.f && m < 0x1p-14f) ? 1.f : 0.f;
            }
            mx = fmaxf(mx, m);
        }
    }
    B = wave_sum(B);
    bad = wave_max(bad);
    if (!(B >= 0.f && B < ldexpf(1.0f, BF ? MSE_B_HI_BF16 : MSE_B_HI_F16))) bad = 1.f;
    if (bad != 0.f) {
        if (lane == 0) rowp[row] = make_float4(0.f, INFINITY, 1.0f, 0.f);
        return;
    }
    float nx;
    if (BF) {
        mx = wave_max(mx);
        int e = 0;
        if (mx > 0.f) (void)frexpf(mx, &e);
        const float s = ldexpf(1.0f, -e);
        for (int d = lane * 8; d < D; d += 512) {
            float a[8];
            widen8<true>(*(const uint4 *)(x + d), a);
#pragma unroll
            for (int j = 0; j < 8; ++j) ss = fmaf(a[j] * s, a[j] * s, ss);
        }
        ss = wave_sum(ss);
        nx = ldexpf(sqrtf(ss) * (1.0f + (float)D * 0x1p-22f) * (1.0f + 0x1p-21f), e);
    } else {
        ss = wave_sum(ss);
        nsub = wave_sum(nsub);                                 // <= D <= 4096: exact
        nx = fmaf(sqrtf(nsub), sub_scale, sqrtf(ss) * (1.0f + (float)D * 0x1p-22f)) * (1.0f + 0x1p-21f);
    }
    if (lane == 0) {
        const float Bdn = B < 0x1p-100f ? 0.f : B * (1.0f - (float)D * 0x1p-22f);
        rowp[row] = make_float4(Bdn, nx, 1.0f, 0.f);
    }
}

// Queries under MSE: tw = fl(c o t) -> qh, ql exactly as query16_kernel writes them (same scale rule, same padding rows);
// qbase[q] = {A_dn, eps_mse ||q'|| (1 + D 2^-22), 2^-f, flag}, flag != 0: a weight outside [0, 2^10] or A^ not finite
template <bool BF>
__global__ __launch_bounds__(256) void mse_query_kernel(const float *__restrict__ cw, const float *__restrict__ tq, int Q, int D,
                                                         half_t *__restrict__ qh, half_t *__restrict__ ql, float4 *__restrict__ qbase,
                                                         float eps_mse) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) {
        if (q < (Q + QPAD - 1) / QPAD * QPAD)
            for (int d = lane * 4; d < D; d += 256) {
                *(uint2 *)(qh + (int64_t)q * D + d) = make_uint2(0u, 0u);
                *(uint2 *)(ql + (int64_t)q * D + d) = make_uint2(0u, 0u);
            }
        return;
    }
    const float *x = tq + (int64_t)q * D;
    float mx = 0.f, A = 0.f, cbad = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4 *)(x + d), c = *(const float4 *)(cw + d);
        const float tv[4] = {v.x, v.y, v.z, v.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float w = __fmul_rn(cv[j], tv[j]);
            mx = fmaxf(mx, fabsf(w));
            A += __fmul_rn(w, tv[j]);
            cbad = !(cv[j] >= 0.f && cv[j] <= 0x1p10f) ? 1.f : cbad;
        }
    }
    mx = wave_max(mx);
    A = wave_sum(A);
    cbad = wave_max(cbad);
    int e = 0;
    if (mx > 0.f && mx < INFINITY) {
        (void)frexpf(mx, &e);
        e -= BF ? BF_QMAX_EXP : 14;
    }
    if (e < -126) e = -126;             // (query16_kernel's clamps: such a query is flagged by mse_state_kernel)
    if (BF && e > BF_SCALE_LO) e = BF_SCALE_LO;
    const float s = ldexpf(1.0f, -e);
    float ss = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4 *)(x + d), c = *(const float4 *)(cw + d);
        const float a[4] = {__fmul_rn(c.x, v.x) * s, __fmul_rn(c.y, v.y) * s, __fmul_rn(c.z, v.z) * s, __fmul_rn(c.w, v.w) * s};
        if (BF) {
            bf16x4 h, l;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ss = fmaf(a[j], a[j], ss);
                h[j] = (bf16_t)a[j];
                l[j] = (bf16_t)(a[j] - (float)h[j]);
            }
            *(bf16x4 *)(qh + (int64_t)q * D + d) = h;
            *(bf16x4 *)(ql + (int64_t)q * D + d) = l;
            continue;
        }
        typedef __attribute__((ext_vector_type(4))) _Float16 half4;
        half4 h, l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ss = fmaf(a[j], a[j], ss);
            h[j] = (half_t)a[j];
            l[j] = (half_t)(a[j] - (float)h[j]);
        }
        *(half4 *)(qh + (int64_t)q * D + d) = h;
        *(half4 *)(ql + (int64_t)q * D + d) = l;
    }
    ss = wave_sum(ss);
    if (lane == 0) {
        const float nq = sqrtf(ss) * (1.0f + (float)D * 0x1p-22f);
        const bool flag = cbad != 0.f || !(A >= 0.f && A < INFINITY);
        const float Adn = !(A >= 0x1p-100f) ? 0.f : A * (1.0f - (float)D * 0x1p-22f);
        qbase[q] = make_float4(flag ? 0.f : Adn, eps_mse * nq, s, flag ? 1.f : 0.f);
    }
}

// init_state_kernel and token_state_kernel under MSE: the first threshold (a floor that is not a number counts as none), empty lists,
// the first test row, and the queries stage 1 cannot serve (see above)
__global__ void mse_state_kernel(int Q, int Q_padded, const float *__restrict__ thr0, const float4 *__restrict__ qbase, float fD, float gamma,
                                 float4 *__restrict__ qpar, float *__restrict__ tau_q, int *__restrict__ cnt, int *__restrict__ rn,
                                 int *__restrict__ overflow, float scale_lo, float scale_hi) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) {
        if (q < Q_padded) qpar[q] = make_float4(NAN, NAN, NAN, NAN);   // padding of the last query tile: t = NaN, no pair passes
        return;
    }
    float tau = thr0 ? thr0[q] : -INFINITY;
    if (!(tau == tau)) tau = -INFINITY;
    tau_q[q] = tau;
    cnt[q] = 0;
    rn[q] = 0;
    const float4 qb = qbase[q];
    bool out;
    qpar[q] = mse_test_row(tau, qb, fD, gamma, &out);
    overflow[q] = out || qb.w != 0.f || qb.z >= scale_hi || qb.z <= scale_lo || !(qb.y > 0.f && qb.y < 0x1p60f) ? 1 : 0;
}

// ---- Weighted MSE under combine 'mean' (skyemb_token_mse_mean_pool / _rowp / skyemb_distance_topk_tokens_mean_prefiltered) ---------------
// Contract: the distance chain per token, then the grouped kernels' fold (((0 + d_0) + d_1) + ...) / float(P) in token order; in key
// space (key = -dist) that fold of keys is its negation bit for bit, so stage 2 is token_rescore_body with DIST and the TOK_MEAN fold.
// The mean is LINEAR in the tokens: per image i and query q, in real arithmetic, with P a power of two,
//   D mean_p dist(q, x_p) = A_q + Bbar_i - 2 (c o t_q) . m_i,   m_i = (1/P) sum_p x_p,   Bbar_i = (1/P) sum_p sum_d c_d x_pd^2,
// the operand shape of "Weighted MSE" above with a row that is an IMAGE: stage 1 is the ROW pass (prefilter_kernel without TOK) over a
// pooled 16-bit image [N, D], P times fewer rows than the bank, as under the cosine 'mean'; the query constants, the first state and
// the threshold refresh are mse_query_kernel's, mse_state_kernel's and mse_test_row's, fed the eps and gamma below.
// The pooled image (token_mse_mean_pool_kernel; it depends on the bank only): m_fl = fl(sum_p x_p) / P -- the widened tokens summed in
// fp32 in token order from +0 (the first addition is exact), one exact scale by 1 / P --, then m' = m_fl 2^-e with the largest |m'_d|
// in [2^13, 2^14) (exact; e = 0 for a zero row) rounded ONCE to the bank's dtype (bf16: elements below 2^-40 stored as zero).  That is
// the situation of the cosine mean's pooled image, points (b) + (a) there:  |dot^ - q' . m'| <= eps_m ||q'|| ||m'||,  eps_m = eps_m_of.
//   pooling    per element |fl(sum_p x_pd) - sum_p x_pd| <= 1.01 (P - 1) 2^-24 sum_p |x_pd| (P - 1 <= 63 rounded additions; nothing
//              underflows: fp16 elements are multiples of 2^-24, bf16 elements of the window multiples of 2^-67), so by the triangle
//              inequality over the tokens  ||m_fl - m|| <= kappa c1,  kappa = 1.01 P 2^-24,  c1 = mean_p ||x_p||_2.
//   tw         tw_d = fl(c_d t_d) against c_d t_d: 2^-24 relative (or the absolute 2^-150 of "Weighted MSE"), against
//              ||m|| <= ||m_fl|| + kappa c1: below 2^-22 ||q'|| R1 2^e with R1 as follows.
// Together  |dot^ - 2^-(f + e) (c o t) . m| <= eps ||q'|| R1,   eps = eps_m + 2^-22,   R1 = ||m'|| + (kappa / eps_m) c1 2^-e  (raised; the
// SMALLER eps_m, hi + lo, so one image serves both variants), hence
//   D mean_real >= A_dn + Bbar_dn - 2 2^(f + e) (dot^ + eps ||q'|| R1) =: L.
// Bbar_dn <= Bbar in the manner of B_dn: token_mse_mean_rowp_kernel adds the P D non-negative terms c_d x_pd^2 lane by lane.  A lane
// takes 8 consecutive elements per 512-element step of a row -- only D / 8 lanes have any when D < 512 --, so an active lane's chain is
// n_B = 8 P ceil(D / 512) fused multiply-adds into one accumulator (the squares exact inside the windows; P D / 64 of them only when
// 512 divides D: 8 P at D = 128), and wave_sum folds the 64 lanes in 6 more additions (an idle lane adds an exact 0).  Every term and
// partial sum is non-negative, so the fp32 sum is within 1.01 (n_B + 6) 2^-24 of the real one (n_B + 6 <= 4102):
// Bbar_dn = Bbar^ (1 - (n_B + 8) 2^-23), twice that, and 0 below 2^-100.
// The contract's own roundings: each token distance as above, dist_p^ >= dist_p (1 - 2^-24)^n, n = 4 ceil(D / 64) + 9; the fold adds P
// non-negative terms with P - 1 rounded additions and divides exactly, so mean^ >= mean_real (1 - 2^-24)^(n + P - 1) - (what
// underflows: below 2^-126 in units of D dist, the division's 2^-150 included), and an image can reach the distance threshold theta
// only if  L <= D theta (1 + gamma) + 2^-126,   gamma = gamma_mse_of(D) + P 2^-24 = (4 ceil(D / 64) + 12 + P) 2^-24
// ((1 - 2^-24)^-n' <= 1 + (n' + 3) 2^-24 for every n' <= 328).  Times 2^-(f + 1 + e) this is the test instruction as it stands,
//   t = dot^ - a R0 + c R1 + g R2 >= 0,   rowp[i] = {Bbar_dn 2^-e, R1, 2^-e, 0},   qpar[q] = mse_test_row's {-a, c, g, 0}.
// An image is UNBOUNDABLE -- zeros in the pooled row where the bank alone decides it, and {0, inf, 1, 0}: a candidate of every query,
// decided by stage 2 -- when a token has an inf / NaN element (bf16: a nonzero element outside [2^-60, 2^120)), when R1 or R2 = 2^-e
// reach 2^60 (a pooled row of heavy cancellation, bf16 only: fp16 keeps 2^-e <= 2^43), when Bbar^ is not a number in [0, 2^36) (fp16) /
// [0, 2^96) (bf16), or when R0 leaves that same window: with the query windows of mse_state_kernel a R0 and c R1 then stay finite, and
// g R2 overflows only where its sign already decides the test.  An image whose tokens cancel to an exactly zero pooled row is an
// ordinary image: m' = 0, dot^ = 0, R1 the pooling term alone.  Queries are flagged as under "Weighted MSE".
__host__ __device__ inline double eps_mse_mean_of(int D, bool lo, bool bf) { return eps_m_of(D, lo, bf) + 0x1p-22; }
__host__ __device__ inline double gamma_mse_mean_of(int D, int P) { return gamma_mse_of(D) + P * 0x1p-24; }
inline double kappa_mse_mean_of(int P) { return 1.01 * P * 0x1p-24; }

// One wave per image: the pooled row and the bank's share of its constants, paux[i] = {R1, 2^-e}; an unboundable image {inf, 1} and a
// zero pooled row; padding rows {NaN, 0}.  tail / tail_first: as in token_mean_pool_kernel.  kfac = kappa / eps_m (hi + lo), raised.
template <bool BF>
__global__ __launch_bounds__(128) void token_mse_mean_pool_kernel(const unsigned short *__restrict__ bank, int64_t N, int P, int D,
                                                                   unsigned short *__restrict__ pooled, float2 *__restrict__ paux,
                                                                   int64_t rows_padded, unsigned short *__restrict__ tail,
                                                                   int64_t tail_first, float kfac) {
    __shared__ float sm[2][4096];                             // the image's sums, D <= 4096; a lane only ever touches its own elements
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t img = (int64_t)blockIdx.x * 2 + w;
    if (img >= rows_padded) return;
    unsigned short *t = tail && img >= tail_first ? tail + (img - tail_first) * D : nullptr;
    if (img >= N) {
        if (t)
            for (int d = lane * 8; d < D; d += 512) *(uint4 *)(t + d) = make_uint4(0u, 0u, 0u, 0u);
        if (lane == 0) paux[img] = make_float2(NAN, 0.f);
        return;
    }
    float *m = sm[w];
    for (int d = lane * 8; d < D; d += 512) {
        *(float4 *)(m + d) = make_float4(0.f, 0.f, 0.f, 0.f);
        *(float4 *)(m + d + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float bad = 0.f, c1 = 0.f;
    for (int p = 0; p < P; ++p) {
        const unsigned short *x = bank + (img * P + p) * D;
        float ss = 0.f;
        for (int d = lane * 8; d < D; d += 512) {
            float a[8];
            widen8<BF>(*(const uint4 *)(x + d), a);
            const float4 s0 = *(const float4 *)(m + d), s1 = *(const float4 *)(m + d + 4);
            float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float mag = fabsf(a[j]);
                if (BF) bad = (!(mag < ldexpf(1.0f, BF_ROW_HI)) || (mag > 0.f && mag < ldexpf(1.0f, -BF_ROW_LO))) ? 1.f : bad;
                else bad = !(mag < INFINITY) ? 1.f : bad;
                ss = fmaf(a[j], a[j], ss);                     // (bf16: a square may overflow: c1 = inf, R1 = inf, unboundable)
                s[j] = s[j] + a[j];                            // token order: p ascending
            }
            *(float4 *)(m + d) = make_float4(s[0], s[1], s[2], s[3]);
            *(float4 *)(m + d + 4) = make_float4(s[4], s[5], s[6], s[7]);
        }
        c1 += sqrtf(wave_sum(ss));
    }
    const float inv_p = 1.0f / (float)P;                      // a power of two
    float mx = 0.f;
    for (int d = lane * 8; d < D; d += 512) {
        const float4 u = *(const float4 *)(m + d), v = *(const float4 *)(m + d + 4);
        mx = fmaxf(fmaxf(mx, fmaxf(fmaxf(fabsf(u.x), fabsf(u.y)), fmaxf(fabsf(u.z), fabsf(u.w)))),
                   fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    mx = wave_max(mx) * inv_p;
    bad = wave_max(bad);
    if (!(mx < INFINITY)) bad = 1.f;
    int e = 0;
    if (bad == 0.f && mx > 0.f) {
        (void)frexpf(mx, &e);
        e -= 14;                                               // mx 2^-e in [2^13, 2^14)
    }
    const float s = ldexpf(1.0f, -e);                          // (|e| <= 101 inside the windows: finite)
    // norms rounded up: the fp32 sums of squares and of P terms, the square roots
    const float up = (1.0f + (float)(D + 64) * 0x1p-22f) * (1.0f + 0x1p-20f);
    float ss = 0.f;
    if (bad == 0.f)
        for (int d = lane * 8; d < D; d += 512) {
            const float4 u = *(const float4 *)(m + d), v = *(const float4 *)(m + d + 4);
            const float a[8] = {u.x * inv_p * s, u.y * inv_p * s, u.z * inv_p * s, u.w * inv_p * s,
                                v.x * inv_p * s, v.y * inv_p * s, v.z * inv_p * s, v.w * inv_p * s};
#pragma unroll
            for (int j = 0; j < 8; ++j) ss = fmaf(a[j], a[j], ss);
        }
    ss = wave_sum(ss);
    const float r1 = fmaf(kfac * s, c1 * inv_p * up, sqrtf(ss) * up) * (1.0f + 0x1p-21f);
    if (!(r1 < 0x1p60f) || !(s < 0x1p60f)) bad = 1.f;
    unsigned short *o = pooled + img * D;
    for (int d = lane * 8; d < D; d += 512) {
        const float4 u = *(const float4 *)(m + d), v = *(const float4 *)(m + d + 4);
        const float a[8] = {u.x * inv_p * s, u.y * inv_p * s, u.z * inv_p * s, u.w * inv_p * s,
                            v.x * inv_p * s, v.y * inv_p * s, v.z * inv_p * s, v.w * inv_p * s};
        unsigned int r[4] = {0u, 0u, 0u, 0u};
        if (bad == 0.f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned short h0, h1;
                if (BF) {
                    h0 = __builtin_bit_cast(unsigned short, (bf16_t)(fabsf(a[2 * j]) < 0x1p-40f ? 0.f : a[2 * j]));
                    h1 = __builtin_bit_cast(unsigned short, (bf16_t)(fabsf(a[2 * j + 1]) < 0x1p-40f ? 0.f : a[2 * j + 1]));
                } else {
                    h0 = __builtin_bit_cast(unsigned short, (half_t)a[2 * j]);
                    h1 = __builtin_bit_cast(unsigned short, (half_t)a[2 * j + 1]);
                }
                r[j] = (unsigned int)h0 | ((unsigned int)h1 << 16);
            }
        }
        const uint4 raw = make_uint4(r[0], r[1], r[2], r[3]);
        *(uint4 *)(o + d) = raw;
        if (t) *(uint4 *)(t + d) = raw;
    }
    if (lane == 0) paux[img] = bad != 0.f ? make_float2(INFINITY, 1.0f) : make_float2(r1, s);
}

// Row constants under the weights c: one wave per image, a second pass over the bank (16 bytes per lane and load).
// rowp[i] = {Bbar_dn 2^-e, R1, 2^-e, 0} from paux[i] = {R1, 2^-e}; unboundable {0, inf, 1, 0}; padding rows the sentinel {0, NaN, 0, 0}.
template <bool BF>
__global__ __launch_bounds__(256) void token_mse_mean_rowp_kernel(const unsigned short *__restrict__ bank, const float *__restrict__ cw,
                                                                   const float2 *__restrict__ paux, int64_t N, int P, int D,
                                                                   float4 *__restrict__ rowp, int64_t rows_padded) {
    const int lane = threadIdx.x & 63;
    const int64_t img = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (img >= rows_padded) return;
    if (img >= N) {
        if (lane == 0) rowp[img] = make_float4(0.f, NAN, 0.f, 0.f);
        return;
    }
    const unsigned short *x = bank + img * P * D;
    float B = 0.f;
    for (int p = 0; p < P; ++p, x += D)
        for (int d = lane * 8; d < D; d += 512) {
            float a[8];
            widen8<BF>(*(const uint4 *)(x + d), a);
            const float4 c0 = *(const float4 *)(cw + d), c1 = *(const float4 *)(cw + d + 4);
            const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) B = fmaf(c[j], a[j] * a[j], B);    // the square is exact inside the windows (an inf / NaN: B^ fails its own)
        }
    B = wave_sum(B) * (1.0f / (float)P);                      // Bbar^; the scale is a power of two
    if (lane != 0) return;
    const float2 aux = paux[img];
    const float hi = ldexpf(1.0f, BF ? MSE_B_HI_BF16 : MSE_B_HI_F16);
    const int n_b = 8 * P * ((D + 511) / 512);                 // fmas of an active lane's chain (the derivation above), <= 4096
    const float Bdn = B < 0x1p-100f ? 0.f : B * (1.0f - (float)(n_b + 8) * 0x1p-23f);
    float r0 = Bdn * aux.y;                                    // exact, a power of two ...
    if (r0 < 0x1p-126f) r0 = 0.f;                              // ... unless it underflows, where it could round up: lowered to 0
    const bool ok = B >= 0.f && B < hi && r0 < hi && aux.x < INFINITY;     // (NaN fails every comparison)
    rowp[img] = ok ? make_float4(r0, aux.x, aux.y, 0.f) : make_float4(0.f, INFINITY, 1.0f, 0.f);
}

// ---- Weighted MSE with PER-QUERY weights (skyemb_token_mse_pq_image / skyemb_distance_topk_tokens_prefiltered_pq) ------------------------
// Contract: the same chain with query q's own row of c [Q, D] (skyemb_distance_token_topk_pq).  B_r = sum c_qd x_d^2 now depends on the
// query, so it cannot ride in a row constant; it joins the dot product instead.  With c_q >= 0, in real arithmetic
//   D dist = sum_d c_qd (x_d - t_qd)^2 = A_q - 2 u_q . y_x,   u_q = [c_q o t_q ; -c_q / 2],   y_x = [x ; x o x],   A_q = sum c_qd t_qd^2:
// ONE dot product of length 2 D per token.  Stage 1 therefore runs the TOK instances of prefilter_kernel unchanged over a second
// resident 16-bit image of the bank, rows y^_i = [x_i ; r16(x_i o x_i)] of length 2 D (mse_pq_image_kernel: 4 N P D bytes beside the
// bank's 2 N P D, independent of the weights), against query images built from u_q (mse_pq_query_kernel); the row constant B is 0.
// No power of two is folded into the squares: fp16 rows are admitted up to |x| < 2^8 and bf16 has fp32's range.
// The image.  x is a 16-bit number, so x * x is exact in fp32 (where it neither overflows nor underflows: the window below) and
// r16 is ONE round-to-nearest-even to the operand format, rho its unit roundoff: 2^-11 (fp16, 11 significant bits) / 2^-8 (bf16, 8
// significant bits: numbers of [2^e, 2^(e+1)) are 2^(e-7) apart, half of that is 2^(e-8)).  A square v in [2^e, 2^(e+1)) of the
// format's normal range moves by at most rho 2^e <= rho min(v, r16(v)); the bound is attained (x = 95.5 in bf16: 9120.25 -> 9152),
// and by every element of a row at once when they are equal, so nothing below the unit roundoff will do.  fp16 only: a square below 2^-14 (0 < |x| < 2^-7) lands on
// the subnormal grid and moves by at most 2^-25 absolute instead (to zero below 2^-25).
// The bound.  u' = 2^-f u_q with u_q the fp32 numbers the kernel forms -- first half fl(c o t), second half -c / 2, exact (a
// subnormal c loses at most 2^-150) --, split hi / lo as mse_query_kernel splits tw.  Three steps:
//   (1) the resident bound of the file header on the stored rows y^, length 2 D:  |dot^ - 2^-f sum u_d y^_d| <= eps_a(2 D) ||u'|| ||y^|| + s_i,
//       s_i = ||u'|| sqrt(nsub_i) 2^-14 (fp16: nsub_i counts the subnormal elements 0 < |y^_d| < 2^-14 of BOTH halves; nothing is
//       assumed about whether the matrix core flushes them), no additive term for bf16 under (R) on both halves;
//   (2) the rounding of the squares, Cauchy-Schwarz over the second half:  |2^-f sum_{d >= D} u_d (y^_d - y_d)| <= ||u'|| ||y^ - y||
//       <= ||u'|| (rho ||y^|| + sqrt(nsq_i) 2^-25), nsq_i the number of fp16 squares rounded on the subnormal grid (0 for bf16).  In the
//       form the constant is quoted: ||x o x|| <= (1 + rho) ||y^|| and rho ||x o x|| <= rho (1 + rho) ||y^||, which is no smaller;
//   (3) fl(c o t) against c o t: 2^-22, the argument of eps_mse above (||u|| >= ||tw||, ||y|| >= ||x||);
//   (4) bf16 only, the query split at the SAME unit roundoff: |q'_d - qh_d| <= 2^-8 |q'_d| and, with lo, |r_d - ql_d| <= 2^-8 |r_d| <=
//       2^-16 |q'_d|.  eps_a_bf16_of prices these two at 2^-9 and 2^-18; kappa = 2^-9 (hi only) / 2^-16 - 2^-18 (hi + lo) is the
//       difference, added here so that this bound does not lean on it (attained too: q'_d = 2^-21 (1 + 2^-8) for every d).
// Together  |dot^ - 2^-f u_q . y_x| <= eps_pq ||u'|| ny,
//   eps_pq = eps_a(2 D; resident fp16 | bf16; hi | hi + lo) + rho (1 + rho) + 2^-22 (+ kappa, bf16)
//   ny_i  >= ||y^_i||_2 (1 + 2 D 2^-22) + (sqrt(nsub_i) 2^-14 + sqrt(nsq_i) 2^-25) / eps_pq (hi + lo), rounded up (bf16: no second term).
// Hence  D dist_real >= A_dn - 2 2^f (dot^ + eps_pq ||u'|| ny)  with A_dn as above, and the candidate test is mse_test_row's with
// rowp[i] = {0, ny_i, 1, 0} and qbase[q] = {A_dn, eps_pq ||u'||, 2^-f, flag}: mse_state_kernel and the threshold refresh stand as they
// are, gamma taken at the real D (the contract's chain still has D terms).
// A row is UNBOUNDABLE -- {0, inf, 1, 0} and a ZERO image row, so that dot^ stays a number and the row is a candidate of every query,
// decided by stage 2 -- when it has an inf / NaN element, when a square leaves the operand format's range (fp16: |x| >= 2^8; below
// that r16(x^2) <= 65472 is finite), when a nonzero element has its stored square outside [2^-60, 2^120) (bf16: (R) on the second
// half, which implies it on the first and keeps x * x exact in fp32), or when ny is not finite.
// A query is flagged by a negative, NaN or above-2^10 weight IN ITS OWN ROW (the row constants do not depend on the weights, so the
// others stay served), by c_q o t_q = 0 (as tw = 0 is above), and by mse_state_kernel's windows.
__host__ __device__ inline double eps_pq_of(int D, bool lo, bool bf) {
    const double rho = bf ? 0x1p-8 : 0x1p-11;
    const double eps = (bf ? eps_a_bf16_of(2 * D, lo) : eps_a_of(2 * D, lo, true)) + rho * (1.0 + rho) + 0x1p-22;
    return bf ? eps + (lo ? 0x1p-16 - 0x1p-18 : 0x1p-9) : eps;
}

// eight squares of 16-bit elements, rounded once to the operand format: the stored words, and their values as fp32
template <bool BF>
__device__ __forceinline__ uint4 squares8(const float (&a)[8], float (&v)[8]) {
    unsigned int u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float s0 = a[2 * j] * a[2 * j], s1 = a[2 * j + 1] * a[2 * j + 1];
        unsigned short h0, h1;
        if (BF) {
            h0 = __builtin_bit_cast(unsigned short, (bf16_t)s0);
            h1 = __builtin_bit_cast(unsigned short, (bf16_t)s1);
        } else {
            h0 = __builtin_bit_cast(unsigned short, (half_t)s0);
            h1 = __builtin_bit_cast(unsigned short, (half_t)s1);
        }
        u[j] = (unsigned int)h0 | ((unsigned int)h1 << 16);
    }
    const uint4 raw = make_uint4(u[0], u[1], u[2], u[3]);
    widen8<BF>(raw, v);
    return raw;
}

// The image and its row constants: one wave per row, 16 bytes per lane and load.  image [rows_padded, 2 D]: row i = [x_i ; r16(x_i o x_i)],
// an unboundable row and the padding rows i >= N zeros; rowp[i] = {0, ny_i, 1, 0}, unboundable {0, inf, 1, 0}, padding the sentinel
// {0, NaN, 0, 0}.  sub_scale = 2^-14 / eps_pq (hi + lo), raised.  D % 8 == 0.
template <bool BF>
__global__ __launch_bounds__(256) void mse_pq_image_kernel(const unsigned short *__restrict__ bank, int64_t N, int D,
                                                            unsigned short *__restrict__ image, float4 *__restrict__ rowp, int64_t rows_padded,
                                                            float sub_scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_padded) return;
    unsigned short *o = image + row * 2 * D;
    if (row >= N) {
        for (int d = lane * 8; d < 2 * D; d += 512) *(uint4 *)(o + d) = make_uint4(0u, 0u, 0u, 0u);
        if (lane == 0) rowp[row] = make_float4(0.f, NAN, 0.f, 0.f);
        return;
    }
    const unsigned short *x = bank + row * D;
    float ss = 0.f, nsub = 0.f, nsq = 0.f, bad = 0.f, mx = 0.f;
    for (int d = lane * 8; d < D; d += 512) {
        const uint4 raw = *(const uint4 *)(x + d);
        float a[8], v[8];
        widen8<BF>(raw, a);
        *(uint4 *)(o + d) = raw;
        *(uint4 *)(o + D + d) = squares8<BF>(a, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float m = fabsf(a[j]);
            if (BF) {
                bad = (m != 0.f && !(v[j] >= ldexpf(1.0f, -BF_ROW_LO) && v[j] < ldexpf(1.0f, BF_ROW_HI))) ? 1.f : bad;   // NaN: m != 0
                mx = fmaxf(mx, fmaxf(m, v[j]));
            } else {
                bad = !(m < 0x1p8f) ? 1.f : bad;               // inf, NaN, or a square outside fp16
                ss = fmaf(a[j], a[j], ss);
                ss = fmaf(v[j], v[j], ss);
                nsub += (m > 0.f && m < 0x1p-14f) ? 1.f : 0.f;
                nsub += (v[j] > 0.f && v[j] < 0x1p-14f) ? 1.f : 0.f;
                nsq += (m > 0.f && m < 0x1p-7f) ? 1.f : 0.f;
            }
        }
    }
    bad = wave_max(bad);
    float ny = INFINITY;
    if (bad == 0.f) {
        if (BF) {
            mx = wave_max(mx);
            int e = 0;
            if (mx > 0.f) (void)frexpf(mx, &e);                // mx 2^-e in [0.5, 1); e in (-BF_ROW_LO, BF_ROW_HI]
            const float s = ldexpf(1.0f, -e);
            for (int d = lane * 8; d < D; d += 512) {
                float a[8], v[8];
                widen8<true>(*(const uint4 *)(x + d), a);
                (void)squares8<true>(a, v);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    ss = fmaf(a[j] * s, a[j] * s, ss);
                    ss = fmaf(v[j] * s, v[j] * s, ss);
                }
            }
            ss = wave_sum(ss);
            ny = ldexpf(sqrtf(ss) * (1.0f + (float)(2 * D) * 0x1p-22f) * (1.0f + 0x1p-21f), e);
        } else {
            ss = wave_sum(ss);                                 // 2 D <= 4096 terms below 2^32 each
            nsub = wave_sum(nsub);                             // <= 2 D <= 4096: exact
            nsq = wave_sum(nsq);
            ny = fmaf(sqrtf(nsub) + sqrtf(nsq) * 0x1p-11f, sub_scale, sqrtf(ss) * (1.0f + (float)(2 * D) * 0x1p-22f)) * (1.0f + 0x1p-21f);
        }
    }
    if (!(ny < INFINITY)) {                                    // unboundable: a zero image row, so that dot^ is a number
        for (int d = lane * 8; d < D; d += 512) {              // (every lane overwrites the addresses it wrote itself above)
            *(uint4 *)(o + d) = make_uint4(0u, 0u, 0u, 0u);
            *(uint4 *)(o + D + d) = make_uint4(0u, 0u, 0u, 0u);
        }
        ny = INFINITY;
    }
    if (lane == 0) rowp[row] = make_float4(0.f, ny, 1.0f, 0.f);
}

// Queries under per-query weights: one wave per query.  u_q = [fl(c_q o t_q) ; -c_q / 2] -> qh, ql [Q_padded, 2 D] exactly as
// mse_query_kernel writes tw (same scale rule over all 2 D elements, same padding rows); qbase[q] = {A_dn, eps_pq ||u'|| (1 + 2 D 2^-22),
// 2^-f, flag}, flag != 0: a weight of row q outside [0, 2^10], c_q o t_q = 0 or A^ not finite
template <bool BF>
__global__ __launch_bounds__(256) void mse_pq_query_kernel(const float *__restrict__ cw, const float *__restrict__ tq, int Q, int D,
                                                            half_t *__restrict__ qh, half_t *__restrict__ ql, float4 *__restrict__ qbase,
                                                            float eps_pq) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int D2 = 2 * D;
    if (q >= Q) {
        if (q < (Q + QPAD - 1) / QPAD * QPAD)
            for (int d = lane * 4; d < D2; d += 256) {
                *(uint2 *)(qh + (int64_t)q * D2 + d) = make_uint2(0u, 0u);
                *(uint2 *)(ql + (int64_t)q * D2 + d) = make_uint2(0u, 0u);
            }
        return;
    }
    const float *x = tq + (int64_t)q * D, *cq = cw + (int64_t)q * D;
    float mx = 0.f, mw = 0.f, A = 0.f, cbad = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4 *)(x + d), c = *(const float4 *)(cq + d);
        const float tv[4] = {v.x, v.y, v.z, v.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float w = __fmul_rn(cv[j], tv[j]);
            mw = fmaxf(mw, fabsf(w));
            mx = fmaxf(mx, fabsf(0.5f * cv[j]));
            A += __fmul_rn(w, tv[j]);
            cbad = !(cv[j] >= 0.f && cv[j] <= 0x1p10f) ? 1.f : cbad;
        }
    }
    mw = wave_max(mw);
    mx = fmaxf(wave_max(mx), mw);
    A = wave_sum(A);
    cbad = wave_max(cbad);
    int e = 0;
    if (mx > 0.f && mx < INFINITY) {
        (void)frexpf(mx, &e);
        e -= BF ? BF_QMAX_EXP : 14;
    }
    if (e < -126) e = -126;             // (query16_kernel's clamps: such a query is flagged by mse_state_kernel)
    if (BF && e > BF_SCALE_LO) e = BF_SCALE_LO;
    const float s = ldexpf(1.0f, -e);
    float ss = 0.f;
    for (int d = lane * 4; d < D2; d += 256) {
        const int dd = d < D ? d : d - D;                      // (D % 4 == 0: a lane's four elements lie in one half)
        const float4 v = *(const float4 *)(x + dd), c = *(const float4 *)(cq + dd);
        float a[4];
        if (d < D) {
            a[0] = __fmul_rn(c.x, v.x) * s, a[1] = __fmul_rn(c.y, v.y) * s, a[2] = __fmul_rn(c.z, v.z) * s, a[3] = __fmul_rn(c.w, v.w) * s;
        } else {
            a[0] = (-0.5f * c.x) * s, a[1] = (-0.5f * c.y) * s, a[2] = (-0.5f * c.z) * s, a[3] = (-0.5f * c.w) * s;
        }
        if (BF) {
            bf16x4 h, l;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ss = fmaf(a[j], a[j], ss);
                h[j] = (bf16_t)a[j];
                l[j] = (bf16_t)(a[j] - (float)h[j]);
            }
            *(bf16x4 *)(qh + (int64_t)q * D2 + d) = h;
            *(bf16x4 *)(ql + (int64_t)q * D2 + d) = l;
            continue;
        }
        typedef __attribute__((ext_vector_type(4))) _Float16 half4;
        half4 h, l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ss = fmaf(a[j], a[j], ss);
            h[j] = (half_t)a[j];
            l[j] = (half_t)(a[j] - (float)h[j]);
        }
        *(half4 *)(qh + (int64_t)q * D2 + d) = h;
        *(half4 *)(ql + (int64_t)q * D2 + d) = l;
    }
    ss = wave_sum(ss);
    if (lane == 0) {
        const float nq = sqrtf(ss) * (1.0f + (float)D2 * 0x1p-22f);
        const bool flag = cbad != 0.f || !(mw > 0.f) || !(A >= 0.f && A < INFINITY);
        const float Adn = !(A >= 0x1p-100f) ? 0.f : A * (1.0f - (float)D * 0x1p-22f);
        qbase[q] = make_float4(flag ? 0.f : Adn, eps_pq * nq, s, flag ? 1.f : 0.f);
    }
}

// One wave per image: the pooled row and its constants (the derivation above).  tail / tail_first / the padding sentinel: as in
// bank16_rowp_lp_kernel, with images for rows.  kfac = kappa / eps_m (hi + lo), raised.
template <bool BF>
__global__ __launch_bounds__(128) void token_mean_pool_kernel(const unsigned short *__restrict__ bank, const float *__restrict__ xn, int64_t N,
                                                               int P, int D, unsigned short *__restrict__ pooled, float4 *__restrict__ rowp,
                                                               int64_t rows_padded, unsigned short *__restrict__ tail, int64_t tail_first,
                                                               float kfac) {
    __shared__ float sm[2][4096];                             // the image's sums, D <= 4096; a lane only ever touches its own elements
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t img = (int64_t)blockIdx.x * 2 + w;
    if (img >= rows_padded) return;
    unsigned short *t = tail && img >= tail_first ? tail + (img - tail_first) * D : nullptr;
    if (img >= N) {
        if (t)
            for (int d = lane * 4; d < D; d += 256) *(uint2 *)(t + d) = make_uint2(0u, 0u);
        if (lane == 0) rowp[img] = make_float4(0.f, NAN, 0.f, 0.f);
        return;
    }
    float *m = sm[w];
    for (int d = lane * 4; d < D; d += 256) *(float4 *)(m + d) = make_float4(0.f, 0.f, 0.f, 0.f);
    float bad = 0.f, c1 = 0.f, c2 = 0.f;
    for (int p = 0; p < P; ++p) {
        const int64_t row = img * P + p;
        const float n = xn[row];
        const bool nok = n >= 0x1p-40f && n <= 0x1p40f;        // (false for 0, inf and NaN)
        const float nn = nok ? n : 1.0f;
        const unsigned short *x = bank + row * D;
        float ss = 0.f;
        for (int d = lane * 4; d < D; d += 256) {
            const float4 v = BF ? row4((const bf16_t *)(x + d)) : row4((const half_t *)(x + d));
            const float a[4] = {v.x, v.y, v.z, v.w};
            float4 s4 = *(float4 *)(m + d);
            float *s = (float *)&s4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float mag = fabsf(a[j]);
                if (BF) bad = (!(mag < ldexpf(1.0f, BF_ROW_HI)) || (mag > 0.f && mag < ldexpf(1.0f, -BF_ROW_LO))) ? 1.f : bad;
                else bad = !(mag < INFINITY) ? 1.f : bad;
                const float u = __fdiv_rn(a[j], nn);
                ss = fmaf(u, u, ss);
                s[j] = s[j] + u;                               // token order: p ascending
            }
            *(float4 *)(m + d) = s4;
        }
        ss = wave_sum(ss);
        const float nu = sqrtf(ss);
        if (!nok || !(nu >= 0x1p-20f && nu <= 0x1p20f)) bad = 1.f;
        c1 += nu;
        c2 += __fdiv_rn(nu, nn);
    }
    const float inv_p = 1.0f / (float)P;                      // a power of two
    float mx = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4 *)(m + d);
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    mx = wave_max(mx) * inv_p;
    bad = wave_max(bad);
    if (!(mx < INFINITY) || (mx > 0.f && mx < 0x1p-40f)) bad = 1.f;
    int e = 0;
    if (bad == 0.f && mx > 0.f) {
        (void)frexpf(mx, &e);
        e -= 14;                                               // mx 2^-e in [2^13, 2^14); -54 <= e <= 7
    }
    const float s = ldexpf(1.0f, -e);
    // norms rounded up: the fp32 sums of squares and of P terms, the divisions, the square roots
    const float up = (1.0f + (float)(D + 64) * 0x1p-22f) * (1.0f + 0x1p-20f);
    float ss = 0.f;
    if (bad == 0.f)
        for (int d = lane * 4; d < D; d += 256) {
            const float4 v = *(const float4 *)(m + d);
            const float a[4] = {v.x * inv_p * s, v.y * inv_p * s, v.z * inv_p * s, v.w * inv_p * s};
            for (int j = 0; j < 4; ++j) ss = fmaf(a[j], a[j], ss);
        }
    ss = wave_sum(ss);
    const float r1 = fmaf(kfac * s, c1 * inv_p * up, sqrtf(ss) * up) * (1.0f + 0x1p-21f);
    const float r2 = c2 * inv_p * s * up;
    if (!(r1 < 0x1p60f) || !(r2 < 0x1p60f)) bad = 1.f;
    unsigned short *o = pooled + img * D;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4 *)(m + d);
        const float a[4] = {v.x * inv_p * s, v.y * inv_p * s, v.z * inv_p * s, v.w * inv_p * s};
        uint2 raw;
        if (bad != 0.f) {
            raw = make_uint2(0u, 0u);
        } else if (BF) {
            bf16x4 h;
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = (bf16_t)(fabsf(a[j]) < 0x1p-40f ? 0.f : a[j]);
            raw = __builtin_bit_cast(uint2, h);
        } else {
            typedef __attribute__((ext_vector_type(4))) _Float16 half4;
            half4 h;
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = (half_t)a[j];
            raw = __builtin_bit_cast(uint2, h);
        }
        *(uint2 *)(o + d) = raw;
        if (t) *(uint2 *)(t + d) = raw;
    }
    if (lane == 0) rowp[img] = bad != 0.f ? make_float4(0.f, INFINITY, 1.0f, 0.f) : make_float4(s, r1, r2, 0.f);
}

__device__ __forceinline__ unsigned long long image_key(float score, int image) {
    return ((unsigned long long)orderable(score) << 32) | (unsigned int)~(unsigned int)image;   // larger: better score, then lower image
}

// key of the kth largest (1-based, kth <= n) among the 64-bit keys[0..n) (LDS); 8 radix passes of 8 bits.  All threads return it.
__device__ unsigned long long radix_kth_largest64(const unsigned long long *keys, int n, int kth, int *hist, int tid, int nthreads) {
    unsigned long long prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int b = tid; b < 256; b += nthreads) hist[b] = 0;
        __syncthreads();
        for (int e = tid; e < n; e += nthreads) {
            const unsigned long long kx = keys[e];
            if ((kx & mask) == prefix) atomicAdd(&hist[(int)((kx >> shift) & 255ull)], 1);
        }
        __syncthreads();
        radix_pick_bin(hist, kth, tid);
        __syncthreads();
        const int b = hist[256];
        kth = hist[257];
        prefix |= (unsigned long long)b << shift;
        mask |= 255ull << shift;
        __syncthreads();
    }
    return prefix;
}

// after init_state_kernel: empty running lists, a floor that is not a number counts as none, and the queries stage 1 cannot serve
// gfac >= 0: the search combines by mean -- the test parameters become those of the mean bound (mean_test_row; gfac = eps / eps_m,
// NaN when eps is negative or not finite) and the query windows of that bound apply.  gfac < 0: min / max, as ever.
__global__ void token_state_kernel(int Q, const float4 *__restrict__ qbase, float *__restrict__ tau_q, int *__restrict__ rn,
                                   int *__restrict__ overflow, float gfac, float4 *__restrict__ qpar) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    rn[q] = 0;
    if (!(tau_q[q] == tau_q[q])) tau_q[q] = -INFINITY;        // (init_state_kernel has opened the test for it already)
    const float4 qb = qbase[q];
    const float c = qb.y;                                      // eps_a ||q'||
    if (!(c > 0.f && c < INFINITY)) overflow[q] = 1;
    if (!(gfac < 0.f)) {
        bool bad;
        qpar[q] = mean_test_row(tau_q[q], qb, gfac, &bad);
        if (bad || !(qb.w >= 0x1p-20f && qb.w <= 0x1p20f) || !(qb.z >= 0x1p-34f && qb.z <= 0x1p34f)) overflow[q] = 1;
    }
}

// one workgroup (256 threads) per query: the exact combined scores of the slice's candidate images, the merge into the running
// list, the new threshold; final: the ordered result.  lgp: P = 2^lgp <= 64 tokens, one lane each, 256 / P images per round.
// TOPT ('min' under top_t, the `_top` entries; fold is TOK_MIN): the image scores d[top_t - 1], the top_t-th best of its token scores,
// by the grouped kernels' own network (token_combine.h) in their operand order -- so bit for bit their value, ties by fmaxf / fminf.
// There an image of 32 / 64 tokens meets the network as two / four 16-token tiles, one after the other, with the 16 best so far
// carried; here the tiles sit side by side on 32 / 64 lanes: each is sorted in its own 16 lanes, then tiles 1, 2, 3 are merged, in
// that order, into the lanes of tile 0 (top_tile's step with the carry in tile 0's lanes and the new tile fetched across).
// Without TOPT top_t is not read: the instruction stream of the kernels without it.
// MAP ('mean' under a selection, the `_mean_prefiltered_sel` entry; fold is TOK_MEAN): stage 1 ran over the COMPACTED pooled image of
// skyemb_token_mean_select_gather, so a candidate is a position c in [0, S) of it and the image is map[c]; its token rows are read from
// the full bank and the keys carry the image, so the lists, the threshold and the result are those of the unmapped search (map is
// ascending: (score desc, image asc) is (score desc, position asc)).  Without MAP neither map nor S is read.
// DIST (the weighted-MSE search, "Weighted MSE" below; fold is TOK_MIN or TOK_MAX in KEY space): tw holds the raw queries t, cw the
// weights c [D], and a token's score is key = -dist by the distance contract's chain (distance_chain.h; a NaN distance is key -inf);
// qn, xn and eps are not read, gfac is the widening of the threshold and the next test row is mse_test_row's.  Without DIST cw is
// not read: the instruction stream of the cosine kernels.
// DIST with fold TOK_MEAN (the weighted-MSE search under combine 'mean'): the mean fold below over the keys -dist_p -- the negation of
// the contract's mean of distances bit for bit --, and the DIST refresh, which is tested before the fold's.
// DIST with TOPT (distance 'max' under top_t, the `_top` entries of the MSE search; fold is TOK_MIN): with a[0] <= a[1] <= ... an image's
// token distances, a[top_t - 1] is the top_t-th LARGEST key, so the keys go through the same network and top_finish<MIN>: bit for bit
// distance_token_kernel's value, which sorts the same keys by the same functions.  A NaN distance is key -inf and sorts last; fewer
// than top_t finite distances: key -inf, never returned.
template <typename X, bool TOPT = false, bool MAP = false, bool DIST = false>
__device__ __forceinline__ void token_rescore_body(const float *__restrict__ tw, const float *__restrict__ qn, const X *__restrict__ bank,
                                                   const float *__restrict__ xn, int64_t N, int D, int lgp, int fold, float gfac, int k,
                                                   float eps, int64_t idx_offset, int cap, const float4 *__restrict__ qbase, int *__restrict__ cnt,
                                                   const int *__restrict__ cand_i, unsigned long long *__restrict__ list,
                                                   int *__restrict__ rn, float4 *__restrict__ qpar, float *__restrict__ tau_q,
                                                   int *__restrict__ overflow, int final, float *__restrict__ out_s,
                                                   int64_t *__restrict__ out_i, int *__restrict__ redo, int top_t = 0,
                                                   const int *__restrict__ map = nullptr, int S = 0,
                                                   const float *__restrict__ cw = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long *keys = (unsigned long long *)smem;     // [TOK_KMAX + cap] the running list, then the slice's candidates
    unsigned long long *kept = keys + TOK_KMAX + cap;          // [TOK_KMAX] the new running list
    float *sq = (float *)(kept + TOK_KMAX);                    // [D] weighted query (DIST: the raw query t)
    int *hist = (int *)(sq + D);                               // [260] + two counters
    float *sc = (float *)(hist + 264);                         // DIST: [D] the weights c (16-byte aligned: 264 ints)
    const int tid = threadIdx.x, q = blockIdx.x;
    const int raw = cnt[q];
    const int n = raw < cap ? raw : cap;
    const int r0 = rn[q];                                      // <= k <= TOK_KMAX
    bool bad = raw > cap;                                      // more candidates than the list holds: the grouped search decides
    for (int d = tid; d < D; d += 256) sq[d] = tw[(int64_t)q * D + d];
    if constexpr (DIST)
        for (int d = tid; d < D; d += 256) sc[d] = cw[d];
    unsigned long long *mine = list + (int64_t)q * TOK_KMAX;
    for (int e = tid; e < r0; e += 256) keys[e] = mine[e];
    if (tid == 0) { hist[260] = 0; hist[261] = 0; }
    __syncthreads();
    const int P = 1 << lgp, G = 256 >> lgp;
    const int g = tid >> lgp, p = tid & (P - 1);
    float qnv = 0.f;
    if constexpr (!DIST) qnv = qn[q];
    for (int base = 0; base < n; base += G) {                // (uniform trip count: every lane takes part in the shuffles)
        const int c = base + g;
        int img = c < n ? cand_i[(int64_t)q * cap + c] : 0;
        if constexpr (MAP) {
            if (img < 0 || img >= S) { img = 0; bad = true; }  // never read outside the map (stage 1 appends positions of real rows only)
            img = map[img];
        }
        if (img < 0 || img >= N) { img = 0; bad = true; }      // never read outside the bank (stage 1 appends images of real rows only)
        const int64_t row = (int64_t)img * P + p;
        const X *x = bank + row * D;
        float s;
        if constexpr (DIST) {
            const float dist = dist_row_serial<SKYEMB_METRIC_MSE>([&](int d) { return row4(x + d); }, sq, sc, D);
            s = dist == dist ? -dist : -INFINITY;              // key space; a NaN distance ranks as distance +inf
        } else {
            float acc = 0.f;
            for (int d = 0; d < D; d += 4) {                   // explicit fmaf only: the contract's chain, d ascending
                const float4 v = row4(x + d);
                acc = fmaf(sq[d], v.x, acc);
                acc = fmaf(sq[d + 1], v.y, acc);
                acc = fmaf(sq[d + 2], v.z, acc);
                acc = fmaf(sq[d + 3], v.w, acc);
            }
            s = finish_score(acc, qnv, xn[row], eps);          // a NaN score is -inf: out under min and mean, ignored under max
        }
        if constexpr (TOPT) {
            const int ln = tid & 63, tp = P < 16 ? P : 16, n16 = ln & 15;
            float v = sort_desc(s, ln & (tp - 1), tp);         // every tile of 16 (or image of P < 16) tokens, descending over its lanes
            if (P > 16) {                                      // wave-uniform
                const float mir = lane_xor(v, 15);             // the tile's sorted scores, mirrored: top_tile's second operand
                const int first = ln & ~(P - 1);
                for (int j = 1; j < (P >> 4); ++j) {
                    const float u = __shfl(mir, first + 16 * j + n16, 64);
                    v = merge_desc16(fmaxf(v, u), n16);        // (what lanes past the image's first 16 hold from here on is not read)
                }
            }
            s = top_finish<SKYEMB_COMBINE_MIN>(v, ln, P, top_t);   // lane first + top_t - 1: d[top_t - 1]; -inf with fewer than top_t scores
        } else if (fold == TOK_MEAN) {
            // the grouped kernels' fold (combine_tile<SKYEMB_COMBINE_MEAN>, token_combine.h): (((0 + s_0) + s_1) + ...) in token
            // order, one division by float(P), a sum that is not a number scores -inf
            const int first = (tid & 63) & ~(P - 1);
            float sum = 0.f;
            for (int j = 0; j < P; ++j) sum = sum + __shfl(s, first + j, 64);
            s = __fdiv_rn(sum, (float)P);
            s = s == s ? s : -INFINITY;
        } else {
            for (int o = 1; o < P; o <<= 1) {
                const float u = __shfl_xor(s, o, 64);
                s = fold == TOK_MAX ? fmaxf(s, u) : fminf(s, u);
            }
        }
        // an image that scores -inf is never returned: key 0, below every key that counts
        if (p == 0 && c < n) keys[r0 + c] = s > -INFINITY ? image_key(s, img) : 0ull;
    }
    if (__syncthreads_or(bad) && tid == 0) overflow[q] = 1;
    const int m = r0 + n;
    int live = 0;
    for (int e = tid; e < m; e += 256) live += keys[e] != 0ull ? 1 : 0;
    if (live) atomicAdd(&hist[260], live);
    __syncthreads();
    live = hist[260];
    const int kk = live < k ? live : k;                        // the new running list's length
    unsigned long long kth = ~0ull;
    if (kk > 0) kth = radix_kth_largest64(keys, m, kk, hist, tid, 256);   // (keys are distinct: exactly kk of them are >= kth)
    for (int e = tid; e < m; e += 256)
        if (kk > 0 && keys[e] >= kth) {
            const int slot = atomicAdd(&hist[261], 1);
            if (slot < TOK_KMAX) kept[slot] = keys[e];         // (always: distinct keys)
        }
    __syncthreads();
    for (int e = tid; e < kk; e += 256) mine[e] = kept[e];
    if (tid == 0) {
        rn[q] = kk;
        cnt[q] = 0;
        float tau = tau_q[q];
        if (kk == k) tau = fmaxf(tau, unorderable((unsigned int)(kth >> 32)));   // k images decided: their k-th best exact score
        tau_q[q] = tau;
        const float4 qb = qbase[q];
        if constexpr (DIST) {
            bool out;
            qpar[q] = mse_test_row(tau, qb, (float)D, gfac, &out);
            if (out) overflow[q] = 1;                          // a test parameter left fp32's range: the grouped search decides
        } else if (fold == TOK_MEAN) {
            bool out;
            qpar[q] = mean_test_row(tau, qb, gfac, &out);
            if (out) overflow[q] = 1;                          // tau qn' left fp32's range: the grouped search decides
        } else {
            const float t = tau > -3.0e38f ? tau : -3.0e38f;   // (select_kernel's parameters of the next phase)
            float a = t * qb.x, b = t * eps * qb.z;
            a -= fabsf(a) * 0x1p-19f;
            b -= fabsf(b) * 0x1p-19f;
            if (!(a > -3.0e38f)) a = -3.0e38f;
            qpar[q] = test_row(a, b, qb.y);
        }
    }
    if (!final) return;
    for (int e = tid; e < k; e += 256) {
        if (e < kk) {
            const unsigned long long me = kept[e];
            int rank = 0;
            for (int j = 0; j < kk; ++j) rank += kept[j] > me ? 1 : 0;
            out_s[(int64_t)q * k + rank] = unorderable((unsigned int)(me >> 32));
            out_i[(int64_t)q * k + rank] = idx_offset + (int64_t)(~(unsigned int)me);
        } else {
            out_s[(int64_t)q * k + e] = -INFINITY;
            out_i[(int64_t)q * k + e] = -1;
        }
    }
    if (tid == 0) redo[q] = overflow[q] ? 1 : 0;               // (this thread's own store above included)
}

#define TOKEN_RESCORE_PARAMS(X)                                                                                                  \
    const float *__restrict__ tw, const float *__restrict__ qn, const X *__restrict__ bank, const float *__restrict__ xn, int64_t N, \
        int D, int lgp, int fold, float gfac, int k, float eps, int64_t idx_offset, int cap, const float4 *__restrict__ qbase,       \
        int *__restrict__ cnt, const int *__restrict__ cand_i, unsigned long long *__restrict__ list, int *__restrict__ rn,          \
        float4 *__restrict__ qpar, float *__restrict__ tau_q, int *__restrict__ overflow, int final, float *__restrict__ out_s,     \
        int64_t *__restrict__ out_i, int *__restrict__ redo
#define TOKEN_RESCORE_PASS tw, qn, bank, xn, N, D, lgp, fold, gfac, k, eps, idx_offset, cap, qbase, cnt, cand_i, list, rn, qpar, tau_q, overflow, \
                           final, out_s, out_i, redo
__global__ __launch_bounds__(256) void token_rescore_lp_kernel(TOKEN_RESCORE_PARAMS(half_t)) { token_rescore_body<half_t>(TOKEN_RESCORE_PASS); }
__global__ __launch_bounds__(256) void token_rescore_bf_kernel(TOKEN_RESCORE_PARAMS(bf16_t)) { token_rescore_body<bf16_t>(TOKEN_RESCORE_PASS); }
__global__ __launch_bounds__(256) void token_rescore_top_lp_kernel(TOKEN_RESCORE_PARAMS(half_t), int top_t) {
    token_rescore_body<half_t, true>(TOKEN_RESCORE_PASS, top_t);
}
__global__ __launch_bounds__(256) void token_rescore_top_bf_kernel(TOKEN_RESCORE_PARAMS(bf16_t), int top_t) {
    token_rescore_body<bf16_t, true>(TOKEN_RESCORE_PASS, top_t);
}
__global__ __launch_bounds__(256) void token_rescore_map_lp_kernel(TOKEN_RESCORE_PARAMS(half_t), const int *__restrict__ map, int S) {
    token_rescore_body<half_t, false, true>(TOKEN_RESCORE_PASS, 0, map, S);
}
__global__ __launch_bounds__(256) void token_rescore_map_bf_kernel(TOKEN_RESCORE_PARAMS(bf16_t), const int *__restrict__ map, int S) {
    token_rescore_body<bf16_t, false, true>(TOKEN_RESCORE_PASS, 0, map, S);
}
__global__ __launch_bounds__(256) void token_rescore_mse_lp_kernel(TOKEN_RESCORE_PARAMS(half_t), const float *__restrict__ cw) {
    token_rescore_body<half_t, false, false, true>(TOKEN_RESCORE_PASS, 0, nullptr, 0, cw);
}
__global__ __launch_bounds__(256) void token_rescore_mse_bf_kernel(TOKEN_RESCORE_PARAMS(bf16_t), const float *__restrict__ cw) {
    token_rescore_body<bf16_t, false, false, true>(TOKEN_RESCORE_PASS, 0, nullptr, 0, cw);
}
__global__ __launch_bounds__(256) void token_rescore_mse_top_lp_kernel(TOKEN_RESCORE_PARAMS(half_t), int top_t, const float *__restrict__ cw) {
    token_rescore_body<half_t, true, false, true>(TOKEN_RESCORE_PASS, top_t, nullptr, 0, cw);
}
__global__ __launch_bounds__(256) void token_rescore_mse_top_bf_kernel(TOKEN_RESCORE_PARAMS(bf16_t), int top_t, const float *__restrict__ cw) {
    token_rescore_body<bf16_t, true, false, true>(TOKEN_RESCORE_PASS, top_t, nullptr, 0, cw);
}
// per-query weights ("Weighted MSE with PER-QUERY weights" above): cw is c [Q, D] and the workgroup of query q reads its row
__global__ __launch_bounds__(256) void token_rescore_mse_pq_lp_kernel(TOKEN_RESCORE_PARAMS(half_t), const float *__restrict__ cw) {
    token_rescore_body<half_t, false, false, true>(TOKEN_RESCORE_PASS, 0, nullptr, 0, cw + (int64_t)blockIdx.x * D);
}
__global__ __launch_bounds__(256) void token_rescore_mse_pq_bf_kernel(TOKEN_RESCORE_PARAMS(bf16_t), const float *__restrict__ cw) {
    token_rescore_body<bf16_t, false, false, true>(TOKEN_RESCORE_PASS, 0, nullptr, 0, cw + (int64_t)blockIdx.x * D);
}
// MSE under combine 'mean' ("Weighted MSE under combine 'mean'" above): DIST with the TOK_MEAN fold -- the keys -dist_p summed in token
// order from 0, one division by float(P), a sum that is not a number is key -inf; the threshold refresh is the DIST branch's.  The fold is
// these kernels' own (the `fold` argument is not read), so the min / max branches are not compiled into them.
__global__ __launch_bounds__(256) void token_rescore_mse_mean_lp_kernel(TOKEN_RESCORE_PARAMS(half_t), const float *__restrict__ cw) {
    token_rescore_body<half_t, false, false, true>(tw, qn, bank, xn, N, D, lgp, TOK_MEAN, gfac, k, eps, idx_offset, cap, qbase, cnt, cand_i, list, rn,
                                                   qpar, tau_q, overflow, final, out_s, out_i, redo, 0, nullptr, 0, cw);
}
__global__ __launch_bounds__(256) void token_rescore_mse_mean_bf_kernel(TOKEN_RESCORE_PARAMS(bf16_t), const float *__restrict__ cw) {
    token_rescore_body<bf16_t, false, false, true>(tw, qn, bank, xn, N, D, lgp, TOK_MEAN, gfac, k, eps, idx_offset, cap, qbase, cnt, cand_i, list, rn,
                                                   qpar, tau_q, overflow, final, out_s, out_i, redo, 0, nullptr, 0, cw);
}
#undef TOKEN_RESCORE_PARAMS
#undef TOKEN_RESCORE_PASS

// ---- 'mean' under a selection of images: the compacted pooled image (skyemb_token_mean_select_gather) ------------------------------
// Stage 1 under 'mean' never reads the bank, only the pooled image [N, D] and its constants, so a selection is served by COMPACTING
// them: row j of pooled_sel / rowp_sel is row idx[j] of pooled / rowp bit for bit (the {0, inf, 1, 0} of an unboundable image
// included: it stays a candidate of every query), and stage 1 is the unselected pass over S rows.  A deselected image appears
// nowhere.  One wave per compacted row, 16 bytes per lane and step (D % 32 == 0: whole vectors); rows S .. rows_padded-1: the padding
// sentinel, zeros in the tail tile (bank16_rowp_lp_kernel's layout: tail_first = S rounded down to whole tiles).  An idx outside
// [0, N) is never followed: its row is padding.
__global__ __launch_bounds__(256) void token_mean_select_gather_kernel(const unsigned short *__restrict__ pooled, const float4 *__restrict__ rowp,
                                                                        const int64_t *__restrict__ idx, int64_t N, int64_t S, int D,
                                                                        unsigned short *__restrict__ pooled_sel, float4 *__restrict__ rowp_sel,
                                                                        int64_t rows_padded, unsigned short *__restrict__ tail,
                                                                        int64_t tail_first, int *__restrict__ map) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= rows_padded) return;
    unsigned short *t = tail && j >= tail_first ? tail + (j - tail_first) * D : nullptr;
    const int64_t src = j < S ? idx[j] : -1;
    const bool on = src >= 0 && src < N;
    for (int d = lane * 8; d < D; d += 512) {
        const uint4 v = on ? *(const uint4 *)(pooled + src * D + d) : make_uint4(0u, 0u, 0u, 0u);
        if (j < S) *(uint4 *)(pooled_sel + j * D + d) = v;
        if (t) *(uint4 *)(t + d) = v;
    }
    if (lane == 0) {
        rowp_sel[j] = on ? rowp[src] : make_float4(0.f, NAN, 0.f, 0.f);
        if (j < S) map[j] = on ? (int)src : 0;
    }
}

// ---- a selection of the bank's IMAGES (skyemb_token_prefilter_select_prepare) -------------------------------------------------------
// words: bit i & 31 of word i >> 5 is IMAGE i, padding bits zero (skyemb_pack_select); the row constants and the tiles are per
// token row.  The masked copy: row i keeps its constants iff image i >> lgp is selected; every other row -- the {0, inf, 1, 0} of
// an unboundable row included: under 'max' it would make its deselected image a candidate of every query -- and every row past
// R = N P gets the padding sentinel (select_rowp_kernel's rule, image by image).
__global__ __launch_bounds__(256) void token_select_rowp_kernel(const unsigned int *__restrict__ words, const float4 *__restrict__ rowp,
                                                                 int64_t R, int lgp, int64_t rows_padded, float4 *__restrict__ rowp_sel) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows_padded) return;
    const int64_t img = i >> lgp;
    const bool on = i < R && ((words[img >> 5] >> (img & 31)) & 1u) != 0u;
    rowp_sel[i] = on ? rowp[i] : make_float4(0.f, NAN, 0.f, 0.f);
}
// the live tiles, ascending (select_tiles_kernel's list), and for each the number of selected images up to and including it.  A
// tile holds BT >> lgp images: whole words down to 32 images (P <= 8), else an aligned field of 16, 8 or 4 bits of one word.
// info = {the number of live tiles, 1 if the last bank tile is one of them}.  One workgroup, 1024 tiles per round.
__global__ __launch_bounds__(1024) void token_select_tiles_kernel(const unsigned int *__restrict__ words, int64_t nwords, int lgp,
                                                                   int tiles_all, int *__restrict__ tiles, int *__restrict__ cum,
                                                                   int *__restrict__ info) {
    __shared__ int wlive[16], wcnt[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ipt = BT >> lgp;                                 // images per tile
    int base = 0, cbase = 0;
    for (int r0 = 0; r0 < tiles_all; r0 += 1024) {
        const int t = r0 + tid;
        int pc = 0;
        if (t < tiles_all) {
            const int64_t first = (int64_t)t * ipt;            // a multiple of ipt: the field never leaves its word
            if (ipt >= 32) {
                for (int j = 0; j < ipt / 32; ++j) {
                    const int64_t wi = (first >> 5) + j;
                    if (wi < nwords) pc += __popc(words[wi]);
                }
            } else if ((first >> 5) < nwords) {
                pc = __popc((words[first >> 5] >> (int)(first & 31)) & ((1u << ipt) - 1u));
            }
        }
        const bool live = pc > 0;
        int inc = pc;                                          // inclusive scan of the counts over the wave
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        const unsigned long long m = __ballot(live);
        if (lane == 0) wlive[wave] = __builtin_popcountll(m);
        if (lane == 63) wcnt[wave] = inc;
        __syncthreads();
        int off = base, tot = 0, coff = cbase, ctot = 0;
        for (int w = 0; w < 16; ++w) {
            off += w < wave ? wlive[w] : 0;
            tot += wlive[w];
            coff += w < wave ? wcnt[w] : 0;
            ctot += wcnt[w];
        }
        off += __builtin_popcountll(m & ((1ull << lane) - 1));
        if (live) {                                            // off < the number of live tiles <= tiles_all
            tiles[off] = t;
            cum[off] = coff + inc;
        }
        if (t == tiles_all - 1) info[1] = live ? 1 : 0;
        base += tot;
        cbase += ctot;
        __syncthreads();
    }
    if (tid == 0) info[0] = base;
}

inline int log2_of(int P) {
    int l = 0;
    while ((1 << l) < P) ++l;
    return l;
}

}  // namespace

#define TOKEN_PREFILTER_MSG "many-query patch-token search: needs P a divisor of 64, D %% 32 == 0, 128 <= D <= 4096, 1 <= k <= %d, " \
                            "k <= N, 2048 <= N * P < 2^31 rows and Q >= 1 (Q=%d N=%lld P=%d D=%d k=%d)"
extern "C" int skyemb_token_prefilter_applicable(int Q, int64_t N, int P, int D, int k) {
    const bool ok = pfplan::tokens_shape_ok(Q, N, P, D, k);
    if (!ok) skyemb_set_error(TOKEN_PREFILTER_MSG, TOK_KMAX, Q, (long long)N, P, D, k);
    return ok ? 1 : 0;
}

// ---- 'min' / 'max' under top_t: the shape rule above plus 1 <= top_t <= min(P, 16); 'mean' under top_t is not served (the mean of the
// top_t best is not bounded by a count of pass bits)
#define TOKEN_TOPT_MEAN_MSG "many-query patch-token search: top_t under combine mean is not served by the two-stage route (the mean of " \
                            "the top_t best token scores is not bounded by a count of passing rows); the grouped search serves it"
#define TOKEN_TOPT_RANGE_MSG "many-query patch-token search: top_t must be 1 .. min(P, 16) (top_t=%d P=%d)"
extern "C" int skyemb_token_topt_prefilter_applicable(int Q, int64_t N, int P, int D, int k, int combine, int top_t) {
    if (combine != SKYEMB_COMBINE_MIN && combine != SKYEMB_COMBINE_MAX) {
        if (combine == SKYEMB_COMBINE_MEAN) skyemb_set_error(TOKEN_TOPT_MEAN_MSG);
        else skyemb_set_error("many-query patch-token search: unknown combine code %d", combine);
        return 0;
    }
    if (!skyemb_token_prefilter_applicable(Q, N, P, D, k)) return 0;     // (its own text)
    if (top_t < 1 || top_t > (P < 16 ? P : 16)) {
        skyemb_set_error(TOKEN_TOPT_RANGE_MSG, top_t, P);
        return 0;
    }
    return 1;
}

extern "C" int64_t skyemb_token_prefilter_ws_bytes(int Q, int D, int k) {
    return carve(nullptr, Q, D, pfplan::cap_of(k), nullptr) + align256((int64_t)Q * TOK_KMAX * 8);
}

// ---- combine 'mean': the limits of the token route with rows = images (stage 1 walks the pooled image's N rows)
#define TOKEN_MEAN_PREFILTER_MSG "many-query patch-token search, combine mean: needs P a divisor of 64, D %% 32 == 0, 128 <= D <= 4096, " \
                                 "1 <= k <= %d, k <= N, N >= 2048 images, N * P < 2^31 rows and Q >= 1 (Q=%d N=%lld P=%d D=%d k=%d)"
extern "C" int skyemb_token_mean_prefilter_applicable(int Q, int64_t N, int P, int D, int k) {
    const bool ok = pfplan::mean_shape_ok(Q, N, P, D, k);
    if (!ok) skyemb_set_error(TOKEN_MEAN_PREFILTER_MSG, TOK_KMAX, Q, (long long)N, P, D, k);
    return ok ? 1 : 0;
}

extern "C" int64_t skyemb_token_mean_prefilter_ws_bytes(int Q, int D, int k) { return skyemb_token_prefilter_ws_bytes(Q, D, k); }

extern "C" double skyemb_token_mean_prefilter_eps_m(int D, int lo, int dtype) { return eps_m_of(D, lo != 0, dtype == SKYEMB_BF16); }

extern "C" int skyemb_token_mean_pool(const void *bank16, int dtype, const float *xn, int64_t N, int P, int D, void *pooled16, float *rowp,
                                      void *tail, void *stream) {
    const char *who = "skyemb_token_mean_pool";
    SKY_CHECK_ARG(sky_is_lp(dtype), "%s: dtype " RESIDENT_DTYPE_MSG, who, dtype);
    SKY_CHECK_ARG(bank16 && xn && pooled16 && rowp, "%s: null argument", who);
    SKY_CHECK_ARG(N > 0 && P >= 1 && P <= 64 && 64 % P == 0 && D % BK == 0 && D >= BK && D <= 4096 && N * P < (1ll << 31),
                  "%s: expected P a divisor of 64, D %% 32 == 0, D <= 4096 and fewer than 2^31 token rows (N=%lld P=%d D=%d)", who,
                  (long long)N, P, D);
    SKY_CHECK_ARG(N % BT == 0 || tail, "%s: N = %lld is no whole number of %d-image tiles: a tail tile [%d, D] is needed", who, (long long)N,
                  BT, BT);
    SKY_CHECK_ARG(aligned16(bank16) && aligned16(pooled16) && aligned16(tail), "%s: the bank, the pooled image and the tail tile must be "
                  "16-byte aligned", who);
    const int64_t padded = skyemb_bank16_rowp_rows(N);
    const bool bf = dtype == SKYEMB_BF16;
    const float kfac = (float)(kappa_of(D, P) / eps_m_of(D, true, bf) * (1.0 + 1e-6));
    const dim3 grid((unsigned)(padded / 2));
#define POOL_ARGS (const unsigned short *)bank16, xn, N, P, D, (unsigned short *)pooled16, (float4 *)rowp, padded, \
                  N % BT ? (unsigned short *)tail : nullptr, N / BT * BT, kfac
    if (bf) hipLaunchKernelGGL(token_mean_pool_kernel<true>, grid, dim3(128), 0, (hipStream_t)stream, POOL_ARGS);
    else hipLaunchKernelGGL(token_mean_pool_kernel<false>, grid, dim3(128), 0, (hipStream_t)stream, POOL_ARGS);
#undef POOL_ARGS
    SKY_LAUNCH_CHECK(who);
    return 0;
}

// ---- the same search under a selection of the bank's images ---------------------------------------------------------------------------
extern "C" int skyemb_token_prefilter_select_prepare(const uint32_t *words, int64_t N, int P, const float *rowp, float *rowp_sel,
                                                     int *tiles, int *cum, int *info, void *stream) {
    const char *who = "skyemb_token_prefilter_select_prepare";
    SKY_CHECK_ARG(words && rowp && rowp_sel && tiles && cum && info, "%s: null argument", who);
    SKY_CHECK_ARG(N > 0 && P >= 1 && P <= 64 && 64 % P == 0 && N * P < (1ll << 31),
                  "%s: N = %lld, P = %d: expected P a divisor of 64 and 1 .. 2^31 - 1 token rows", who, (long long)N, P);
    const int64_t R = N * P, padded = skyemb_bank16_rowp_rows(R);
    const int lgp = log2_of(P);
    hipLaunchKernelGGL(token_select_rowp_kernel, dim3((unsigned)(padded / 256)), dim3(256), 0, (hipStream_t)stream, words,
                       (const float4 *)rowp, R, lgp, padded, (float4 *)rowp_sel);
    hipLaunchKernelGGL(token_select_tiles_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, words, ceil_div64(N, 32), lgp,
                       (int)(padded / BT), tiles, cum, info);
    SKY_LAUNCH_CHECK(who);
    return 0;
}

// ---- The host layer of every search entry point: one plan (prefilter_plan.h), one driver ------------------------------------------------
// An entry point states its call as a request and its pointers; sky_prefilter_plan decides everything (variant, slices, instances, LDS
// bytes, constants); `search` checks the pointers, carves the workspace and launches what the plan says.
//   rows     bank: the fp32 rows stage 2 re-scores, bank16 their fp16 image (skyemb_bank16_prepare) -- or bank NULL: bank16 is a resident
//            16-bit bank that both stages read, its last N % BT rows through `tail`.  Stage 2: select_kernel after every slice, one exact
//            re-score at the end.
//   tokens   bank16 the resident token bank [N, P, D]; stage 1 the TOK (top_t > 1: CNT) instances over its flat rows, stage 2 a token
//            re-score after every slice -- d[top_t - 1] by the TOPT kernels under 'min' with 1 <= top_t < P.
//   mean     stage 1 is the ROW search over the pooled image of skyemb_token_mean_pool (`pooled`, with ITS tail and rowp: a row is an image,
//            no TOK fold) under the mean bound's constants; stage 2 re-scores the candidate images' tokens from bank16 as ever.
//            Under a selection (`map`): the same request over the S rows of the COMPACTED pooled image; stage 2 follows map to the bank.
// tiles (a search under a selection, the two select_prepare calls): rowp is the masked copy, the slices walk the live-tile list (SEL).
namespace {

static_assert(pfplan::BT == BT && pfplan::BK == BK && pfplan::QPAD == QPAD && pfplan::NSTAGE == NSTAGE && pfplan::SCAP == SCAP &&
                  pfplan::RESCORE_MAX == RESCORE_MAX && pfplan::TOK_KMAX == TOK_KMAX && pfplan::STAGE_BYTES == stage_bytes(false) &&
                  pfplan::STAGE_BYTES == stage_bytes(true) && pfplan::qtile(false) == qtile(false) && pfplan::qtile(true) == qtile(true) &&
                  TOK_MIN == 0 && TOK_MAX == 1 && TOK_MEAN == 2, "prefilter_plan.h restates the kernels' geometry");
// Stage 1: the 56 instances of prefilter_kernel, each named once.  Row (sel, bf) x MODE 0 1 2 x LO; TOK and TOK + CNT: MODE 1 and 2 only.
constexpr int stage1_index(int mode, bool lo, bool sel, bool bf, bool tok, bool cnt) { return ((((tok + cnt) * 3 + mode) * 2 + lo) * 2 + sel) * 2 + bf; }
template <int I>
constexpr auto stage1_instance() {
    constexpr int family = I / 24, mode = I / 8 % 3;
    constexpr bool lo = I / 4 % 2, sel = I / 2 % 2, bf = I % 2;
    if constexpr (family > 0 && mode == 0) return nullptr;
    else return &prefilter_kernel<mode, lo, sel, bf, (family > 0), (family > 1)>;
}
using Stage1Fn = decltype(stage1_instance<0>());
template <int... I>
constexpr std::array<Stage1Fn, sizeof...(I)> stage1_table(std::integer_sequence<int, I...>) { return {{stage1_instance<I>()...}}; }
constexpr auto STAGE1 = stage1_table(std::make_integer_sequence<int, 72>{});

// Stage 2's instances.  The re-scores differ in their bank's element type, so they are launched through their addresses (launch_like).
using SelectFn = decltype(&select_kernel<false>);
constexpr SelectFn SELECT[2] = {select_kernel<false>, select_kernel<true>};                                        // [sel]
const void *const RESCORE[3][2] = {{(const void *)rescore_kernel<false>, (const void *)rescore_kernel<true>},      // [bank][few = sel]
                                   {(const void *)rescore_lp_kernel<false>, (const void *)rescore_lp_kernel<true>},
                                   {(const void *)rescore_bf_kernel<false>, (const void *)rescore_bf_kernel<true>}};
const void *const TOKEN_RESCORE[2][2] = {{(const void *)token_rescore_lp_kernel, (const void *)token_rescore_bf_kernel},     // [topt][bf]
                                         {(const void *)token_rescore_top_lp_kernel, (const void *)token_rescore_top_bf_kernel}};
const void *const TOKEN_RESCORE_MAP[2] = {(const void *)token_rescore_map_lp_kernel, (const void *)token_rescore_map_bf_kernel};   // [bf]
const void *const TOKEN_RESCORE_MSE_PQ[2] = {(const void *)token_rescore_mse_pq_lp_kernel, (const void *)token_rescore_mse_pq_bf_kernel};   // [bf]
const void *const TOKEN_RESCORE_MSE[2][2] = {{(const void *)token_rescore_mse_lp_kernel, (const void *)token_rescore_mse_bf_kernel},   // [topt][bf]
                                             {(const void *)token_rescore_mse_top_lp_kernel, (const void *)token_rescore_mse_top_bf_kernel}};
const void *const TOKEN_RESCORE_MSE_MEAN[2] = {(const void *)token_rescore_mse_mean_lp_kernel, (const void *)token_rescore_mse_mean_bf_kernel};   // [bf]

// the pointer arguments of an entry point; NULL where it has none
struct SearchArgs {
    const float *tw, *qn, *bank, *xn;
    const void *bank16;
    int dtype;                                 // of bank16 as the caller gave it (a request's bank is -1 when it is neither 16-bit format)
    const void *tail, *pooled;
    const float *rowp;
    const int *tiles;
    int64_t idx_offset;
    const float *thr0;
    void *ws;
    int64_t ws_bytes;
    float *out_s;
    int64_t *out_i;
    int *redo;
    void *stream;
    // 'mean' over a compacted selection (skyemb_cosine_topk_tokens_mean_prefiltered_sel; NULL / 0 everywhere else): the request's N is
    // the S compacted rows stage 1 walks, map their images, bank_N the bank's image count, who the entry's own name
    const int *map;
    int64_t bank_N;
    const char *who;
    // weighted MSE (skyemb_distance_topk_tokens_prefiltered and its _top / _sel / _top_sel forms; NULL everywhere else): the weights
    // c [D]; tw then holds the raw queries t, rowp is skyemb_token_mse_rowp's (under a selection: its masked copy), qn and xn are NULL,
    // and the result is in key space (key = -distance).  With a 'mean' request (skyemb_distance_topk_tokens_mean_prefiltered): pooled,
    // tail and rowp are those of skyemb_token_mse_mean_pool / _rowp, and the constants are the MSE mean bound's
    const float *cw;
    // per-query weights (skyemb_distance_topk_tokens_prefiltered_pq; NULL everywhere else): the image [r.N * r.P, r.D] of
    // skyemb_token_mse_pq_image, r.D = 2 D twice the bank's row length and r.N its images padded to whole tiles.  Stage 1 multiplies
    // the image at r.D, stage 2 re-scores the bank [bank_N, P, D] at D; cw is c [Q, D], tw the raw queries t [Q, D]
    const void *image;
};

int bank_of(int dtype) { return dtype == SKYEMB_BF16 ? SKYEMB_PF_BANK_BF16 : dtype == SKYEMB_F16 ? SKYEMB_PF_BANK_F16 : -1; }
// the entry point a request is reported under (dtype SKYEMB_F16 of a `_resident` entry IS the `_lp` entry; top_t == 0 IS the plain one)
const char *who_of(const skyemb_prefilter_request_t &r) {
    if (r.kind == SKYEMB_PF_TOKENS_MEAN) return "skyemb_cosine_topk_tokens_mean_prefiltered";
    if (r.kind == SKYEMB_PF_TOKENS)
        return r.sel ? (r.top_t ? "skyemb_cosine_topk_tokens_prefiltered_top_sel" : "skyemb_cosine_topk_tokens_prefiltered_sel")
                     : (r.top_t ? "skyemb_cosine_topk_tokens_prefiltered_top" : "skyemb_cosine_topk_tokens_prefiltered");
    if (r.bank == SKYEMB_PF_BANK_F32) return r.sel ? "skyemb_cosine_topk_prefiltered_sel" : "skyemb_cosine_topk_prefiltered";
    if (r.bank == SKYEMB_PF_BANK_F16) return r.sel ? "skyemb_cosine_topk_prefiltered_lp_sel" : "skyemb_cosine_topk_prefiltered_lp";
    return r.sel ? "skyemb_cosine_topk_prefiltered_resident_sel" : "skyemb_cosine_topk_prefiltered_resident";
}

// SKYEMB_PREFILTER_LO as the planner takes it (read per call on purpose: a sub-microsecond scan, and the tests switch it)
int lo_of_env() {
    const char *lo_env = getenv("SKYEMB_PREFILTER_LO");
    return lo_env && lo_env[0] == '0' ? 0 : lo_env && lo_env[0] == '1' ? 1 : SKYEMB_PF_LO_UNSET;
}

// sky_prefilter_plan with its refusals put into words; no device is touched
int plan_or_refuse(const skyemb_prefilter_request_t &r, const char *who, skyemb_prefilter_plan_t *p) {
    const bool rows = r.kind == SKYEMB_PF_ROWS;
    const long long N = (long long)r.N, tiles_all = (long long)ceil_div64(rows ? r.N : r.N * r.P, BT);
    const int code = pfplan::sky_prefilter_plan(r, p);
    const char *prepare = rows ? "skyemb_prefilter_select_prepare" : "skyemb_token_prefilter_select_prepare";
    if (code == pfplan::PF_OK) return 0;
    if (code == pfplan::PF_ROWS_SHAPE)
        skyemb_set_error("%s: outside the prefiltered subset (Q >= 17, D %% 32 == 0, k <= %d, N >= %d)", who, RESCORE_MAX - 64, 8 * BT);
    else if (code == pfplan::PF_MEAN_COMBINE)
        skyemb_set_error("%s: combine code %d: this entry combines by mean (min and max are served by skyemb_cosine_topk_tokens_prefiltered)",
                         who, r.combine);
    else if (code == pfplan::PF_MEAN_SHAPE) skyemb_set_error("%s: " TOKEN_MEAN_PREFILTER_MSG, who, TOK_KMAX, r.Q, N, r.P, r.D, r.k);
    else if (code == pfplan::PF_TOPT_MEAN) skyemb_set_error("%s: " TOKEN_TOPT_MEAN_MSG, who);
    else if (code == pfplan::PF_TOKENS_COMBINE)
        skyemb_set_error("%s: combine code %d: this entry combines by min or max (mean is served by "
                         "skyemb_cosine_topk_tokens_mean_prefiltered)", who, r.combine);
    else if (code == pfplan::PF_TOKENS_SHAPE) skyemb_set_error("%s: " TOKEN_PREFILTER_MSG, who, TOK_KMAX, r.Q, N, r.P, r.D, r.k);
    else if (code == pfplan::PF_TOPT_RANGE)
        skyemb_set_error("%s: top_t must be 0 (all tokens) or 1 .. min(P, 16) (top_t=%d P=%d)", who, r.top_t, r.P);
    else if (code == pfplan::PF_SEL_INFO)
        skyemb_set_error("%s: n_live = %d, last_live = %d: expected 1 .. %lld live tiles and a flag (%s's info)", who, r.n_live, r.last_live,
                         tiles_all, prepare);
    else if (code == pfplan::PF_SEL_ONLY_TAIL && rows)
        skyemb_set_error("%s: the selection's only live tile is the resident bank's tail tile; the phases need a whole live tile", who);
    else if (code == pfplan::PF_SEL_ONLY_TAIL)
        skyemb_set_error("%s: the selection's only live tile is the bank's tail tile; the slices need a whole live tile", who);
    else if (code == pfplan::PF_SEL_DIRECT)
        skyemb_set_error("%s: the first slice ends at position %d, expected 1 .. n_live = %d", who, r.direct_sel, r.n_live);
    else if (code == pfplan::PF_TOO_LARGE && rows)
        skyemb_set_error("%s: Q x N too large: ceil(N / 2048) * ceil(Q / %d) * (D / 32) must stay below 2^31, the range of stage 1's work-item "
                         "and k-step counters (Q=%d N=%lld D=%d); search the queries in batches", who, qtile(p->use_lo), r.Q, N, r.D);
    else if (code == pfplan::PF_TOO_LARGE)
        skyemb_set_error("%s: Q x N P too large: ceil(N P / 2048) * ceil(Q / %d) * (D / 32) must stay below 2^31 (Q=%d N=%lld P=%d D=%d); search the "
                         "queries in batches", who, qtile(p->use_lo), r.Q, N, r.P, r.D);
    else
        skyemb_set_error("skyemb_prefilter_plan: no entry point takes this request (kind=%d bank=%d lo=%d sel=%d has_thr0=%d)", r.kind, r.bank,
                         r.lo, r.sel, r.has_thr0);
    return 1;
}

// Launch `kernel` through its address with the parameter list of `like`: the arguments convert to like's parameter types, so number and types are
// checked at compile time (a re-score table's kernels share one *_PARAMS text and differ only in the bank's element type; errors: SKY_LAUNCH_CHECK)
template <typename... P>
void launch_like(void (*like)(P...), const void *kernel, unsigned grid, size_t lds, hipStream_t st, std::common_type_t<P>... a) {
    void *args[] = {(void *)&a...};
    (void)hipLaunchKernel(kernel, dim3(grid), dim3(256), args, lds, st);
}

#if defined(PF_STAMP) || defined(PF_CLOCK)
// the diagnostic builds (-DPF_CLOCK / -DPF_STAMP): stage 1 adds to 32 counters, zeroed before every slice, read back and printed after it
unsigned long long *pf_dbg() {
    static unsigned long long *dbg = nullptr;
    if (!dbg) { hipMalloc(&dbg, 32 * 8); }
    return dbg;
}
void pf_dbg_report(hipStream_t st, int p, int mode, int Q, const Workspace &w) {
    unsigned long long h[32];
    hipStreamSynchronize(st);
    hipMemcpy(h, pf_dbg(), sizeof(h), hipMemcpyDeviceToHost);
#ifdef PF_CLOCK
    if (h[23])
        fprintf(stderr, "[clock] phase %d (%s): in-kernel clock %.3f GHz over %.2f ms, %.0f shader cycles per k-step (256 MFMAs = 64 per SIMD x 16 cycles = 1024 at the "
                        "matrix pipe's rate), steps/wg %.0f\n",
                p, mode == 0 ? "take-all" : mode == 1 ? "direct append" : "staged", (double)h[20] / (double)h[21] * 0.1, (double)h[21] / h[23] * 1e-5,
                (double)h[20] / (double)h[22], (double)h[22] / h[23]);
#endif
#ifdef PF_STAMP
    const double n = (double)h[16] * 4.0;     // steps summed over workgroups x 4 waves per group
    if (mode == 2) {
        int hc[PF_GRID];
        hipMemcpy(hc, w.wg_count, sizeof(hc), hipMemcpyDeviceToHost);
        long tot = 0; int mx = 0;
        for (int i = 0; i < PF_GRID; ++i) { tot += hc[i]; if (hc[i] > mx) mx = hc[i]; }
        fprintf(stderr, "[stamp] phase %d staged candidates: total %ld (%.1f per query), max per workgroup %d of %d\n", p, tot, (double)tot / Q, mx, w.capw);
    }
    fprintf(stderr, "[stamp] phase %d steps/wg %.0f | early: wait %.0f P0 %.0f read+issue %.0f P1 %.0f mult %.0f | late: wait %.0f P0 %.0f read+issue %.0f P1 %.0f mult %.0f (cycles of s_memtime per k-step)\n",
            p, (double)h[16] / 256.0, h[0] / n, h[1] / n, h[2] / n, h[3] / n, h[4] / n, h[8] / n, h[9] / n, h[10] / n, h[11] / n, h[12] / n);
    const double ni = (double)h[17] * 4.0;    // items summed over workgroups x 4 waves per group
    fprintf(stderr, "[stamp] phase %d items/wg %.0f | item epilogue, cycles per item: early tests %.0f appends %.0f zero %.0f | late tests %.0f appends %.0f zero %.0f\n",
            p, (double)h[17] / 256.0, h[5] / ni, h[6] / ni, h[7] / ni, h[13] / ni, h[14] / ni, h[15] / ni);
#endif
}
#endif

int search(skyemb_prefilter_request_t r, const SearchArgs &a) {
    const char *who = a.who ? a.who : who_of(r);
    const bool rows = r.kind == SKYEMB_PF_ROWS, mean = r.kind == SKYEMB_PF_TOKENS_MEAN;
    SKY_CHECK_ARG(r.bank >= 0, "%s: dtype " RESIDENT_DTYPE_MSG, who, a.dtype);
    SKY_CHECK_ARG(a.tw && (a.cw || (a.qn && a.xn)) && a.bank16 && a.rowp && a.ws && a.out_s && a.out_i && a.redo &&
                      (r.bank != SKYEMB_PF_BANK_F32 || a.bank) && (!r.sel || a.tiles) && (!mean || a.pooled), "%s: null argument", who);
    r.lo = lo_of_env();
    skyemb_prefilter_plan_t p;
    if (plan_or_refuse(r, who, &p)) return 1;
    const int Q = r.Q, D = r.D, k = r.k, bank = r.bank;
    const bool pq = a.image != nullptr;                        // per-query weights: stage 1 over the image at D = 2 Dr, stage 2 over the bank at Dr
    const int Dr = pq ? D / 2 : D;                             // the row length of the bank stage 2 reads
    const void *s1_bank = pq ? a.image : mean ? a.pooled : a.bank16;          // the rows stage 1 multiplies
    if (bank != SKYEMB_PF_BANK_F32) {
        SKY_CHECK_ARG(p.rows % BT == 0 || a.tail, rows ? "%s: N = %lld is no whole number of %d-row tiles: the tail tile of %s is needed"
                                                       : "%s: %lld rows are no whole number of %d-row tiles: the tail tile of %s is needed",
                      who, (long long)p.rows, BT, a.map ? "skyemb_token_mean_select_gather" : mean && a.cw ? "skyemb_token_mse_mean_pool" : mean ? "skyemb_token_mean_pool" : rows && bank == SKYEMB_PF_BANK_F16 ? "skyemb_bank16_rowp_lp"
                                                                                                                      : "skyemb_resident_rowp");
        SKY_CHECK_ARG(aligned16(a.bank16) && aligned16(a.tail) && aligned16(s1_bank), "%s: the bank and the tail tile must be 16-byte aligned",
                      who);
    }
    SKY_CHECK_ARG(a.ws_bytes >= (rows ? skyemb_topk_prefilter_ws_bytes(Q, D, k) : skyemb_token_prefilter_ws_bytes(Q, D, k)),
                  "%s: workspace too small", who);
    hipStream_t st = (hipStream_t)a.stream;
    Workspace w;
    const int64_t used = carve((char *)a.ws, Q, D, p.cap, &w);
    unsigned long long *list = (unsigned long long *)((char *)a.ws + used);     // token routes: the running lists (lengths: nsel) follow
    // the LDS limits this request's instances need: both variants of every mode of its family, as ever
    int rc = 0;
    for (int mode = rows ? 0 : 1; mode <= 2; ++mode)
        for (int lo = 0; lo <= 1; ++lo)
            for (int s = rows ? 0 : p.sel; s <= p.sel; ++s)    // (a row search under a selection launches its tail through the non-SEL instance)
                if (rc == 0) rc = sky_set_lds_limit((const void *)STAGE1[stage1_index(mode, lo, s, p.bf, p.tok, p.cnt)], p.lds_stage1_limit, who);
    const bool mse = a.cw != nullptr;                          // weighted MSE: its own constants and re-score, [D] more floats of LDS for c
    const void *token_rescore = pq ? TOKEN_RESCORE_MSE_PQ[p.bf] : mse && mean ? TOKEN_RESCORE_MSE_MEAN[p.bf] : mse ? TOKEN_RESCORE_MSE[p.top_t != 0][p.bf] : a.map ? TOKEN_RESCORE_MAP[p.bf] : TOKEN_RESCORE[p.top_t != 0][p.bf];
    // (per-query weights: the plan's t [2 Dr] IS t [Dr] beside c_q [Dr], within LDS_TOKEN_RESCORE_LIMIT as it stands)
    const int lds_close = p.lds_close + (mse && !pq ? D * 4 : 0), lds_close_limit = p.lds_close_limit + (mse && !pq ? 4096 * 4 : 0);
    const float gamma_mse = (float)((mean ? gamma_mse_mean_of(Dr, r.P) : gamma_mse_of(Dr)) * (1.0 + 1e-6));
    if (rc == 0) rc = sky_set_lds_limit(rows ? (const void *)SELECT[0] : token_rescore, lds_close_limit, who);
    if (rc == 0 && rows && p.sel) rc = sky_set_lds_limit((const void *)SELECT[1], p.lds_close_limit, who);
    if (rc != 0) return rc;
    const dim3 qgrid((unsigned)((p.q_padded + 3) / 4));
    if (mse) {
        // (the plan's own eps_a is the cosine bound's: under MSE the eps of the route is computed here, beside eps_mse_of)
        const float eps_mse = (float)((pq ? eps_pq_of(Dr, p.use_lo, p.bf) : mean ? eps_mse_mean_of(D, p.use_lo, p.bf) : eps_mse_of(D, p.use_lo, p.bf)) *
                                      (1.0 + 1e-6));
        if (pq && p.bf) hipLaunchKernelGGL(mse_pq_query_kernel<true>, qgrid, dim3(256), 0, st, a.cw, a.tw, Q, Dr, w.qh, w.ql, w.qbase, eps_mse);
        else if (pq) hipLaunchKernelGGL(mse_pq_query_kernel<false>, qgrid, dim3(256), 0, st, a.cw, a.tw, Q, Dr, w.qh, w.ql, w.qbase, eps_mse);
        else if (p.bf) hipLaunchKernelGGL(mse_query_kernel<true>, qgrid, dim3(256), 0, st, a.cw, a.tw, Q, D, w.qh, w.ql, w.qbase, eps_mse);
        else hipLaunchKernelGGL(mse_query_kernel<false>, qgrid, dim3(256), 0, st, a.cw, a.tw, Q, D, w.qh, w.ql, w.qbase, eps_mse);
        hipLaunchKernelGGL(mse_state_kernel, dim3((unsigned)((p.q_padded + 255) / 256)), dim3(256), 0, st, Q, p.q_padded, a.thr0, (const float4 *)w.qbase,
                           (float)Dr, gamma_mse, w.qpar, w.tau, w.cnt, w.nsel, w.overflow, p.bf ? ldexpf(1.0f, -BF_SCALE_LO) : 0.f,
                           ldexpf(1.0f, p.bf ? BF_SCALE_HI : MSE_SCALE_HI_F16));
    } else if (p.bf) hipLaunchKernelGGL(query16_kernel<true>, qgrid, dim3(256), 0, st, a.tw, a.qn, Q, D, w.qh, w.ql, w.qbase, p.eps_a_f32);
    else hipLaunchKernelGGL(query16_kernel<false>, qgrid, dim3(256), 0, st, a.tw, a.qn, Q, D, w.qh, w.ql, w.qbase, p.eps_a_f32);
    if (!mse)
        hipLaunchKernelGGL(init_state_kernel, dim3((unsigned)((p.q_padded + 255) / 256)), dim3(256), 0, st, Q, p.q_padded, a.thr0, w.qbase, r.eps,
                           w.qpar, w.tau, w.cnt, w.overflow, p.first_rows, p.bf ? ldexpf(1.0f, -BF_SCALE_LO) : 0.f,
                           p.bf ? ldexpf(1.0f, BF_SCALE_HI) : 0x1p126f);
    if (!rows && !mse)
        hipLaunchKernelGGL(token_state_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, Q, (const float4 *)w.qbase, w.tau, w.nsel,
                           w.overflow, p.gfac, w.qpar);
    // one stage-1 launch over positions [t0, t1) of `base`: of the live-tile list with the SEL instance, else the bank tiles themselves
    auto stage1 = [&](int mode, bool sel, const void *base, int t0, int t1) {
        const Stage1Fn kernel = STAGE1[stage1_index(mode, p.use_lo, sel, p.bf, p.tok, p.cnt)];
        auto go = [&](auto... dbg) {
            hipLaunchKernelGGL(kernel, dim3(PF_GRID), dim3(NT), p.lds_stage1, st, w.qh, w.ql, (const half_t *)base, (const float4 *)a.rowp,
                               sel ? a.tiles : (const int *)nullptr, w.qpar, Q, p.rows, D, t0, t1, p.cap, w.cnt, w.cand_i, w.cand_d, w.wg_list,
                               w.wg_count, w.capw, w.overflow, p.tok_word, dbg...);
        };
#if defined(PF_STAMP) || defined(PF_CLOCK)
        go(pf_dbg());
#else
        go();
#endif
    };
    auto token_rescore_as = [&](auto like, int final, auto... top_t) {               // (top_t: what the instance takes behind redo)
        launch_like(like, token_rescore, Q, lds_close, st, a.tw, a.qn, (const half_t *)a.bank16, a.xn, a.map || pq ? a.bank_N : r.N, Dr, p.lgp, p.fold,
                    mse ? gamma_mse : p.gfac, k, r.eps,
                    a.idx_offset, p.cap, w.qbase, w.cnt, w.cand_i, list, w.nsel, w.qpar, w.tau, w.overflow, final, a.out_s, a.out_i, a.redo, top_t...);
    };
    // The kernel addresses tile t at base + t * BT rows, so the base handed over for the tail is the one that puts tile T_tail on
    // `tail` (an address only: it is the single tile of that launch, and under SEL the list's last entry holds T_tail).
    const void *tail_base = (const void *)((uintptr_t)a.tail - (uintptr_t)p.T_tail * BT * D * sizeof(half_t));
    for (int i = 0; i < p.n_slices; ++i) {
        const skyemb_prefilter_slice_t &s = p.slice[i];
#if defined(PF_STAMP) || defined(PF_CLOCK)
        hipMemsetAsync(pf_dbg(), 0, 32 * 8, st);
#endif
        stage1(s.mode, p.sel, s1_bank, s.t0, s.t1);
        if (s.bucket)
            hipLaunchKernelGGL(bucket_kernel, dim3(8, PF_GRID), dim3(256), 0, st, (const uint4 *)w.wg_list, (const int *)w.wg_count, w.capw, p.cap,
                               w.cnt, w.cand_i, w.cand_d);
        // the tail tile: direct appends under the slice's threshold -- at most BT candidates per query behind whatever the lists hold
        if (s.tail) stage1(1, s.tail_sel, tail_base, s.tail_pos, s.tail_pos + 1);
#if defined(PF_STAMP) || defined(PF_CLOCK)
        pf_dbg_report(st, i, s.mode, Q, w);
#endif
        if (rows)
            hipLaunchKernelGGL(SELECT[p.sel], dim3((unsigned)Q), dim3(256), p.lds_close, st, Q, k, p.cap, r.eps, w.qbase, (const float4 *)a.rowp, a.xn,
                               w.cnt, w.cand_i, w.cand_d, w.qpar, w.tau, w.overflow, s.final, w.sel_i, w.nsel, w.bound);
        else if (a.map) token_rescore_as(token_rescore_map_lp_kernel, s.final, a.map, (int)r.N);   // the MAP kernels take map and S last
        else if (pq) token_rescore_as(token_rescore_mse_pq_lp_kernel, s.final, a.cw);               // c [Q, D] last
        else if (mse && p.top_t) token_rescore_as(token_rescore_mse_top_lp_kernel, s.final, p.top_t, a.cw);   // MSE under top_t: top_t, then c
        else if (p.top_t) token_rescore_as(token_rescore_top_lp_kernel, s.final, p.top_t);      // the TOPT kernels take top_t last
        else if (mse) token_rescore_as(token_rescore_mse_lp_kernel, s.final, a.cw);                 // the MSE kernels (mean's too) take c last
        else token_rescore_as(token_rescore_lp_kernel, s.final);
    }
    if (rows)
        launch_like(rescore_kernel<false>, RESCORE[bank][p.sel], Q, p.lds_rescore, st, a.tw, a.qn,
                    (const float *)(bank == SKYEMB_PF_BANK_F32 ? a.bank : a.bank16), a.xn, Q, D, k, r.eps, a.idx_offset, w.sel_i, w.nsel, w.bound,
                    w.overflow, a.out_s, a.out_i, a.redo);
    SKY_LAUNCH_CHECK(who);
    return 0;
}

skyemb_prefilter_request_t request(int kind, int bank, int Q, int64_t N, int P, int D, int k, int combine, int top_t, float eps, const float *thr0,
                                   bool sel = false, int n_live = 0, int last_live = 0, int direct_sel = 0) {
    return {kind, bank, Q, P, D, k, N, combine, top_t, thr0 != nullptr, sel, n_live, last_live, direct_sel, 0, eps};
}

}  // namespace

extern "C" int skyemb_prefilter_plan(const skyemb_prefilter_request_t *req, skyemb_prefilter_plan_t *out) {
    if (!req || !out) return skyemb_set_error("skyemb_prefilter_plan: null argument"), 1;
    skyemb_prefilter_request_t r = *req;
    if (r.lo == -1) r.lo = lo_of_env();
    return plan_or_refuse(r, who_of(r), out);
}

extern "C" int skyemb_cosine_topk_prefiltered(const float *tw, const float *qn, int Q, const float *bank, const float *xn, const void *bank16,
                                              const float *rowp, int64_t N, int D, int k, float eps, int64_t idx_offset, const float *thr0,
                                              void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo, void *stream) {
    return search(request(SKYEMB_PF_ROWS, SKYEMB_PF_BANK_F32, Q, N, 1, D, k, 0, 0, eps, thr0),
                  {tw, qn, bank, xn, bank16, SKYEMB_F32, nullptr, nullptr, rowp, nullptr, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream});
}

extern "C" int skyemb_cosine_topk_prefiltered_sel(const float *tw, const float *qn, int Q, const float *bank, const float *xn, const void *bank16,
                                                  const float *rowp_sel, const int *tiles, int n_live, int last_live, int64_t N, int D, int k,
                                                  float eps, int64_t idx_offset, void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i,
                                                  int *redo, void *stream) {
    return search(request(SKYEMB_PF_ROWS, SKYEMB_PF_BANK_F32, Q, N, 1, D, k, 0, 0, eps, nullptr, true, n_live, last_live),
                  {tw, qn, bank, xn, bank16, SKYEMB_F32, nullptr, nullptr, rowp_sel, tiles, idx_offset, nullptr, ws, ws_bytes, out_s, out_i, redo, stream});
}

// ---- a resident 16-bit bank of either format (dtype SKYEMB_F16: the _lp entry points, SKYEMB_BF16: the bf16 search) --------------------
extern "C" int skyemb_cosine_topk_prefiltered_resident(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                                       const void *tail, const float *rowp, int64_t N, int D, int k, float eps,
                                                       int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes, float *out_s,
                                                       int64_t *out_i, int *redo, void *stream) {
    return search(request(SKYEMB_PF_ROWS, bank_of(dtype), Q, N, 1, D, k, 0, 0, eps, thr0),
                  {tw, qn, nullptr, xn, bank16, dtype, tail, nullptr, rowp, nullptr, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream});
}

extern "C" int skyemb_cosine_topk_prefiltered_resident_sel(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                                           const void *tail, const float *rowp_sel, const int *tiles, int n_live, int last_live,
                                                           int64_t N, int D, int k, float eps, int64_t idx_offset, void *ws, int64_t ws_bytes,
                                                           float *out_s, int64_t *out_i, int *redo, void *stream) {
    return search(request(SKYEMB_PF_ROWS, bank_of(dtype), Q, N, 1, D, k, 0, 0, eps, nullptr, true, n_live, last_live),
                  {tw, qn, nullptr, xn, bank16, dtype, tail, nullptr, rowp_sel, tiles, idx_offset, nullptr, ws, ws_bytes, out_s, out_i, redo, stream});
}

extern "C" int skyemb_cosine_topk_prefiltered_lp(const float *tw, const float *qn, int Q, const void *bank16, const float *xn, const void *tail,
                                                 const float *rowp, int64_t N, int D, int k, float eps, int64_t idx_offset, const float *thr0,
                                                 void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo, void *stream) {
    return skyemb_cosine_topk_prefiltered_resident(tw, qn, Q, bank16, SKYEMB_F16, xn, tail, rowp, N, D, k, eps, idx_offset, thr0, ws, ws_bytes,
                                                   out_s, out_i, redo, stream);
}

extern "C" int skyemb_cosine_topk_prefiltered_lp_sel(const float *tw, const float *qn, int Q, const void *bank16, const float *xn, const void *tail,
                                                     const float *rowp_sel, const int *tiles, int n_live, int last_live, int64_t N, int D, int k,
                                                     float eps, int64_t idx_offset, void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i,
                                                     int *redo, void *stream) {
    return skyemb_cosine_topk_prefiltered_resident_sel(tw, qn, Q, bank16, SKYEMB_F16, xn, tail, rowp_sel, tiles, n_live, last_live, N, D, k, eps,
                                                       idx_offset, ws, ws_bytes, out_s, out_i, redo, stream);
}

// ---- patch-token banks: min / max, under top_t (0: the plain call), under a selection of images; mean -----------------------------------
extern "C" int skyemb_cosine_topk_tokens_prefiltered_top(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                                         const void *tail, const float *rowp, int64_t N, int P, int D, int k, int combine,
                                                         int top_t, float eps, int64_t idx_offset, const float *thr0, void *ws,
                                                         int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo, void *stream) {
    return search(request(SKYEMB_PF_TOKENS, bank_of(dtype), Q, N, P, D, k, combine, top_t, eps, thr0),
                  {tw, qn, nullptr, xn, bank16, dtype, tail, nullptr, rowp, nullptr, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream});
}

extern "C" int skyemb_cosine_topk_tokens_prefiltered(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                                     const void *tail, const float *rowp, int64_t N, int P, int D, int k, int combine, float eps,
                                                     int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes, float *out_s,
                                                     int64_t *out_i, int *redo, void *stream) {
    return skyemb_cosine_topk_tokens_prefiltered_top(tw, qn, Q, bank16, dtype, xn, tail, rowp, N, P, D, k, combine, 0, eps, idx_offset, thr0, ws,
                                                     ws_bytes, out_s, out_i, redo, stream);
}

extern "C" int skyemb_cosine_topk_tokens_prefiltered_top_sel(const float *tw, const float *qn, int Q, const void *bank16, int dtype,
                                                             const float *xn, const void *tail, const float *rowp_sel, const int *tiles,
                                                             int n_live, int last_live, int direct_end, int64_t N, int P, int D, int k,
                                                             int combine, int top_t, float eps, int64_t idx_offset, const float *thr0, void *ws,
                                                             int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo, void *stream) {
    return search(request(SKYEMB_PF_TOKENS, bank_of(dtype), Q, N, P, D, k, combine, top_t, eps, thr0, true, n_live, last_live, direct_end),
                  {tw, qn, nullptr, xn, bank16, dtype, tail, nullptr, rowp_sel, tiles, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream});
}

extern "C" int skyemb_cosine_topk_tokens_prefiltered_sel(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                                         const void *tail, const float *rowp_sel, const int *tiles, int n_live, int last_live,
                                                         int direct_end, int64_t N, int P, int D, int k, int combine, float eps,
                                                         int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes, float *out_s,
                                                         int64_t *out_i, int *redo, void *stream) {
    return skyemb_cosine_topk_tokens_prefiltered_top_sel(tw, qn, Q, bank16, dtype, xn, tail, rowp_sel, tiles, n_live, last_live, direct_end, N, P,
                                                         D, k, combine, 0, eps, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream);
}

// (tail and rowp are those of skyemb_token_mean_pool: stage 1's operands are the pooled image's)
extern "C" int skyemb_cosine_topk_tokens_mean_prefiltered(const float *tw, const float *qn, int Q, const void *bank16, int dtype, const float *xn,
                                                          const void *tail, const float *rowp, int64_t N, int P, int D, int k, int combine,
                                                          float eps, int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes,
                                                          float *out_s, int64_t *out_i, int *redo, const void *pooled16, void *stream) {
    return search(request(SKYEMB_PF_TOKENS_MEAN, bank_of(dtype), Q, N, P, D, k, combine, 0, eps, thr0),
                  {tw, qn, nullptr, xn, bank16, dtype, tail, pooled16, rowp, nullptr, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream});
}

// ---- 'mean' under a selection of images: the compacted pooled image, then the unselected search over it ----------------------------------
extern "C" int skyemb_token_mean_select_gather(const void *pooled16, const float *rowp, const int64_t *idx, int64_t N, int64_t S, int D,
                                               int dtype, void *pooled_sel, float *rowp_sel, void *tail_sel, int *map, void *stream) {
    const char *who = "skyemb_token_mean_select_gather";
    SKY_CHECK_ARG(sky_is_lp(dtype), "%s: dtype " RESIDENT_DTYPE_MSG, who, dtype);
    SKY_CHECK_ARG(pooled16 && rowp && idx && pooled_sel && rowp_sel && map, "%s: null argument", who);
    SKY_CHECK_ARG(S >= 1 && S <= N && N < (1ll << 31) && D % BK == 0 && D >= BK && D <= 4096,
                  "%s: expected 1 <= S <= N < 2^31 images, D %% 32 == 0 and D <= 4096 (N=%lld S=%lld D=%d)", who, (long long)N, (long long)S, D);
    SKY_CHECK_ARG(S % BT == 0 || tail_sel, "%s: S = %lld is no whole number of %d-image tiles: a tail tile [%d, D] is needed", who, (long long)S,
                  BT, BT);
    SKY_CHECK_ARG(aligned16(pooled16) && aligned16(pooled_sel) && aligned16(tail_sel), "%s: the pooled image, its compacted copy and the tail "
                  "tile must be 16-byte aligned", who);
    const int64_t padded = skyemb_bank16_rowp_rows(S);
    hipLaunchKernelGGL(token_mean_select_gather_kernel, dim3((unsigned)(padded / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned short *)pooled16, (const float4 *)rowp, idx, N, S, D, (unsigned short *)pooled_sel, (float4 *)rowp_sel, padded,
                       S % BT ? (unsigned short *)tail_sel : nullptr, S / BT * BT, map);
    SKY_LAUNCH_CHECK(who);
    return 0;
}

// (tail_sel, rowp_sel, pooled_sel and map are those of skyemb_token_mean_select_gather; the plan is the unselected mean request over S rows)
extern "C" int skyemb_cosine_topk_tokens_mean_prefiltered_sel(const float *tw, const float *qn, int Q, const void *bank16, int dtype,
                                                              const float *xn, const void *tail_sel, const float *rowp_sel, int64_t N,
                                                              int64_t S, const int *map, int P, int D, int k, int combine, float eps,
                                                              int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes, float *out_s,
                                                              int64_t *out_i, int *redo, const void *pooled_sel, void *stream) {
    const char *who = "skyemb_cosine_topk_tokens_mean_prefiltered_sel";
    SKY_CHECK_ARG(combine == SKYEMB_COMBINE_MEAN, "%s: combine code %d: this entry combines by mean (min and max under a selection are served "
                  "by skyemb_cosine_topk_tokens_prefiltered_sel)", who, combine);
    SKY_CHECK_ARG(S >= 8 * BT, "%s: S = %lld selected images: stage 1 needs S >= %d (the grouped search serves a smaller selection)", who,
                  (long long)S, 8 * BT);
    SKY_CHECK_ARG(k <= S, "%s: k = %d exceeds the S = %lld selected images", who, k, (long long)S);
    SKY_CHECK_ARG(S <= N, "%s: S = %lld selected images of a bank of N = %lld", who, (long long)S, (long long)N);
    SKY_CHECK_ARG(P >= 1 && N * P < (1ll << 31), "%s: N * P must stay below 2^31 token rows (N=%lld P=%d)", who, (long long)N, P);
    SKY_CHECK_ARG(map, "%s: null argument (map)", who);
    return search(request(SKYEMB_PF_TOKENS_MEAN, bank_of(dtype), Q, S, P, D, k, combine, 0, eps, thr0),
                  {tw, qn, nullptr, xn, bank16, dtype, tail_sel, pooled_sel, rowp_sel, nullptr, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream,
                   map, N, who});
}

// ---- weighted MSE over a resident token bank (min | max): the constants and the search ("Weighted MSE" above) -----------------------------
#define TOKEN_MSE_PREFILTER_MSG "many-query weighted-MSE patch-token search: needs P a divisor of 64, D %% 32 == 0, 128 <= D <= 4096, " \
                                "1 <= k <= %d, k <= N, 2048 <= N * P < 2^31 rows and Q >= 1 (Q=%d N=%lld P=%d D=%d k=%d)"
extern "C" int skyemb_token_mse_prefilter_applicable(int Q, int64_t N, int P, int D, int k) {
    const bool ok = pfplan::tokens_shape_ok(Q, N, P, D, k);
    if (!ok) skyemb_set_error(TOKEN_MSE_PREFILTER_MSG, TOK_KMAX, Q, (long long)N, P, D, k);
    return ok ? 1 : 0;
}

extern "C" double skyemb_token_mse_prefilter_eps(int D, int lo, int dtype) { return eps_mse_of(D, lo != 0, dtype == SKYEMB_BF16); }

extern "C" double skyemb_token_mse_prefilter_gamma(int D) { return gamma_mse_of(D); }

extern "C" int skyemb_token_mse_rowp(const void *bank16, int dtype, const float *c, int64_t R, int D, float *rowp, void *tail, void *stream) {
    const char *who = "skyemb_token_mse_rowp";
    SKY_CHECK_ARG(sky_is_lp(dtype), "%s: dtype " RESIDENT_DTYPE_MSG, who, dtype);
    SKY_CHECK_ARG(bank16 && c && rowp && R > 0 && D > 0 && D % BK == 0 && D <= 4096, "%s: bad arguments", who);
    SKY_CHECK_ARG(R % BT == 0 || tail, "%s: %lld rows are no whole number of %d-row tiles: a tail tile [%d, D] is needed", who, (long long)R, BT, BT);
    SKY_CHECK_ARG(aligned16(bank16) && aligned16(tail) && aligned16(c), "%s: the bank, the tail tile and c must be 16-byte aligned", who);
    const int64_t padded = skyemb_bank16_rowp_rows(R);
    const dim3 grid((unsigned)ceil_div64(padded, 4));
    // fp16: one set of row constants serves both variants: the smaller eps_mse (hi + lo) gives the larger, always valid, term
    const float sub_scale = (float)(0x1p-14 / eps_mse_of(D, true, false) * (1.0 + 1e-6));
#define MSE_ROWP_ARGS (const unsigned short *)bank16, c, R, D, (float4 *)rowp, padded, R % BT ? (unsigned short *)tail : nullptr, R / BT * BT, sub_scale
    if (dtype == SKYEMB_BF16) hipLaunchKernelGGL(mse_rowp_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, MSE_ROWP_ARGS);
    else hipLaunchKernelGGL(mse_rowp_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, MSE_ROWP_ARGS);
#undef MSE_ROWP_ARGS
    SKY_LAUNCH_CHECK(who);
    return 0;
}

// (combine is the DISTANCE combine: min -> the key-space MAX fold, max -> the key-space MIN fold; out_s holds keys = -distance)
// One body for the plain call and its _top / _sel / _top_sel forms.  In key space distance 'max' under top_t is 'min' under top_t (the
// top_t-th largest key: the counting fold, the TOPT re-score); distance 'min' is a[0] whatever top_t says, the plain call.  The request
// is the cosine one of the same shape, so the planner decides top_t == P and the selection's limits as it does there.
namespace {
int mse_search(const char *who, const float *c, const float *t, int Q, const void *bank16, int dtype, const float *rowp, const void *tail,
               const int *tiles, bool sel, int n_live, int last_live, int direct_end, int64_t N, int P, int D, int k, int combine, int top_t,
               int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i, int *redo, void *stream) {
    SKY_CHECK_ARG(c && aligned16(c) && aligned16(t), "%s: c and t must be given and 16-byte aligned", who);
    SKY_CHECK_ARG(combine == SKYEMB_COMBINE_MIN || combine == SKYEMB_COMBINE_MAX, "%s: combine code %d: this entry combines by min or max "
                  "(mean is served by skyemb_distance_token_topk)", who, combine);
    if (!skyemb_token_mse_prefilter_applicable(Q, N, P, D, k)) {
        char why[512];
        snprintf(why, sizeof why, "%s", skyemb_last_error());
        skyemb_set_error("%s: %s", who, why);
        return 1;
    }
    SKY_CHECK_ARG(top_t >= 0 && top_t <= (P < 16 ? P : 16), "%s: top_t must be 0 (all tokens) or 1 .. min(P, 16) (top_t=%d P=%d)", who, top_t, P);
    const int key_combine = combine == SKYEMB_COMBINE_MIN ? SKYEMB_COMBINE_MAX : SKYEMB_COMBINE_MIN;
    return search(request(SKYEMB_PF_TOKENS, bank_of(dtype), Q, N, P, D, k, key_combine, key_combine == SKYEMB_COMBINE_MIN ? top_t : 0, 0.f, thr0,
                          sel, n_live, last_live, direct_end),
                  {t, nullptr, nullptr, nullptr, bank16, dtype, tail, nullptr, rowp, tiles, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream,
                   nullptr, 0, who, c});
}
}  // namespace

extern "C" int skyemb_distance_topk_tokens_prefiltered(const float *c, const float *t, int Q, const void *bank16, int dtype, const float *rowp,
                                                       const void *tail, int64_t N, int P, int D, int k, int combine, int64_t idx_offset,
                                                       const float *thr0, void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i,
                                                       int *redo, void *stream) {
    return mse_search("skyemb_distance_topk_tokens_prefiltered", c, t, Q, bank16, dtype, rowp, tail, nullptr, false, 0, 0, 0, N, P, D, k, combine, 0,
                      idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream);
}

// ---- the same search under top_t (distance 'max': a[top_t - 1]) and under a selection of the bank's images ----------------------------------
extern "C" int skyemb_token_mse_topt_prefilter_applicable(int Q, int64_t N, int P, int D, int k, int combine, int top_t) {
    if (combine != SKYEMB_COMBINE_MIN && combine != SKYEMB_COMBINE_MAX) {
        if (combine == SKYEMB_COMBINE_MEAN)
            skyemb_set_error("many-query weighted-MSE patch-token search: combine mean is not served by the two-stage route (the mean of token "
                             "distances is no count of passing rows); the grouped search serves it");
        else skyemb_set_error("many-query weighted-MSE patch-token search: unknown combine code %d", combine);
        return 0;
    }
    if (!skyemb_token_mse_prefilter_applicable(Q, N, P, D, k)) return 0;     // (its own text)
    if (top_t < 1 || top_t > (P < 16 ? P : 16)) {
        skyemb_set_error("many-query weighted-MSE patch-token search: top_t must be 1 .. min(P, 16) (top_t=%d P=%d)", top_t, P);
        return 0;
    }
    return 1;
}

extern "C" int skyemb_distance_topk_tokens_prefiltered_top(const float *c, const float *t, int Q, const void *bank16, int dtype,
                                                           const float *rowp, const void *tail, int64_t N, int P, int D, int k, int combine,
                                                           int top_t, int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes,
                                                           float *out_s, int64_t *out_i, int *redo, void *stream) {
    return mse_search(top_t ? "skyemb_distance_topk_tokens_prefiltered_top" : "skyemb_distance_topk_tokens_prefiltered", c, t, Q, bank16, dtype, rowp,
                      tail, nullptr, false, 0, 0, 0, N, P, D, k, combine, top_t, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream);
}

extern "C" int skyemb_distance_topk_tokens_prefiltered_top_sel(const float *c, const float *t, int Q, const void *bank16, int dtype,
                                                               const float *rowp_sel, const void *tail, const int *tiles, int n_live,
                                                               int last_live, int direct_end, int64_t N, int P, int D, int k, int combine,
                                                               int top_t, int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes,
                                                               float *out_s, int64_t *out_i, int *redo, void *stream) {
    return mse_search(top_t ? "skyemb_distance_topk_tokens_prefiltered_top_sel" : "skyemb_distance_topk_tokens_prefiltered_sel", c, t, Q, bank16, dtype,
                      rowp_sel, tail, tiles, true, n_live, last_live, direct_end, N, P, D, k, combine, top_t, idx_offset, thr0, ws, ws_bytes, out_s,
                      out_i, redo, stream);
}

extern "C" int skyemb_distance_topk_tokens_prefiltered_sel(const float *c, const float *t, int Q, const void *bank16, int dtype,
                                                           const float *rowp_sel, const void *tail, const int *tiles, int n_live, int last_live,
                                                           int direct_end, int64_t N, int P, int D, int k, int combine, int64_t idx_offset,
                                                           const float *thr0, void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i,
                                                           int *redo, void *stream) {
    return skyemb_distance_topk_tokens_prefiltered_top_sel(c, t, Q, bank16, dtype, rowp_sel, tail, tiles, n_live, last_live, direct_end, N, P, D, k,
                                                           combine, 0, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream);
}

// ---- weighted MSE with per-query weights c [Q, D] ("Weighted MSE with PER-QUERY weights" above) --------------------------------------------
#define TOKEN_MSE_PQ_PREFILTER_MSG "many-query weighted-MSE patch-token search with per-query weights: needs P a divisor of 64, D %% 32 == 0, " \
                                   "128 <= D <= 2048 (stage 1 multiplies rows of 2 D), 1 <= k <= %d, k <= N, 2048 <= N * P rows, fewer than 2^31 " \
                                   "rows after padding to whole %d-row tiles, and Q >= 1 (Q=%d N=%lld P=%d D=%d k=%d)"
extern "C" int skyemb_token_mse_pq_prefilter_applicable(int Q, int64_t N, int P, int D, int k) {
    const bool ok = D >= 4 * BK && D <= 2048 && D % BK == 0 && pfplan::tokens_shape_ok(Q, N, P, 2 * D, k) &&
                    skyemb_bank16_rowp_rows(N * P) < (1ll << 31);
    if (!ok) skyemb_set_error(TOKEN_MSE_PQ_PREFILTER_MSG, TOK_KMAX, BT, Q, (long long)N, P, D, k);
    return ok ? 1 : 0;
}

extern "C" double skyemb_token_mse_pq_prefilter_eps(int D, int lo, int dtype) { return eps_pq_of(D, lo != 0, dtype == SKYEMB_BF16); }

extern "C" int skyemb_token_mse_pq_image(const void *bank16, int dtype, int64_t R, int D, void *image, float *rowp, void *stream) {
    const char *who = "skyemb_token_mse_pq_image";
    SKY_CHECK_ARG(sky_is_lp(dtype), "%s: dtype " RESIDENT_DTYPE_MSG, who, dtype);
    SKY_CHECK_ARG(bank16 && image && rowp && R > 0 && D >= 4 * BK && D % BK == 0 && D <= 2048, "%s: bad arguments (R=%lld, D=%d: D %% 32 == 0, "
                  "128 <= D <= 2048)", who, (long long)R, D);
    SKY_CHECK_ARG(aligned16(bank16) && aligned16(image), "%s: the bank and the image must be 16-byte aligned", who);
    const int64_t padded = skyemb_bank16_rowp_rows(R);
    SKY_CHECK_ARG(padded < (1ll << 31), "%s: R = %lld rows: the image must hold fewer than 2^31 rows after padding to whole %d-row tiles", who,
                  (long long)R, BT);
    const dim3 grid((unsigned)ceil_div64(padded, 4));
    // fp16: one image serves both variants: the smaller eps_pq (hi + lo) gives the larger, always valid, term
    const float sub_scale = (float)(0x1p-14 / eps_pq_of(D, true, false) * (1.0 + 1e-6));
    if (dtype == SKYEMB_BF16)
        hipLaunchKernelGGL(mse_pq_image_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short *)bank16, R, D,
                           (unsigned short *)image, (float4 *)rowp, padded, sub_scale);
    else
        hipLaunchKernelGGL(mse_pq_image_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short *)bank16, R, D,
                           (unsigned short *)image, (float4 *)rowp, padded, sub_scale);
    SKY_LAUNCH_CHECK(who);
    return 0;
}

// (combine is the DISTANCE combine, out_s holds keys = -distance, as for skyemb_distance_topk_tokens_prefiltered.  The request plans as
// {tokens, resident, D' = 2 D} over the image's padded images: a bank without a ragged tail, whose padding rows pass no test)
extern "C" int skyemb_distance_topk_tokens_prefiltered_pq(const float *c, const float *t, int Q, const void *bank16, int dtype, const void *image,
                                                          const float *rowp, int64_t N, int P, int D, int k, int combine, int64_t idx_offset,
                                                          const float *thr0, void *ws, int64_t ws_bytes, float *out_s, int64_t *out_i,
                                                          int *redo, void *stream) {
    const char *who = "skyemb_distance_topk_tokens_prefiltered_pq";
    SKY_CHECK_ARG(c && image && aligned16(c) && aligned16(t) && aligned16(image), "%s: c, t and the image must be given and 16-byte aligned", who);
    SKY_CHECK_ARG(combine == SKYEMB_COMBINE_MIN || combine == SKYEMB_COMBINE_MAX, "%s: combine code %d: this entry combines by min or max "
                  "(mean is served by skyemb_distance_token_topk_pq)", who, combine);
    if (!skyemb_token_mse_pq_prefilter_applicable(Q, N, P, D, k)) {
        char why[640];
        snprintf(why, sizeof why, "%s", skyemb_last_error());
        skyemb_set_error("%s: %s", who, why);
        return 1;
    }
    const int key_combine = combine == SKYEMB_COMBINE_MIN ? SKYEMB_COMBINE_MAX : SKYEMB_COMBINE_MIN;
    const int64_t N_padded = skyemb_bank16_rowp_rows(N * P) / P;
    return search(request(SKYEMB_PF_TOKENS, bank_of(dtype), Q, N_padded, P, 2 * D, k, key_combine, 0, 0.f, thr0),
                  {t, nullptr, nullptr, nullptr, bank16, dtype, nullptr, nullptr, rowp, nullptr, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo, stream,
                   nullptr, N, who, c, image});
}

// ---- weighted MSE under combine 'mean' ("Weighted MSE under combine 'mean'" above): the pooled image, its constants, the search -----------
#define TOKEN_MSE_MEAN_PREFILTER_MSG "many-query weighted-MSE patch-token search, combine mean: needs P a divisor of 64, D %% 32 == 0, " \
                                     "128 <= D <= 4096, 1 <= k <= %d, k <= N, N >= 2048 images, N * P < 2^31 rows and Q >= 1 " \
                                     "(Q=%d N=%lld P=%d D=%d k=%d)"
extern "C" int skyemb_token_mse_mean_prefilter_applicable(int Q, int64_t N, int P, int D, int k) {
    const bool ok = pfplan::mean_shape_ok(Q, N, P, D, k);
    if (!ok) skyemb_set_error(TOKEN_MSE_MEAN_PREFILTER_MSG, TOK_KMAX, Q, (long long)N, P, D, k);
    return ok ? 1 : 0;
}

extern "C" double skyemb_token_mse_mean_prefilter_eps(int D, int lo, int dtype) { return eps_mse_mean_of(D, lo != 0, dtype == SKYEMB_BF16); }

extern "C" double skyemb_token_mse_mean_prefilter_gamma(int D, int P) { return gamma_mse_mean_of(D, P); }

namespace {
int mse_mean_shape(const char *who, int dtype, int64_t N, int P, int D) {
    SKY_CHECK_ARG(sky_is_lp(dtype), "%s: dtype " RESIDENT_DTYPE_MSG, who, dtype);
    SKY_CHECK_ARG(N > 0 && P >= 1 && P <= 64 && 64 % P == 0 && D % BK == 0 && D >= BK && D <= 4096 && N * P < (1ll << 31),
                  "%s: expected P a divisor of 64, D %% 32 == 0, D <= 4096 and fewer than 2^31 token rows (N=%lld P=%d D=%d)", who,
                  (long long)N, P, D);
    return 0;
}
}  // namespace

extern "C" int skyemb_token_mse_mean_pool(const void *bank16, int dtype, int64_t N, int P, int D, void *pooled16, float *paux, void *tail,
                                          void *stream) {
    const char *who = "skyemb_token_mse_mean_pool";
    if (mse_mean_shape(who, dtype, N, P, D)) return 1;
    SKY_CHECK_ARG(bank16 && pooled16 && paux, "%s: null argument", who);
    SKY_CHECK_ARG(N % BT == 0 || tail, "%s: N = %lld is no whole number of %d-image tiles: a tail tile [%d, D] is needed", who, (long long)N,
                  BT, BT);
    SKY_CHECK_ARG(aligned16(bank16) && aligned16(pooled16) && aligned16(tail), "%s: the bank, the pooled image and the tail tile must be "
                  "16-byte aligned", who);
    const int64_t padded = skyemb_bank16_rowp_rows(N);
    const bool bf = dtype == SKYEMB_BF16;
    // one image serves both variants: the smaller eps_m (hi + lo) gives the larger, always valid, pooling term
    const float kfac = (float)(kappa_mse_mean_of(P) / eps_m_of(D, true, bf) * (1.0 + 1e-6));
    const dim3 grid((unsigned)(padded / 2));
#define POOL_ARGS (const unsigned short *)bank16, N, P, D, (unsigned short *)pooled16, (float2 *)paux, padded, \
                  N % BT ? (unsigned short *)tail : nullptr, N / BT * BT, kfac
    if (bf) hipLaunchKernelGGL(token_mse_mean_pool_kernel<true>, grid, dim3(128), 0, (hipStream_t)stream, POOL_ARGS);
    else hipLaunchKernelGGL(token_mse_mean_pool_kernel<false>, grid, dim3(128), 0, (hipStream_t)stream, POOL_ARGS);
#undef POOL_ARGS
    SKY_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int skyemb_token_mse_mean_rowp(const void *bank16, int dtype, const float *c, const float *paux, int64_t N, int P, int D,
                                          float *rowp, void *stream) {
    const char *who = "skyemb_token_mse_mean_rowp";
    if (mse_mean_shape(who, dtype, N, P, D)) return 1;
    SKY_CHECK_ARG(bank16 && c && paux && rowp, "%s: null argument", who);
    SKY_CHECK_ARG(aligned16(bank16) && aligned16(c), "%s: the bank and c must be 16-byte aligned", who);
    const int64_t padded = skyemb_bank16_rowp_rows(N);
    const dim3 grid((unsigned)(padded / 4));
#define ROWP_ARGS (const unsigned short *)bank16, c, (const float2 *)paux, N, P, D, (float4 *)rowp, padded
    if (dtype == SKYEMB_BF16) hipLaunchKernelGGL(token_mse_mean_rowp_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, ROWP_ARGS);
    else hipLaunchKernelGGL(token_mse_mean_rowp_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, ROWP_ARGS);
#undef ROWP_ARGS
    SKY_LAUNCH_CHECK(who);
    return 0;
}

// (pooled16 and tail are those of skyemb_token_mse_mean_pool, rowp that of skyemb_token_mse_mean_rowp under the same c; out_s holds keys =
// -distance.  The request plans as the cosine mean's: {SKYEMB_PF_TOKENS_MEAN, the bank's format, D}, eps = 0)
extern "C" int skyemb_distance_topk_tokens_mean_prefiltered(const float *c, const float *t, int Q, const void *bank16, int dtype,
                                                            const void *pooled16, const void *tail, const float *rowp, int64_t N, int P,
                                                            int D, int k, int64_t idx_offset, const float *thr0, void *ws, int64_t ws_bytes,
                                                            float *out_s, int64_t *out_i, int *redo, void *stream) {
    const char *who = "skyemb_distance_topk_tokens_mean_prefiltered";
    SKY_CHECK_ARG(c && aligned16(c) && aligned16(t), "%s: c and t must be given and 16-byte aligned", who);
    if (!skyemb_token_mse_mean_prefilter_applicable(Q, N, P, D, k)) {
        char why[512];
        snprintf(why, sizeof why, "%s", skyemb_last_error());
        skyemb_set_error("%s: %s", who, why);
        return 1;
    }
    return search(request(SKYEMB_PF_TOKENS_MEAN, bank_of(dtype), Q, N, P, D, k, SKYEMB_COMBINE_MEAN, 0, 0.f, thr0),
                  {t, nullptr, nullptr, nullptr, bank16, dtype, tail, pooled16, rowp, nullptr, idx_offset, thr0, ws, ws_bytes, out_s, out_i, redo,
                   stream, nullptr, 0, who, c});
}
