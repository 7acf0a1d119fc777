// Per-image combine of token scores shared by the patch-token kernels (topk_tokens.hip: weighted cosine; distance_tokens.hip:
// weighted MSE / MAE in key space, key = -distance): the plain min | mean | max fold of a 16-row tile and the top-t combine (bitonic
// sort over DPP lane permutes).  A tile is 16 bank rows, one per lane n = lane & 15 of each of the four lane groups g = lane >> 4;
// an image is tp = min(P, 16) neighbouring lanes.  The orders these functions fix are stated in topk_tokens.hip and
// include/skyemb.h.
#pragma once
#include "common.h"

template <int COMBINE>
__device__ __forceinline__ float combine_start() {
    return COMBINE == SKYEMB_COMBINE_MIN ? INFINITY : (COMBINE == SKYEMB_COMBINE_MAX ? -INFINITY : 0.f);
}

// folds the token scores `s` of the tp (1, 2, 4, 8 or 16) lanes this image has in the current tile into `carry`
template <int COMBINE>
__device__ __forceinline__ float combine_tile(float s, float carry, int lane, int tp) {
    if (COMBINE == SKYEMB_COMBINE_MEAN) {
        const int base = lane & ~(tp - 1);
        float acc = carry;
        for (int j = 0; j < tp; ++j) acc = acc + __shfl(s, base + j, 64);
        return acc;
    }
    float v = s;
    for (int o = 1; o < tp; o <<= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = COMBINE == SKYEMB_COMBINE_MIN ? fminf(v, u) : fmaxf(v, u);
    }
    return COMBINE == SKYEMB_COMBINE_MIN ? fminf(carry, v) : fmaxf(carry, v);
}

// the value of lane (lane ^ j), j in {1, 2, 4, 8, 15} (a constant once the callers' loops are unrolled), with every lane active:
// DPP quad / row permutes and, for 4, a swizzle -- no address register, which __shfl_xor's bpermute would keep live per j
__device__ __forceinline__ float lane_xor(float v, int j) {
    const int x = __float_as_int(v);
    switch (j) {
    case 1: return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false));    // quad_perm:[1,0,3,2]
    case 2: return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false));    // quad_perm:[2,3,0,1]
    case 4: return __int_as_float(__builtin_amdgcn_ds_swizzle(x, 0x101F));                      // bit mode: and 0x1f, or 0, xor 4
    case 8: return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, false));   // row_ror:8
    default: return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, false));  // 15: row_mirror
    }
}

// bitonic sort, descending, of the tp (1, 2, 4, 8 or 16) values an image's lane group holds; i = this lane's place in the group
__device__ __forceinline__ float sort_desc(float v, int i, int tp) {
#pragma unroll
    for (int k = 2; k <= 16; k <<= 1) {
        if (k <= tp) {                                              // wave-uniform
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const float u = lane_xor(v, j);
                v = (((i & k) == 0) == ((i & j) == 0)) ? fmaxf(v, u) : fminf(v, u);   // k == tp: i & k == 0, every block descends
            }
        }
    }
    return v;
}

// bitonic merge, descending, of a bitonic sequence over the 16 lanes of a tile
__device__ __forceinline__ float merge_desc16(float v, int i) {
#pragma unroll
    for (int j = 8; j > 0; j >>= 1) {
        const float u = lane_xor(v, j);
        v = (i & j) == 0 ? fmaxf(v, u) : fminf(v, u);
    }
    return v;
}

// top-t combine of one tile: -> the image's best min(P, 16) scores so far, descending over its lane group (`carry`: those of
// the image's earlier tiles, unused on its first tile)
__device__ __forceinline__ float top_tile(float s, float carry, int n_lane, int tp, bool first_tile) {
    float v = sort_desc(s, n_lane & (tp - 1), tp);
    if (!first_tile) v = merge_desc16(fmaxf(carry, lane_xor(v, 15)), n_lane);   // wave-uniform; only P >= 32 gets here
    return v;
}

// the combined score from the sorted scores `v` of a finished image: lanes base .. base + top_t - 1 hold d[0] .. d[top_t-1]
template <int COMBINE>
__device__ __forceinline__ float top_finish(float v, int lane, int tp, int top_t) {
    const int base = lane & ~(tp - 1);
    if (COMBINE == SKYEMB_COMBINE_MIN) return __shfl(v, base + top_t - 1, 64);
    float acc = 0.f;
    for (int j = 0; j < top_t; ++j) acc = acc + __shfl(v, base + j, 64);
    const float c = __fdiv_rn(acc, (float)top_t);
    return c == c ? c : -INFINITY;
}

// ---- host side, shared by topk_tokens.hip and distance_tokens.hip: the launch geometry of the two searches, stated once, and the
// dispatch on a bank's element type

inline int64_t image_unit(int P) { return P < 16 ? 16 : P; }       // lcm(P, 16) for the accepted P

// rows of one wave when R rows are dealt to `lists` waves: whole images and whole 16-row tiles
inline int64_t token_rows_per_wave(int64_t R, int64_t lists, int P) {
    return ceil_div64(ceil_div64(R, lists), image_unit(P)) * image_unit(P);
}

// workgroups (of four waves) of a scores call: at least 64 rows and one whole image per wave, at most 2048
inline int64_t token_scores_blocks(int64_t R, int P) {
    const int64_t blocks = ceil_div64(ceil_div64(R, image_unit(P) < 64 ? 64 : image_unit(P)), 4);
    return blocks > 2048 ? 2048 : blocks;
}

// f(bank as a pointer to its element type); the caller has refused every other bank_dtype code
template <typename F>
int with_bank_type(const void *bank, int bank_dtype, F &&f) {
    if (bank_dtype == SKYEMB_F32) return f((const float *)bank);
    if (bank_dtype == SKYEMB_BF16) return f((const bf16_t *)bank);
    return f((const f16_t *)bank);
}
