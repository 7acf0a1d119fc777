// Overflow probe of a gradient range: the device side of the dynamic loss scale (sky_embeddings_amd/loss_scale.py).  One HBM-bound
// read of the gradients an optimiser step is about to consume; leaves a flag (any +-inf / NaN) and the largest finite |g| in two
// device words that skyemb_adamw_guarded (adamw.hip) and the host's scale policy read.  Shaped like adamw_kernel: 256 threads,
// grid-stride, two four-element groups in flight per lane, at most 256 * 16 workgroups.
#include "common.h"

namespace {

// the four elements at g + 4 * i as raw words: one 16-byte load (fp32) or one 8-byte load (16-bit formats)
template <int WORDS>
struct GuardWords { uint32_t w[WORDS]; };

template <int WORDS>
__device__ __forceinline__ GuardWords<WORDS> guard_load(const void *g, int64_t i);
template <>
__device__ __forceinline__ GuardWords<4> guard_load<4>(const void *g, int64_t i) {
    const uint4 v = *((const uint4 *)g + i);
    return {{v.x, v.y, v.z, v.w}};
}
template <>
__device__ __forceinline__ GuardWords<2> guard_load<2>(const void *g, int64_t i) {
    const uint2 v = *((const uint2 *)g + i);
    return {{v.x, v.y}};
}

// |x| as an unsigned integer orders like |x| itself (IEEE formats), and "not finite" is "exponent field all ones": the kernel
// works on bit patterns only (exponent masks: fp32 0x7f800000, f16 0x7c00, bf16 0x7f80; +-0 and subnormals are finite).
template <int DT>
__device__ __forceinline__ void guard_word(uint32_t w, uint32_t &bad, uint32_t &amax) {
    if (DT == SKYEMB_F32) {
        const uint32_t a = w & 0x7fffffffu;
        const bool fin = (a & 0x7f800000u) != 0x7f800000u;
        bad |= fin ? 0u : 1u;
        amax = max(amax, fin ? a : 0u);
    } else {
        const uint32_t EXP = DT == SKYEMB_F16 ? 0x7c00u : 0x7f80u;
        const uint32_t lo = w & 0x7fffu, hi = (w >> 16) & 0x7fffu;
        const bool fl = (lo & EXP) != EXP, fh = (hi & EXP) != EXP;
        bad |= (fl && fh) ? 0u : 1u;
        amax = max(amax, max(fl ? lo : 0u, fh ? hi : 0u));
    }
}

// the largest |g| of a 16-bit format as fp32 bits (both conversions are exact and monotonic, so the maximum converts last)
template <int DT>
__device__ __forceinline__ uint32_t guard_as_f32_bits(uint32_t a) {
    if (DT == SKYEMB_F32) return a;
    if (DT == SKYEMB_BF16) return a << 16;
    const unsigned short h = (unsigned short)a;
    return __float_as_uint((float)__builtin_bit_cast(f16_t, h));
}

template <int DT>
__global__ __launch_bounds__(256) void grad_probe_kernel(const void *__restrict__ g, int64_t n4, uint32_t *__restrict__ state) {
    constexpr int WORDS = DT == SKYEMB_F32 ? 4 : 2;
    uint32_t bad = 0, amax = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += 2 * stride) {
        GuardWords<WORDS> v[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t i = i0 + u * stride;
#pragma unroll
            for (int j = 0; j < WORDS; ++j) v[u].w[j] = 0;          // (+0: finite, and no candidate for the maximum)
            if (i < n4) v[u] = guard_load<WORDS>(g, i);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < WORDS; ++j) guard_word<DT>(v[u].w[j], bad, amax);
    }
    // registers -> wave -> LDS -> at most one atomicOr and one atomicMax per workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bad |= (uint32_t)__shfl_xor((int)bad, o, 64);
        amax = max(amax, (uint32_t)__shfl_xor((int)amax, o, 64));
    }
    __shared__ uint32_t s_bad[4], s_max[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_bad[wave] = bad; s_max[wave] = amax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        bad = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
        amax = guard_as_f32_bits<DT>(max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
        // only when they would change something (the words only ever grow, so a stale read costs an atomic, never a result)
        if (bad && __hip_atomic_load(&state[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(&state[0], 1u);
        if (amax > __hip_atomic_load(&state[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&state[1], amax);
    }
}

}  // namespace

extern "C" int skyemb_grad_probe(const void *g, int grad_dtype, int64_t n, uint32_t *state, void *stream) {
    SKY_CHECK_ARG(n > 0 && n % 4 == 0, "skyemb_grad_probe: n must be a positive multiple of 4");
    SKY_CHECK_ARG(grad_dtype == SKYEMB_F32 || sky_is_lp(grad_dtype), "skyemb_grad_probe: bad grad_dtype %d", grad_dtype);
    SKY_CHECK_ARG(g != nullptr && (grad_dtype == SKYEMB_F32 ? aligned16(g) : (((uintptr_t)g) & 7) == 0),
                  "skyemb_grad_probe: null or unaligned gradient range");
    SKY_CHECK_ARG(state != nullptr && (((uintptr_t)state) & 3) == 0, "skyemb_grad_probe: null or unaligned state");
    int64_t blocks = ceil_div64(n / 4, 256);
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)blocks), block(256);
    if (grad_dtype == SKYEMB_F32) hipLaunchKernelGGL(grad_probe_kernel<SKYEMB_F32>, grid, block, 0, st, g, n / 4, state);
    else if (grad_dtype == SKYEMB_F16) hipLaunchKernelGGL(grad_probe_kernel<SKYEMB_F16>, grid, block, 0, st, g, n / 4, state);
    else hipLaunchKernelGGL(grad_probe_kernel<SKYEMB_BF16>, grid, block, 0, st, g, n / 4, state);
    SKY_LAUNCH_CHECK("skyemb_grad_probe");
    return 0;
}
