// Half-precision resident banks (bf16 / fp16 rows): the weighted norms of 16-bit rows and the standardise-and-round step that
// builds such a bank batch by batch.  A 16-bit bank is the fp32 bank its elements widen to, so both kernels restate their fp32
// namesakes of topk.hip operation for operation: the norms on exactly widened values, the standardised value rounded once.
#include "common.h"

namespace {

// out = round_to_nearest_even_16( (x - mu) / (sigma + 1e-8) ): standardise_kernel's three fp32 operations, then ONE conversion
// (v_cvt_f16_f32: overflow -> +-inf, subnormals produced; v_cvt_pk_bf16_f32; NaN stays NaN).
template <typename T>
__global__ __launch_bounds__(256) void standardise_lp_kernel(const float *__restrict__ x, const float *__restrict__ mu,
                                                             const float *__restrict__ sigma, T *__restrict__ out, int64_t total4,
                                                             int D4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int d = (int)(i % D4) * 4;
        const float4 v = *(const float4 *)(x + 4 * i);
        const float4 m = *(const float4 *)(mu + d), s = *(const float4 *)(sigma + d);
        store4<T>(out + 4 * i, __fdiv_rn(__fsub_rn(v.x, m.x), __fadd_rn(s.x, 1e-8f)),
                  __fdiv_rn(__fsub_rn(v.y, m.y), __fadd_rn(s.y, 1e-8f)), __fdiv_rn(__fsub_rn(v.z, m.z), __fadd_rn(s.z, 1e-8f)),
                  __fdiv_rn(__fsub_rn(v.w, m.w), __fadd_rn(s.w, 1e-8f)));
    }
}

// norms[n] = sqrt( chain_d fma(w[d] * x[n][d], x[n][d], acc) ) on the widened row: wnorm_kernel's chain (topk.hip).  Block = 256
// rows; 32-wide d chunks are staged through LDS as floats (one 8-byte load of four elements per thread and step), each thread
// walks its own row in order.
template <typename T>
__global__ __launch_bounds__(256) void wnorm_lp_kernel(const T *__restrict__ x, const float *__restrict__ w, float *__restrict__ norms,
                                                       int64_t N, int D) {
    __shared__ float tile[256][33];
    const int tid = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * 256;
    float acc = 0.f;
    for (int d0 = 0; d0 < D; d0 += 32) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int v = tid + i * 256, r = v >> 3, c = (v & 7) * 4;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n0 + r < N && d0 + c < D) val = load4<T>(x + (n0 + r) * D + d0 + c);
            tile[r][c] = val.x; tile[r][c + 1] = val.y; tile[r][c + 2] = val.z; tile[r][c + 3] = val.w;
        }
        __syncthreads();
        const int dn = (D - d0) < 32 ? (D - d0) : 32;
        for (int dd = 0; dd < dn; ++dd) {
            const float xv = tile[tid][dd];
            const float xw = w ? __fmul_rn(w[d0 + dd], xv) : xv;
            acc = fmaf(xw, xv, acc);
        }
    }
    if (n0 + tid < N) norms[n0 + tid] = __fsqrt_rn(acc);
}

}  // namespace

#define LP_DTYPE_MSG "must be SKYEMB_BF16 (0) or SKYEMB_F16 (2), got %d"

extern "C" int skyemb_weighted_norms_lp(const void *x, int dtype, const float *w, float *norms, int64_t N, int D, void *stream) {
    SKY_CHECK_ARG(sky_is_lp(dtype), "skyemb_weighted_norms_lp: dtype " LP_DTYPE_MSG " (fp32 rows take skyemb_weighted_norms)", dtype);
    SKY_CHECK_ARG(x && norms, "skyemb_weighted_norms_lp: bad arguments (x and norms must not be NULL)");
    SKY_CHECK_ARG(N > 0 && D > 0 && D % 4 == 0, "skyemb_weighted_norms_lp: bad shape (N = %lld, D = %d: N > 0, D %% 4 == 0)",
                  (long long)N, D);
    SKY_CHECK_ARG((((uintptr_t)x) & 7) == 0, "skyemb_weighted_norms_lp: x must be 8-byte aligned");
    const dim3 grid((unsigned)ceil_div64(N, 256));
    if (dtype == SKYEMB_BF16)
        hipLaunchKernelGGL(wnorm_lp_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t *)x, w, norms, N, D);
    else
        hipLaunchKernelGGL(wnorm_lp_kernel<f16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const f16_t *)x, w, norms, N, D);
    SKY_LAUNCH_CHECK("skyemb_weighted_norms_lp");
    return 0;
}

extern "C" int skyemb_standardise_lp(const float *x, const float *mu, const float *sigma, void *out, int out_dtype, int64_t N, int D,
                                     void *stream) {
    SKY_CHECK_ARG(sky_is_lp(out_dtype), "skyemb_standardise_lp: out_dtype " LP_DTYPE_MSG " (fp32 output: skyemb_standardise)", out_dtype);
    SKY_CHECK_ARG(x && mu && sigma && out, "skyemb_standardise_lp: bad arguments (x, mu, sigma and out must not be NULL)");
    SKY_CHECK_ARG(N > 0 && D > 0 && D % 4 == 0, "skyemb_standardise_lp: bad shape (N = %lld, D = %d: N > 0, D %% 4 == 0)", (long long)N,
                  D);
    SKY_CHECK_ARG(aligned16(x) && aligned16(mu) && aligned16(sigma) && (((uintptr_t)out) & 7) == 0,
                  "skyemb_standardise_lp: x, mu and sigma must be 16-byte aligned, out 8-byte aligned");
    const int64_t total4 = N * D / 4;
    int64_t blocks = ceil_div64(total4, 256);
    if (blocks > 256 * 16) blocks = 256 * 16;
    if (out_dtype == SKYEMB_BF16)
        hipLaunchKernelGGL(standardise_lp_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, mu, sigma,
                           (bf16_t *)out, total4, D / 4);
    else
        hipLaunchKernelGGL(standardise_lp_kernel<f16_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, mu, sigma,
                           (f16_t *)out, total4, D / 4);
    SKY_LAUNCH_CHECK("skyemb_standardise_lp");
    return 0;
}
