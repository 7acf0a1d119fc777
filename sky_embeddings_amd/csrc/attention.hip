// Multi-head attention core for tiny sequences (N = 5 / 17 / 65 / 66 tokens): one wavefront owns one
// (sample, head); q, k, v (and dO) are staged in LDS as fp32 rows (16-byte aligned pitch), every inner
// product / accumulation runs on float4 LDS reads, softmax statistics stay in fp32, the backward
// recomputes the probabilities.  0.3 % of the model FLOPs: built for latency, not for MFMA.
//
// qkv layout is the reference's: [B, N, 3, H, hd]  (timm Attention: qkv(x).reshape(B,N,3,H,hd)).
//
// Also the attention core's host side, at the end of the file: one driver behind skyemb_mha_fwd and skyemb_mha_bwd, which launches
// what sky_mha_plan (attention_plan.h) says -- these kernels, or the MFMA ones of attention_mfma.hip.
#include "attention_plan.h"
#include "common.h"
#include <stdlib.h>

namespace {

__device__ __forceinline__ float dot4(const float4 a, const float4 b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

// stage one [N, hd] head (rows row_stride elements apart) as fp32 rows of `pitch` floats; 8 elements per lane-step
template <typename T>
__device__ __forceinline__ void load_head(const T *__restrict__ src, int64_t row_stride, float *dst, int N, int hd,
                                          int pitch, float scale, int lane) {
    const int v4 = hd >> 2;
    for (int e = lane; e < N * v4; e += 64) {
        const int n = e / v4, d = (e - n * v4) << 2;
        const float4 x = load4<T>(src + (int64_t)n * row_stride + d);
        *(float4 *)&dst[n * pitch + d] = make_float4(x.x * scale, x.y * scale, x.z * scale, x.w * scale);
    }
}

// P[N][NP] = softmax_j(qs_i . k_j)
__device__ __forceinline__ void scores_softmax(const float *qs, const float *k, float *P, int N, int NP, int hd, int pitch,
                                               int lane) {
    for (int e = lane; e < N * N; e += 64) {
        const int i = e / N, j = e - i * N;
        float a0 = 0.f, a1 = 0.f;
        for (int d = 0; d < hd; d += 8) {
            a0 = dot4(*(const float4 *)&qs[i * pitch + d], *(const float4 *)&k[j * pitch + d], a0);
            a1 = dot4(*(const float4 *)&qs[i * pitch + d + 4], *(const float4 *)&k[j * pitch + d + 4], a1);
        }
        P[i * NP + j] = a0 + a1;
    }
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < N; i += 64) {
        float mx = -INFINITY;
        for (int j = 0; j < N; ++j) mx = fmaxf(mx, P[i * NP + j]);
        float sum = 0.f;
        for (int j = 0; j < N; ++j) {
            const float ev = __expf(P[i * NP + j] - mx);
            P[i * NP + j] = ev;
            sum += ev;
        }
        const float inv = 1.0f / sum;
        for (int j = 0; j < N; ++j) P[i * NP + j] *= inv;
    }
    __builtin_amdgcn_wave_barrier();
}

template <typename T>
__global__ void mha_fwd_kernel(const T *__restrict__ qkv, T *__restrict__ out, int B, int N, int H, int hd, int waves,
                               int per_wave_floats) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head_id = blockIdx.x * waves + wave;
    if (head_id >= B * H) return;
    const int b = head_id / H, h = head_id - b * H;
    const int pitch = hd + 4, D = H * hd, NP = N + 1;
    float *q = lds + (size_t)wave * per_wave_floats, *k = q + N * pitch, *v = k + N * pitch, *P = v + N * pitch;
    const T *base = qkv + (int64_t)b * N * 3 * D + h * hd;
    load_head<T>(base, 3 * D, q, N, hd, pitch, rsqrtf((float)hd), lane);
    load_head<T>(base + D, 3 * D, k, N, hd, pitch, 1.0f, lane);
    load_head<T>(base + 2 * D, 3 * D, v, N, hd, pitch, 1.0f, lane);
    __builtin_amdgcn_wave_barrier();
    scores_softmax(q, k, P, N, NP, hd, pitch, lane);
    const int v4 = hd >> 2;
    for (int e = lane; e < N * v4; e += 64) {
        const int i = e / v4, d = (e - i * v4) << 2;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < N; ++j) {
            const float p = P[i * NP + j];
            const float4 x = *(const float4 *)&v[j * pitch + d];
            acc.x = fmaf(p, x.x, acc.x); acc.y = fmaf(p, x.y, acc.y); acc.z = fmaf(p, x.z, acc.z); acc.w = fmaf(p, x.w, acc.w);
        }
        store4<T>(out + ((int64_t)b * N + i) * D + h * hd + d, acc.x, acc.y, acc.z, acc.w);
    }
}

template <typename T>
__global__ void mha_bwd_kernel(const T *__restrict__ qkv, const T *__restrict__ dout, T *__restrict__ dqkv, int B,
                               int N, int H, int hd, int waves, int per_wave_floats) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head_id = blockIdx.x * waves + wave;
    if (head_id >= B * H) return;
    const int b = head_id / H, h = head_id - b * H;
    const int pitch = hd + 4, D = H * hd, NP = N + 1;
    const float scale = rsqrtf((float)hd);
    float *q = lds + (size_t)wave * per_wave_floats, *k = q + N * pitch, *v = k + N * pitch, *dO = v + N * pitch;
    float *P = dO + N * pitch, *dS = P + N * NP;
    const T *base = qkv + (int64_t)b * N * 3 * D + h * hd;
    load_head<T>(base, 3 * D, q, N, hd, pitch, scale, lane);
    load_head<T>(base + D, 3 * D, k, N, hd, pitch, 1.0f, lane);
    load_head<T>(base + 2 * D, 3 * D, v, N, hd, pitch, 1.0f, lane);
    load_head<T>(dout + (int64_t)b * N * D + h * hd, D, dO, N, hd, pitch, 1.0f, lane);
    __builtin_amdgcn_wave_barrier();
    scores_softmax(q, k, P, N, NP, hd, pitch, lane);
    // dP = dO v^T
    for (int e = lane; e < N * N; e += 64) {
        const int i = e / N, j = e - i * N;
        float a0 = 0.f, a1 = 0.f;
        for (int d = 0; d < hd; d += 8) {
            a0 = dot4(*(const float4 *)&dO[i * pitch + d], *(const float4 *)&v[j * pitch + d], a0);
            a1 = dot4(*(const float4 *)&dO[i * pitch + d + 4], *(const float4 *)&v[j * pitch + d + 4], a1);
        }
        dS[i * NP + j] = a0 + a1;
    }
    __builtin_amdgcn_wave_barrier();
    // dS = P * (dP - rowsum(P * dP))
    for (int i = lane; i < N; i += 64) {
        float dot = 0.f;
        for (int j = 0; j < N; ++j) dot = fmaf(P[i * NP + j], dS[i * NP + j], dot);
        for (int j = 0; j < N; ++j) dS[i * NP + j] = P[i * NP + j] * (dS[i * NP + j] - dot);
    }
    __builtin_amdgcn_wave_barrier();
    T *dbase = dqkv + (int64_t)b * N * 3 * D + h * hd;
    const int v4 = hd >> 2;
    for (int e = lane; e < N * v4; e += 64) {
        const int n = e / v4, d = (e - n * v4) << 2;
        float4 aq = make_float4(0.f, 0.f, 0.f, 0.f), ak = aq, av = aq;
        for (int j = 0; j < N; ++j) {
            const float s_nj = dS[n * NP + j], s_jn = dS[j * NP + n], p_jn = P[j * NP + n];
            const float4 kj = *(const float4 *)&k[j * pitch + d], qj = *(const float4 *)&q[j * pitch + d];
            const float4 oj = *(const float4 *)&dO[j * pitch + d];
            aq.x = fmaf(s_nj, kj.x, aq.x); aq.y = fmaf(s_nj, kj.y, aq.y); aq.z = fmaf(s_nj, kj.z, aq.z); aq.w = fmaf(s_nj, kj.w, aq.w);
            ak.x = fmaf(s_jn, qj.x, ak.x); ak.y = fmaf(s_jn, qj.y, ak.y); ak.z = fmaf(s_jn, qj.z, ak.z); ak.w = fmaf(s_jn, qj.w, ak.w);
            av.x = fmaf(p_jn, oj.x, av.x); av.y = fmaf(p_jn, oj.y, av.y); av.z = fmaf(p_jn, oj.z, av.z); av.w = fmaf(p_jn, oj.w, av.w);
        }
        const int64_t o = (int64_t)n * 3 * D + d;
        store4<T>(dbase + o, aq.x * scale, aq.y * scale, aq.z * scale, aq.w * scale);   // dq = scale * dS k
        store4<T>(dbase + o + D, ak.x, ak.y, ak.z, ak.w);                                // dk = dS^T (scale q)
        store4<T>(dbase + o + 2 * D, av.x, av.y, av.z, av.w);                            // dv = P^T dO
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Streaming fallback for the shapes whose whole head does not fit the LDS plan of attention_plan.h (long sequences in the fp32 parity
// mode, head dims other than the MFMA kernels' 32 / 64 -- the 512-wide single decoder head of maesimple): fp32 arithmetic
// for every dtype, any N <= SKYEMB_MHA_MAX_N, any hd % 8 == 0 up to SH_MAXHD.  Built for correctness, not speed.
//   forward : one wave per query row; keys in chunks of 64 (lane j scores key j), online softmax with the running max and
//             sum in fp32, the output row rescaled when the max grows.
//   backward: one workgroup per (sample, head), the three phases of the long MFMA kernel (attention_mfma.hip):
//             A+C) per query row: a walk over the keys for lse_i and D_i = rowsum(P dP), then a second walk for dQ;
//             B)   per key row: a walk over the queries for dK and dV, the statistics of every query out of LDS.
//             Fixed summation order: deterministic.  LDS: 2 N floats of statistics + two [hd] rows and two [64] chunks
//             per wave (49 KB at N = 4098, hd = 512).
// ---------------------------------------------------------------------------------------------------------------
constexpr int SH_MAXHD = MHA_STREAM_MAX_HD, SH_C = SH_MAXHD / 64;

template <typename T>
__device__ __forceinline__ float dot_row(const float *lds_row, const T *g_row, int hd) {
    float a0 = 0.f, a1 = 0.f;
    for (int d = 0; d < hd; d += 8) {
        a0 = dot4(*(const float4 *)&lds_row[d], load4<T>(g_row + d), a0);
        a1 = dot4(*(const float4 *)&lds_row[d + 4], load4<T>(g_row + d + 4), a1);
    }
    return a0 + a1;
}
template <typename T>
__device__ __forceinline__ void load_row(float *dst, const T *src, int hd, float scale, int lane) {
    for (int d = 4 * lane; d < hd; d += 256) {
        const float4 x = load4<T>(src + d);
        *(float4 *)&dst[d] = make_float4(x.x * scale, x.y * scale, x.z * scale, x.w * scale);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void mha_fwd_stream_kernel(const T *__restrict__ qkv, T *__restrict__ out, int B, int N,
                                                             int H, int hd) {
    __shared__ __attribute__((aligned(16))) float sq[4][SH_MAXHD];
    __shared__ float sp[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.y * 4 + wave;
    if (i >= N) return;
    const int b = blockIdx.x / H, h = blockIdx.x - b * H, D = H * hd;
    const int64_t rs = 3 * (int64_t)D;
    const T *qb = qkv + (int64_t)b * N * rs + h * hd, *kb = qb + D, *vb = qb + 2 * D;
    load_row<T>(sq[wave], qb + (int64_t)i * rs, hd, rsqrtf((float)hd), lane);
    __builtin_amdgcn_wave_barrier();
    float o[SH_C];
#pragma unroll
    for (int c = 0; c < SH_C; ++c) o[c] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int j0 = 0; j0 < N; j0 += 64) {
        const int j = j0 + lane;
        const float s = j < N ? dot_row<T>(sq[wave], kb + (int64_t)j * rs, hd) : -INFINITY;
        const float mn = fmaxf(m, wave_max(s)), alpha = __expf(m - mn);
        const float p = j < N ? __expf(s - mn) : 0.f;
        l = l * alpha + wave_sum(p);
        m = mn;
        sp[wave][lane] = p;
        __builtin_amdgcn_wave_barrier();
        const int nj = N - j0 < 64 ? N - j0 : 64;
#pragma unroll
        for (int c = 0; c < SH_C; ++c) o[c] *= alpha;
        for (int jj = 0; jj < nj; ++jj) {
            const float pj = sp[wave][jj];
            const T *vr = vb + (int64_t)(j0 + jj) * rs;
#pragma unroll
            for (int c = 0; c < SH_C; ++c)
                if (lane + 64 * c < hd) o[c] = fmaf(pj, to_f32<T>(vr[lane + 64 * c]), o[c]);
        }
        __builtin_amdgcn_wave_barrier();
    }
    const float inv = 1.0f / l;
    T *orow = out + ((int64_t)b * N + i) * D + h * hd;
#pragma unroll
    for (int c = 0; c < SH_C; ++c)
        if (lane + 64 * c < hd) orow[lane + 64 * c] = from_f32<T>(o[c] * inv);
}

template <typename T>
__global__ __launch_bounds__(256) void mha_bwd_stream_kernel(const T *__restrict__ qkv, const T *__restrict__ dout,
                                                             T *__restrict__ dqkv, int B, int N, int H, int hd) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *ra = lds + (size_t)threadIdx.x / 64 * 2 * SH_MAXHD, *rb = ra + SH_MAXHD;          // this wave's two rows
    float *sa = lds + 8 * SH_MAXHD + (size_t)threadIdx.x / 64 * 128, *sb = sa + 64;           // this wave's two chunks
    float *lse = lds + 8 * SH_MAXHD + 4 * 128, *dsum = lse + N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / H, h = blockIdx.x - b * H, D = H * hd;
    const int64_t rs = 3 * (int64_t)D;
    const float scale = rsqrtf((float)hd);
    const T *qb = qkv + (int64_t)b * N * rs + h * hd, *kb = qb + D, *vb = qb + 2 * D;
    const T *ob = dout + (int64_t)b * N * D + h * hd;
    T *dqb = dqkv + (int64_t)b * N * rs + h * hd;

    // ---- phases A and C: one query row per wave
    for (int i = wave; i < N; i += 4) {
        load_row<T>(ra, qb + (int64_t)i * rs, hd, scale, lane);
        load_row<T>(rb, ob + (int64_t)i * D, hd, 1.0f, lane);
        __builtin_amdgcn_wave_barrier();
        float m = -INFINITY, l = 0.f, dacc = 0.f;
        for (int j0 = 0; j0 < N; j0 += 64) {
            const int j = j0 + lane;
            const float s = j < N ? dot_row<T>(ra, kb + (int64_t)j * rs, hd) : -INFINITY;
            const float dp = j < N ? dot_row<T>(rb, vb + (int64_t)j * rs, hd) : 0.f;
            const float mn = fmaxf(m, wave_max(s)), alpha = __expf(m - mn);
            const float p = j < N ? __expf(s - mn) : 0.f;
            l = l * alpha + wave_sum(p);
            dacc = dacc * alpha + wave_sum(p * dp);
            m = mn;
        }
        const float lse_i = m + logf(l), d_i = dacc / l;
        if (lane == 0) {
            lse[i] = lse_i;
            dsum[i] = d_i;
        }
        float a[SH_C];
#pragma unroll
        for (int c = 0; c < SH_C; ++c) a[c] = 0.f;
        for (int j0 = 0; j0 < N; j0 += 64) {
            const int j = j0 + lane;
            float ds = 0.f;
            if (j < N) {
                const float s = dot_row<T>(ra, kb + (int64_t)j * rs, hd), dp = dot_row<T>(rb, vb + (int64_t)j * rs, hd);
                ds = __expf(s - lse_i) * (dp - d_i);
            }
            sa[lane] = ds;
            __builtin_amdgcn_wave_barrier();
            const int nj = N - j0 < 64 ? N - j0 : 64;
            for (int jj = 0; jj < nj; ++jj) {
                const float dsj = sa[jj];
                const T *kr = kb + (int64_t)(j0 + jj) * rs;
#pragma unroll
                for (int c = 0; c < SH_C; ++c)
                    if (lane + 64 * c < hd) a[c] = fmaf(dsj, to_f32<T>(kr[lane + 64 * c]), a[c]);
            }
            __builtin_amdgcn_wave_barrier();
        }
        T *dq = dqb + (int64_t)i * rs;
#pragma unroll
        for (int c = 0; c < SH_C; ++c)
            if (lane + 64 * c < hd) dq[lane + 64 * c] = from_f32<T>(a[c] * scale);          // dq = scale dS k
    }
    __syncthreads();
    // ---- phase B: one key row per wave
    for (int j = wave; j < N; j += 4) {
        load_row<T>(ra, kb + (int64_t)j * rs, hd, 1.0f, lane);
        load_row<T>(rb, vb + (int64_t)j * rs, hd, 1.0f, lane);
        __builtin_amdgcn_wave_barrier();
        float ak[SH_C], av[SH_C];
#pragma unroll
        for (int c = 0; c < SH_C; ++c) ak[c] = av[c] = 0.f;
        for (int i0 = 0; i0 < N; i0 += 64) {
            const int i = i0 + lane;
            float p = 0.f, ds = 0.f;
            if (i < N) {
                const float s = dot_row<T>(ra, qb + (int64_t)i * rs, hd) * scale, dp = dot_row<T>(rb, ob + (int64_t)i * D, hd);
                p = __expf(s - lse[i]);
                ds = p * (dp - dsum[i]);
            }
            sa[lane] = p;
            sb[lane] = ds;
            __builtin_amdgcn_wave_barrier();
            const int ni = N - i0 < 64 ? N - i0 : 64;
            for (int ii = 0; ii < ni; ++ii) {
                const float pi = sa[ii], dsi = sb[ii];
                const T *qr = qb + (int64_t)(i0 + ii) * rs, *orow = ob + (int64_t)(i0 + ii) * D;
#pragma unroll
                for (int c = 0; c < SH_C; ++c)
                    if (lane + 64 * c < hd) {
                        ak[c] = fmaf(dsi, to_f32<T>(qr[lane + 64 * c]), ak[c]);
                        av[c] = fmaf(pi, to_f32<T>(orow[lane + 64 * c]), av[c]);
                    }
            }
            __builtin_amdgcn_wave_barrier();
        }
        T *dk = dqb + (int64_t)j * rs + D, *dv = dk + D;
#pragma unroll
        for (int c = 0; c < SH_C; ++c)
            if (lane + 64 * c < hd) {
                dk[lane + 64 * c] = from_f32<T>(ak[c] * scale);                            // dk = dS^T (scale q)
                dv[lane + 64 * c] = from_f32<T>(av[c]);                                    // dv = P^T dO
            }
    }
}

// what sky_mha_plan refuses, in the entry points' words
int plan_or_refuse(bool bwd, int dtype, int B, int N, int H, int hd, int switches, skyemb_mha_plan_t *p) {
    const char *who = bwd ? "skyemb_mha_bwd" : "skyemb_mha_fwd";
    switch (sky_mha_plan(bwd, dtype, B, N, H, hd, switches, p)) {
    case MHA_OK: return 0;
    case MHA_BAD_SHAPE: skyemb_set_error("%s: bad shape (head dim must be a multiple of 8)", who); return 1;
    case MHA_TOO_LONG: skyemb_set_error("%s: N = %d tokens, more than the supported %d", who, N, SKYEMB_MHA_MAX_N); return 1;
    default: skyemb_set_error("%s: head dim %d with N = %d tokens: at most %d", who, hd, N, SH_MAXHD); return 1;
    }
}

// the two diagnostic switches of INTEGRATION.md as SKYEMB_MHA_SW_* bits, read once per process
int env_switches() {
    static const int sw = []() {
        const char *off = getenv("SKYEMB_MHA_MFMA"), *wpb = getenv("SKYEMB_MHA_WPB");
        const int w = wpb ? atoi(wpb) : 0;
        return (off && off[0] == '0' ? SKYEMB_MHA_SW_NO_MFMA : 0) | (w == 1 ? SKYEMB_MHA_SW_WPB1 : w ? SKYEMB_MHA_SW_WPB4 : 0);
    }();
    return sw;
}

// the lds and stream families for element type T (`out` is dqkv in backward)
template <typename T>
int launch_fp32(const skyemb_mha_plan_t &p, bool bwd, const T *qkv, const T *dout, T *out, int B, int N, int H, int hd,
                hipStream_t st, const char *who) {
    const dim3 grid(p.grid_x, p.grid_y), block(p.block);
    if (p.family == SKYEMB_MHA_STREAM) {
        if (!bwd) hipLaunchKernelGGL(mha_fwd_stream_kernel<T>, grid, block, p.lds_bytes, st, qkv, out, B, N, H, hd);
        else hipLaunchKernelGGL(mha_bwd_stream_kernel<T>, grid, block, p.lds_bytes, st, qkv, dout, out, B, N, H, hd);
        return 0;
    }
    if (p.lds_limit)
        if (const int rc = sky_set_lds_limit(bwd ? (const void *)mha_bwd_kernel<T> : (const void *)mha_fwd_kernel<T>, (int)p.lds_limit, who))
            return rc;
    if (!bwd) hipLaunchKernelGGL(mha_fwd_kernel<T>, grid, block, p.lds_bytes, st, qkv, out, B, N, H, hd, p.waves, p.per_wave_floats);
    else hipLaunchKernelGGL(mha_bwd_kernel<T>, grid, block, p.lds_bytes, st, qkv, dout, out, B, N, H, hd, p.waves, p.per_wave_floats);
    return 0;
}

}  // namespace

// attention_mfma.hip: launches a plan of one of the SKYEMB_MHA_MFMA_* families (dtype bf16 / fp16); 0, or sky_set_lds_limit's 2
int skyemb_mha_mfma_launch(const skyemb_mha_plan_t &p, bool bwd, const void *qkv, const void *dout, void *out, int dtype, int B, int N,
                           int H, hipStream_t st, const char *who);

// both directions: validate, plan, raise the LDS limit where the plan asks, launch, check
static int mha_run(bool bwd, const void *qkv, const void *dout, void *out, int dtype, int B, int N, int H, int hd, void *stream) {
    const char *who = bwd ? "skyemb_mha_bwd" : "skyemb_mha_fwd";
    (void)hipGetLastError();           // as SKY_CHECK_ARG: a stale sticky error is not this call's
    skyemb_mha_plan_t p;
    if (const int rc = plan_or_refuse(bwd, dtype, B, N, H, hd, env_switches(), &p)) return rc;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (p.family >= SKYEMB_MHA_MFMA_PACKED) rc = skyemb_mha_mfma_launch(p, bwd, qkv, dout, out, dtype, B, N, H, st, who);
    else if (dtype == SKYEMB_BF16) rc = launch_fp32(p, bwd, (const bf16_t *)qkv, (const bf16_t *)dout, (bf16_t *)out, B, N, H, hd, st, who);
    else if (dtype == SKYEMB_F16) rc = launch_fp32(p, bwd, (const f16_t *)qkv, (const f16_t *)dout, (f16_t *)out, B, N, H, hd, st, who);
    else rc = launch_fp32(p, bwd, (const float *)qkv, (const float *)dout, (float *)out, B, N, H, hd, st, who);
    if (rc) return rc;
    SKY_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int skyemb_mha_fwd(const void *qkv, void *out, int dtype, int B, int N, int H, int hd, void *stream) {
    return mha_run(false, qkv, nullptr, out, dtype, B, N, H, hd, stream);
}

extern "C" int skyemb_mha_bwd(const void *qkv, const void *dout, void *dqkv, int dtype, int B, int N, int H, int hd,
                              void *stream) {
    return mha_run(true, qkv, dout, dqkv, dtype, B, N, H, hd, stream);
}

extern "C" int skyemb_mha_plan(int bwd, int dtype, int B, int N, int H, int hd, int switches, skyemb_mha_plan_t *out) {
    if (!out) {
        skyemb_set_error("skyemb_mha_plan: out is NULL");
        return 1;
    }
    return plan_or_refuse(bwd != 0, dtype, B, N, H, hd, switches < 0 ? env_switches() : switches, out);
}
