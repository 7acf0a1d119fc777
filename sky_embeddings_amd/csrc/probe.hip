// Linear-probe validation fits on the device (sky_embeddings_amd/probe.py; the reference fits scikit-learn estimators on the host,
// utils/pretrain_fns.py:52-159): column statistics and standard scaling, the softmax-regression objective and gradient that
// L-BFGS evaluates, the fp64 Gram of the centred features and the elastic net's cyclic coordinate descent on that Gram.
//
// No atomics anywhere: every sum has ONE order, fixed by the shapes alone (SKYEMB_PROBE_CHUNKS row chunks added in chunk order,
// fixed-size trees inside a workgroup, one thread per output elsewhere), so results do not depend on launch geometry or on the
// row stride of the input.  Built with -ffp-contract=off (csrc/Makefile): a fused multiply-add appears only where fma / fmaf is
// written, which is what tests/probe_reference.py restates.
#include "common.h"

#include <math.h>

namespace {

constexpr int CH = SKYEMB_PROBE_CHUNKS;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// ------------------------------------------------------------------------------------------------ column statistics
// grid (ceil(F / 256), CH): thread = one column of one row chunk; chunk c owns rows [c * rpc, (c + 1) * rpc), rpc = ceil(n / CH).
// SQ = false: part = sum x;  SQ = true: part = sum (x - centre)^2.  fp64 throughout.
template <bool SQ>
__global__ __launch_bounds__(256) void probe_colpart_kernel(const float *__restrict__ X, int64_t ldx, int n, int F,
                                                            const double *__restrict__ centre, double *__restrict__ part) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int rpc = (n + CH - 1) / CH;
    const int r0 = blockIdx.y * rpc, r1 = min(n, r0 + rpc);
    const double c = SQ ? centre[f] : 0.0;
    double acc = 0.0;
#pragma unroll 4
    for (int i = r0; i < r1; ++i) {
        const double v = (double)X[(int64_t)i * ldx + f];
        if (SQ) {
            const double d = v - c;
            acc = acc + d * d;
        } else {
            acc = acc + v;
        }
    }
    part[(int64_t)blockIdx.y * F + f] = acc;
}

// out[f] = (sum over the chunks, in chunk order) / n; scale[f] = sqrt(out) or exactly 1 where out == 0 (scale != NULL: variance pass)
__global__ __launch_bounds__(256) void probe_colfinish_kernel(const double *__restrict__ part, int n, int F, double *__restrict__ out,
                                                              double *__restrict__ scale) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    double s = 0.0;
    for (int c = 0; c < CH; ++c) s = s + part[(int64_t)c * F + f];
    s = s / (double)n;
    out[f] = s;
    if (scale) scale[f] = s == 0.0 ? 1.0 : sqrt(s);
}

__global__ __launch_bounds__(256) void probe_scale_kernel(const float *__restrict__ X, int64_t ldx, int n, int F,
                                                          const double *__restrict__ mean, const double *__restrict__ scale,
                                                          float *__restrict__ out, int64_t ldo) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const double mu = mean[f], sc = scale ? scale[f] : 1.0;
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        const double d = (double)X[(int64_t)i * ldx + f] - mu;
        out[(int64_t)i * ldo + f] = (float)(scale ? d / sc : d);
    }
}

// ------------------------------------------------------------------------------------------ softmax objective, first pass
// Four waves per workgroup, SM_RW rows per wave; W passes through LDS in tiles of SM_FT columns (KP * SM_FT * 4 <= 64 KiB).  A
// row's K logits are summed by ONE wave: lane l takes the columns l, l + 64, ... in ascending order (fmaf), then the xor butterfly.
constexpr int SM_RW = 4, SM_FT = 1024;

template <int KP>
__global__ __launch_bounds__(256) void probe_softmax_fwd_kernel(const float *__restrict__ X, int64_t ldx, const int32_t *__restrict__ y,
                                                                int m, int F, int K, const float *__restrict__ W,
                                                                const float *__restrict__ b, float *__restrict__ R,
                                                                float *__restrict__ rowloss) {
    extern __shared__ float sW[];   // [KP][SM_FT]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row0 = (blockIdx.x * 4 + wave) * SM_RW;
    float acc[SM_RW][KP];
#pragma unroll
    for (int r = 0; r < SM_RW; ++r)
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[r][k] = 0.f;
    const float *xr[SM_RW];
#pragma unroll
    for (int r = 0; r < SM_RW; ++r) xr[r] = X + (int64_t)min(row0 + r, m - 1) * ldx;   // rows past m: read row m - 1, never stored
    for (int f0 = 0; f0 < F; f0 += SM_FT) {
        __syncthreads();
        for (int e = tid; e < KP * SM_FT; e += 256) {
            const int k = e / SM_FT, ff = e % SM_FT;
            sW[e] = (k < K && f0 + ff < F) ? W[(int64_t)k * F + f0 + ff] : 0.f;
        }
        __syncthreads();
        const int fend = min(SM_FT, F - f0);
#pragma unroll 2
        for (int ff = lane; ff < fend; ff += 64) {
            float x[SM_RW];
#pragma unroll
            for (int r = 0; r < SM_RW; ++r) x[r] = xr[r][f0 + ff];
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const float w = sW[k * SM_FT + ff];
#pragma unroll
                for (int r = 0; r < SM_RW; ++r) acc[r][k] = fmaf(x[r], w, acc[r][k]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < SM_RW; ++r)
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[r][k] = wave_sum(acc[r][k]);
    const float mf = (float)m;
#pragma unroll
    for (int r = 0; r < SM_RW; ++r) {
        const int i = row0 + r;
        if (i >= m) continue;                       // (wave-uniform)
        const int yi = y[i];
        float z[KP], mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            z[k] = k < K ? acc[r][k] + b[k] : -INFINITY;
            mx = fmaxf(mx, z[k]);
        }
        float s = 0.f, zy = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            z[k] = k < K ? expf(z[k] - mx) : 0.f;   // z now holds the exponentials; the label's logit is kept as zy - mx below
            if (k < K) s = s + z[k];
        }
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k == yi) zy = acc[r][k] + b[k < K ? k : 0];
        if (lane == 0) {
            rowloss[i] = (logf(s) + mx) - zy;
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < K) R[(int64_t)i * K + k] = (z[k] / s - (k == yi ? 1.f : 0.f)) / mf;
        }
    }
}

// grid K + 2, 256 threads: block k < K: gb[k] = sum_i R[i, k]; block K: sum of the row losses; block K + 1: sum W^2.
// Thread t adds its elements t, t + 256, ... in ascending order in fp64, then a fixed 256-leaf tree.
__global__ __launch_bounds__(256) void probe_softmax_reduce_kernel(const float *__restrict__ R, const float *__restrict__ rowloss,
                                                                   const float *__restrict__ W, int m, int F, int K,
                                                                   float *__restrict__ gb, double *__restrict__ lossparts) {
    __shared__ double tree[256];
    const int tid = threadIdx.x, which = blockIdx.x;
    double acc = 0.0;
    if (which < K) {
        for (int i = tid; i < m; i += 256) acc = acc + (double)R[(int64_t)i * K + which];
    } else if (which == K) {
        for (int i = tid; i < m; i += 256) acc = acc + (double)rowloss[i];
    } else {
        const int64_t n = (int64_t)K * F;
        for (int64_t i = tid; i < n; i += 256) {
            const double w = (double)W[i];
            acc = acc + w * w;
        }
    }
    tree[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) tree[tid] = tree[tid] + tree[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        if (which < K) gb[which] = (float)tree[0];
        else lossparts[which - K] = tree[0];
    }
}

// ----------------------------------------------------------------------------------------- softmax objective, second pass
// grid (ceil(F / 64), CH), one wave: thread = one column of one row chunk, part[c][k][f] = sum over the chunk's rows (ascending,
// fmaf) of R[i, k] X[i, f].
template <int KP>
__global__ __launch_bounds__(64) void probe_softmax_wgrad_kernel(const float *__restrict__ X, int64_t ldx, int m, int F, int K,
                                                                 const float *__restrict__ R, float *__restrict__ part) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    const int rpc = (m + CH - 1) / CH;
    const int r0 = blockIdx.y * rpc, r1 = min(m, r0 + rpc);
    if (f >= F) return;
    float acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.f;
#pragma unroll 4
    for (int i = r0; i < r1; ++i) {
        const float x = X[(int64_t)i * ldx + f];
        const float *__restrict__ ri = R + (int64_t)i * K;
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < K) acc[k] = fmaf(ri[k], x, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < KP; ++k)
        if (k < K) part[((int64_t)blockIdx.y * K + k) * F + f] = acc[k];
}

// gW[k, f] = fp32(sum over the chunks in chunk order (fp64) + l2 W[k, f]);  loss = lossparts[0] / m + 0.5 l2 lossparts[1]
__global__ __launch_bounds__(256) void probe_softmax_finish_kernel(const float *__restrict__ part, const float *__restrict__ W, int m,
                                                                   int F, int K, double l2, const double *__restrict__ lossparts,
                                                                   float *__restrict__ gW, double *__restrict__ loss) {
    const int64_t n = (int64_t)K * F, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) *loss = lossparts[0] / (double)m + (0.5 * l2) * lossparts[1];
    if (e >= n) return;
    double s = 0.0;
    for (int c = 0; c < CH; ++c) s = s + (double)part[(int64_t)c * n + e];
    gW[e] = (float)(s + l2 * (double)W[e]);
}

// ------------------------------------------------------------------------------------------------------------ fp64 Gram
// G = Xc^T Xc on plain fp64 FMAs: a 64 x 64 tile per workgroup, 4 x 4 outputs per thread, rows staged through LDS 16 at a time
// (fp32, widened on the way to the FMA).  Every G[i, j] is ONE thread's fma chain over the rows in ascending order.  Only the
// tiles on and above the diagonal are computed; each value is stored to (i, j) and (j, i), so G is symmetric bit for bit.
__global__ __launch_bounds__(256) void probe_gram_kernel(const float *__restrict__ Xc, int64_t ldx, int m, int F, double *__restrict__ G) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    __shared__ __attribute__((aligned(16))) float sA[16][64];
    __shared__ __attribute__((aligned(16))) float sB[16][64];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int I0 = bi * 64, J0 = bj * 64;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;
    const int lr = tid >> 4, lc = (tid & 15) * 4;
    for (int r0 = 0; r0 < m; r0 += 16) {
        const int row = r0 + lr;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = lc + u;
            sA[lr][c] = (row < m && I0 + c < F) ? Xc[(int64_t)row * ldx + I0 + c] : 0.f;
            sB[lr][c] = (row < m && J0 + c < F) ? Xc[(int64_t)row * ldx + J0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const float4 a4 = *(const float4 *)&sA[rr][ti * 4];
            const float4 b4 = *(const float4 *)&sB[rr][tj * 4];
            const double a[4] = {(double)a4.x, (double)a4.y, (double)a4.z, (double)a4.w};
            const double c[4] = {(double)b4.x, (double)b4.y, (double)b4.z, (double)b4.w};
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[p][s] = fma(a[p], c[s], acc[p][s]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int gi = I0 + ti * 4 + p, gj = J0 + tj * 4 + s;
            if (gi < F && gj < F) {
                G[(int64_t)gi * F + gj] = acc[p][s];
                G[(int64_t)gj * F + gi] = acc[p][s];
            }
        }
}

// q[f] = sum_i Xc[i, f] yc[i] (one thread per column, rows ascending, fma); the last workgroup: ynorm2 = sum yc^2 (64-leaf tree)
__global__ __launch_bounds__(64) void probe_xty_kernel(const float *__restrict__ Xc, int64_t ldx, const float *__restrict__ yc, int m,
                                                       int F, double *__restrict__ q, double *__restrict__ ynorm2) {
    const int tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ double tree[64];
        double acc = 0.0;
        for (int i = tid; i < m; i += 64) {
            const double v = (double)yc[i];
            acc = fma(v, v, acc);
        }
        tree[tid] = acc;
        __syncthreads();
        for (int s = 32; s > 0; s >>= 1) {
            if (tid < s) tree[tid] = tree[tid] + tree[tid + s];
            __syncthreads();
        }
        if (tid == 0) *ynorm2 = tree[0];
        return;
    }
    const int f = blockIdx.x * 64 + tid;
    if (f >= F) return;
    double acc = 0.0;
#pragma unroll 8
    for (int i = 0; i < m; ++i) acc = fma((double)Xc[(int64_t)i * ldx + f], (double)yc[i], acc);
    q[f] = acc;
}

// ------------------------------------------------------------------------------- elastic net: coordinate descent on the Gram
// ONE persistent workgroup of 8 waves.  w, H = G w, q and diag(G) live in LDS as fp64 (32 F bytes), so a coordinate that stays
// where it is costs LDS reads only -- and 64 of them are examined at once: lane l of every wave evaluates coordinate j0 + l
// against the CURRENT H; the lowest lane whose coordinate moves is the next one cyclic order would move (everything before it was
// judged on the H it would have seen), it is applied -- all 512 threads add d * G[j, :] to their slice of H between two barriers
// -- and the group is re-examined from the lane behind it.  All waves take the same decisions from the same LDS words, so the
// barriers are uniform.
// Latency: the rows of the coordinates that were non-zero at the start of the sweep are the ones that move; their indices are listed
// once per sweep and each thread keeps its slice of the next CD_PD listed rows in registers, loaded CD_PD moves ahead.  A move
// outside the list (a coordinate entering the model) loads its row on the spot; a listed coordinate that did not move drops the ring
// (reloaded from the list: rare, and then only late in a fit).
constexpr int CD_NT = 512, CD_EPT = SKYEMB_PROBE_MAX_F / CD_NT, CD_PD = 4;
struct CdRow { double v[CD_EPT]; };

__device__ __forceinline__ CdRow cd_load_row(const double *__restrict__ G, int F, int j, int tid, bool on) {
    CdRow r;
#pragma unroll
    for (int s = 0; s < CD_EPT; ++s) {
        const int i = tid + s * CD_NT;
        r.v[s] = (on && i < F) ? G[(int64_t)j * F + i] : 0.0;
    }
    return r;
}

// sum / max over the workgroup: per-thread value -> wave butterfly -> one word per wave, added in wave order by every thread
template <bool MAX>
__device__ __forceinline__ double cd_block_reduce(double v, double *red, int tid) {
    v = MAX ? wave_max_f64(v) : wave_sum_f64(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int k = 1; k < CD_NT / 64; ++k) t = MAX ? fmax(t, red[k]) : t + red[k];
    return t;
}

__global__ __launch_bounds__(CD_NT) void probe_enet_cd_kernel(const double *__restrict__ G, const double *__restrict__ q_g,
                                                              const double *__restrict__ ynorm2_g, int F, double a1, double b2,
                                                              int max_iter, double tol, double *__restrict__ w_out,
                                                              int32_t *__restrict__ status, double *__restrict__ gap_out) {
    extern __shared__ double cd_sm[];
    double *w = cd_sm, *H = cd_sm + F, *q = cd_sm + 2 * F, *dg = cd_sm + 3 * F, *red = cd_sm + 4 * F;
    int *list = (int *)(red + CD_NT / 64);
    __shared__ int s_nl;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < F; i += CD_NT) {
        w[i] = 0.0;
        H[i] = 0.0;
        q[i] = q_g[i];
        dg[i] = G[(int64_t)i * F + i];
    }
    __syncthreads();
    const double ynorm2 = *ynorm2_g, tolg = tol * ynorm2;
    double gap = tol + 1.0;
    int nl = 0, sweeps = 0, converged = 0;
    for (int it = 0; it < max_iter; ++it) {
        int k = 0;
        CdRow ring[CD_PD];
#pragma unroll
        for (int s = 0; s < CD_PD; ++s) ring[s] = cd_load_row(G, F, s < nl ? list[s] : 0, tid, s < nl);
        double dwmax = 0.0;
        for (int j0 = 0; j0 < F; j0 += 64) {
            int start = 0;
            while (start < 64) {
                const int j = j0 + lane;
                double wj = 0.0, wn = 0.0;
                bool ch = false;
                if (j < F && lane >= start) {
                    const double d = dg[j];
                    if (d != 0.0) {
                        wj = w[j];
                        const double t = (q[j] - H[j]) + wj * d;
                        const double at = fabs(t) - a1;
                        wn = at > 0.0 ? copysign(at, t) / (d + b2) : 0.0;
                        ch = wn != wj;
                    }
                }
                const unsigned long long moved = __ballot(ch);
                if (!moved) break;
                const int c = __builtin_ctzll(moved), jc = j0 + c;
                const double dlt = __shfl(wn, c, 64) - __shfl(wj, c, 64), wnew = __shfl(wn, c, 64);
                bool stale = false;
                while (k < nl && list[k] < jc) {
                    ++k;
                    stale = true;
                }
                if (stale) {
#pragma unroll
                    for (int s = 0; s < CD_PD; ++s) ring[s] = cd_load_row(G, F, k + s < nl ? list[k + s] : 0, tid, k + s < nl);
                }
                CdRow row;
                if (k < nl && list[k] == jc) {
                    row = ring[0];
#pragma unroll
                    for (int s = 0; s + 1 < CD_PD; ++s) ring[s] = ring[s + 1];
                    ring[CD_PD - 1] = cd_load_row(G, F, k + CD_PD < nl ? list[k + CD_PD] : 0, tid, k + CD_PD < nl);
                    ++k;
                } else {
                    row = cd_load_row(G, F, jc, tid, true);
                }
                __syncthreads();            // every wave has read H for this decision
                if (tid == 0) w[jc] = wnew;
#pragma unroll
                for (int s = 0; s < CD_EPT; ++s) {
                    const int i = tid + s * CD_NT;
                    if (i < F) H[i] = H[i] + dlt * row.v[s];
                }
                __syncthreads();
                dwmax = fmax(dwmax, fabs(dlt));
                start = c + 1;
            }
        }
        sweeps = it + 1;
        // end of the sweep: max|w|, the list of non-zero coordinates (wave 0, index order), and perhaps the gap
        double wm = 0.0;
        for (int i = tid; i < F; i += CD_NT) wm = fmax(wm, fabs(w[i]));
        const double wmax = cd_block_reduce<true>(wm, red, tid);
        if (tid < 64) {
            int n = 0;
            for (int b0 = 0; b0 < F; b0 += 64) {
                const int j = b0 + lane;
                const bool nz = j < F && w[j] != 0.0;
                const unsigned long long mk = __ballot(nz);
                if (nz) list[n + __popcll(mk & ((1ull << lane) - 1ull))] = j;
                n += __popcll(mk);
            }
            if (lane == 0) s_nl = n;
        }
        __syncthreads();
        nl = s_nl;
        if (wmax == 0.0 || dwmax / wmax < tol || it == max_iter - 1) {
            double qw = 0.0, wH = 0.0, ww = 0.0, l1 = 0.0, dn = 0.0;
            for (int i = tid; i < F; i += CD_NT) {
                const double wi = w[i], Hi = H[i], qi = q[i];
                qw = qw + wi * qi;
                wH = wH + wi * Hi;
                ww = ww + wi * wi;
                l1 = l1 + fabs(wi);
                dn = fmax(dn, fabs((qi - Hi) - b2 * wi));
            }
            qw = cd_block_reduce<false>(qw, red, tid);
            wH = cd_block_reduce<false>(wH, red, tid);
            ww = cd_block_reduce<false>(ww, red, tid);
            l1 = cd_block_reduce<false>(l1, red, tid);
            dn = cd_block_reduce<true>(dn, red, tid);
            const double R2 = (ynorm2 + wH) - 2.0 * qw;
            double cst;
            if (dn > a1) {
                cst = a1 / dn;
                gap = 0.5 * (R2 + R2 * (cst * cst));
            } else {
                cst = 1.0;
                gap = R2;
            }
            gap = gap + (((a1 * l1 - cst * ynorm2) + cst * qw) + (0.5 * b2) * (1.0 + cst * cst) * ww);
            if (gap < tolg) {
                converged = 1;
                break;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < F; i += CD_NT) w_out[i] = w[i];
    if (tid == 0) {
        status[0] = sweeps;
        status[1] = converged;
        *gap_out = gap;
    }
}

constexpr int CD_LDS_MAX = 4 * SKYEMB_PROBE_MAX_F * 8 + (CD_NT / 64) * 8 + SKYEMB_PROBE_MAX_F * 4;

bool probe_shape_ok(int m, int F) { return m > 0 && F > 0 && F <= SKYEMB_PROBE_MAX_F; }

}  // namespace

extern "C" int skyemb_probe_colstats(const float *X, int64_t ldx, int n, int F, double *mean, double *var, double *scale, double *ws,
                                     void *stream) {
    SKY_CHECK_ARG(n > 0 && F > 0 && ldx >= F, "skyemb_probe_colstats: bad shape n=%d F=%d ldx=%lld", n, F, (long long)ldx);
    SKY_CHECK_ARG(X && mean && var && scale && ws, "skyemb_probe_colstats: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((F + 255) / 256, CH), fin((F + 255) / 256), block(256);
    hipLaunchKernelGGL(probe_colpart_kernel<false>, grid, block, 0, st, X, ldx, n, F, (const double *)nullptr, ws);
    hipLaunchKernelGGL(probe_colfinish_kernel, fin, block, 0, st, (const double *)ws, n, F, mean, (double *)nullptr);
    hipLaunchKernelGGL(probe_colpart_kernel<true>, grid, block, 0, st, X, ldx, n, F, (const double *)mean, ws);
    hipLaunchKernelGGL(probe_colfinish_kernel, fin, block, 0, st, (const double *)ws, n, F, var, scale);
    SKY_LAUNCH_CHECK("skyemb_probe_colstats");
    return 0;
}

extern "C" int skyemb_probe_scale(const float *X, int64_t ldx, int n, int F, const double *mean, const double *scale, float *out,
                                  int64_t ldo, void *stream) {
    SKY_CHECK_ARG(n > 0 && F > 0 && ldx >= F && ldo >= F, "skyemb_probe_scale: bad shape n=%d F=%d ldx=%lld ldo=%lld", n, F,
                  (long long)ldx, (long long)ldo);
    SKY_CHECK_ARG(X && mean && out, "skyemb_probe_scale: null pointer");
    const dim3 grid((F + 255) / 256, n < 1024 ? n : 1024), block(256);
    hipLaunchKernelGGL(probe_scale_kernel, grid, block, 0, (hipStream_t)stream, X, ldx, n, F, mean, scale, out, ldo);
    SKY_LAUNCH_CHECK("skyemb_probe_scale");
    return 0;
}

// workspace of skyemb_probe_softmax_loss_grad: lossparts f64[2] | rowloss f32[m] | R f32[m K] | part f32[CH K F]
extern "C" int64_t skyemb_probe_softmax_ws_bytes(int m, int F, int K) {
    if (!probe_shape_ok(m, F) || K < SKYEMB_PROBE_MIN_K || K > SKYEMB_PROBE_MAX_K) return -1;
    return 16 + 4 * ((int64_t)m + (int64_t)m * K + (int64_t)CH * K * F);
}

extern "C" int skyemb_probe_softmax_loss_grad(const float *X, int64_t ldx, const int32_t *y, int m, int F, int K, const float *W,
                                              const float *b, double l2, double *loss, float *gW, float *gb, void *ws, int64_t ws_bytes,
                                              void *stream) {
    SKY_CHECK_ARG(K >= SKYEMB_PROBE_MIN_K && K <= SKYEMB_PROBE_MAX_K, "skyemb_probe_softmax_loss_grad: K=%d outside %d..%d", K,
                  SKYEMB_PROBE_MIN_K, SKYEMB_PROBE_MAX_K);
    SKY_CHECK_ARG(probe_shape_ok(m, F) && ldx >= F, "skyemb_probe_softmax_loss_grad: bad shape m=%d F=%d (F <= %d) ldx=%lld", m, F,
                  SKYEMB_PROBE_MAX_F, (long long)ldx);
    SKY_CHECK_ARG(X && y && W && b && loss && gW && gb && ws, "skyemb_probe_softmax_loss_grad: null pointer");
    SKY_CHECK_ARG((((uintptr_t)ws) & 7) == 0 && ws_bytes >= skyemb_probe_softmax_ws_bytes(m, F, K),
                  "skyemb_probe_softmax_loss_grad: workspace unaligned or smaller than skyemb_probe_softmax_ws_bytes");
    hipStream_t st = (hipStream_t)stream;
    double *lossparts = (double *)ws;
    float *rowloss = (float *)(lossparts + 2), *R = rowloss + m, *part = R + (int64_t)m * K;
    const int KP = K <= 4 ? 4 : K <= 8 ? 8 : 16;
    const dim3 g1((m + 4 * SM_RW - 1) / (4 * SM_RW)), g2((F + 63) / 64, CH);
    const size_t lds = (size_t)KP * SM_FT * 4;
    if (KP == 4) {
        hipLaunchKernelGGL(probe_softmax_fwd_kernel<4>, g1, dim3(256), lds, st, X, ldx, y, m, F, K, W, b, R, rowloss);
        hipLaunchKernelGGL(probe_softmax_wgrad_kernel<4>, g2, dim3(64), 0, st, X, ldx, m, F, K, (const float *)R, part);
    } else if (KP == 8) {
        hipLaunchKernelGGL(probe_softmax_fwd_kernel<8>, g1, dim3(256), lds, st, X, ldx, y, m, F, K, W, b, R, rowloss);
        hipLaunchKernelGGL(probe_softmax_wgrad_kernel<8>, g2, dim3(64), 0, st, X, ldx, m, F, K, (const float *)R, part);
    } else {
        hipLaunchKernelGGL(probe_softmax_fwd_kernel<16>, g1, dim3(256), lds, st, X, ldx, y, m, F, K, W, b, R, rowloss);
        hipLaunchKernelGGL(probe_softmax_wgrad_kernel<16>, g2, dim3(64), 0, st, X, ldx, m, F, K, (const float *)R, part);
    }
    hipLaunchKernelGGL(probe_softmax_reduce_kernel, dim3(K + 2), dim3(256), 0, st, (const float *)R, (const float *)rowloss, W, m, F, K,
                       gb, lossparts);
    hipLaunchKernelGGL(probe_softmax_finish_kernel, dim3((unsigned)(((int64_t)K * F + 255) / 256)), dim3(256), 0, st,
                       (const float *)part, W, m, F, K, l2, (const double *)lossparts, gW, loss);
    SKY_LAUNCH_CHECK("skyemb_probe_softmax_loss_grad");
    return 0;
}

extern "C" int skyemb_probe_gram(const float *Xc, int64_t ldx, const float *yc, int m, int F, double *G, double *q, double *ynorm2,
                                 void *stream) {
    SKY_CHECK_ARG(probe_shape_ok(m, F) && ldx >= F, "skyemb_probe_gram: bad shape m=%d F=%d (F <= %d) ldx=%lld", m, F,
                  SKYEMB_PROBE_MAX_F, (long long)ldx);
    SKY_CHECK_ARG(Xc && yc && G && q && ynorm2, "skyemb_probe_gram: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int T = (F + 63) / 64;
    hipLaunchKernelGGL(probe_gram_kernel, dim3(T, T), dim3(256), 0, st, Xc, ldx, m, F, G);
    hipLaunchKernelGGL(probe_xty_kernel, dim3(T + 1), dim3(64), 0, st, Xc, ldx, yc, m, F, q, ynorm2);
    SKY_LAUNCH_CHECK("skyemb_probe_gram");
    return 0;
}

extern "C" int skyemb_probe_enet_cd(const double *G, const double *q, const double *ynorm2, int F, double a1, double b2, int max_iter,
                                    double tol, double *w, int32_t *status, double *gap, void *stream) {
    SKY_CHECK_ARG(F > 0 && F <= SKYEMB_PROBE_MAX_F, "skyemb_probe_enet_cd: F=%d outside 1..%d", F, SKYEMB_PROBE_MAX_F);
    SKY_CHECK_ARG(max_iter > 0 && a1 >= 0.0 && b2 >= 0.0 && tol >= 0.0, "skyemb_probe_enet_cd: bad max_iter / penalties / tol");
    SKY_CHECK_ARG(G && q && ynorm2 && w && status && gap, "skyemb_probe_enet_cd: null pointer");
    if (int rc = sky_set_lds_limit((const void *)probe_enet_cd_kernel, CD_LDS_MAX, "skyemb_probe_enet_cd")) return rc;
    const size_t lds = (size_t)4 * F * 8 + (CD_NT / 64) * 8 + (size_t)F * 4;
    hipLaunchKernelGGL(probe_enet_cd_kernel, dim3(1), dim3(CD_NT), lds, (hipStream_t)stream, G, q, ynorm2, F, a1, b2, max_iter, tol, w,
                       status, gap);
    SKY_LAUNCH_CHECK("skyemb_probe_enet_cd");
    return 0;
}
