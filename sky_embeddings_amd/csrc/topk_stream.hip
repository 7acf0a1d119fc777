// Bank-streaming cosine top-k for Q <= 16 queries (the HBM-bound regime, e.g. the reference's one
// target vector): every wavefront streams its own slice of the bank straight from HBM into
// registers (16-byte loads, no LDS staging, no barriers), feeds v_mfma_f32_16x16x4_f32 and keeps
// private sorted top-k lists for the 16 queries in LDS.  Bit-identical to the tiled kernel and to
// oracle/topk_oracle.c: the fma chain runs over d = 0,1,2,... in order.
// The dot product, the A image and the list insertion live in topk_stream.h (shared with topk_tokens.hip).
#include "topk_stream.h"

namespace {

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void cosine_topk_stream_kernel(const float *__restrict__ tw, const float *__restrict__ qn,
                                                                 const float *__restrict__ bank, const float *__restrict__ xn,
                                                                 int Q, int64_t N, int D, int k, float eps, int64_t idx_offset,
                                                                 int64_t rows_per_wave, float *__restrict__ part_s,
                                                                 int64_t *__restrict__ part_i, const float *__restrict__ thr0) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nchunk = D >> 4;
    float4 *imgA = (float4 *)lds;                                   // [nchunk][64]: A fragments of every k-step
    float *ls_all = lds + (size_t)nchunk * 64 * 4;                  // [WAVES][16][k]
    int *li_all = (int *)(ls_all + (size_t)WAVES * 16 * k);        // [WAVES][16][k]
    // A operand image: lane (q = l&15, g = l>>4), element m: tw[q][16c + 4m + g]
    build_imgA<WAVES>(imgA, tw, Q, D, nchunk, tid);
    __syncthreads();
    float *ls = ls_all + (size_t)wave * 16 * k;
    int *li = li_all + (size_t)wave * 16 * k;
    const int wid = blockIdx.x * WAVES + wave;
    const int64_t r_begin = (int64_t)wid * rows_per_wave;
    int64_t r_end = r_begin + rows_per_wave;
    if (r_end > N) r_end = N;
    const int n_lane = lane & 15, g = lane >> 4;
    // per-query list sizes / thresholds live in registers of ALL lanes (wave-uniform arrays of 16)
    int n_in[16];
    float thr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { n_in[q] = 0; thr[q] = (thr0 && q < Q) ? thr0[q] : -INFINITY; }
    float floor_thr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) floor_thr[q] = thr[q];   // valid lower bound of the global k-th best (or -inf)
    float qn4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) qn4[r] = (4 * g + r) < Q ? qn[4 * g + r] : 0.f;

    for (int64_t n0 = r_begin; n0 < r_end; n0 += 16) {
        int64_t row = n0 + n_lane;
        const bool row_ok = row < r_end;
        if (!row_ok) row = r_end - 1;                                // clamp: masked below
        const float *src = bank + row * D + 4 * g;
        const f32x4 acc = stream_dot16(src, imgA, nchunk, lane);
        // C/D: col = lane&15 -> bank row n0 + n_lane, row = 4g + r -> query
        const float xnv = xn[row];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q_mine = 4 * g + r;
            const float s = (row_ok && q_mine < Q) ? finish_score(acc[r], qn4[r], xnv, eps) : -INFINITY;
            // candidates of the 4 queries {r, 4+r, 8+r, 12+r} (one per lane group), rows ascending within a group
            float my_thr = -INFINITY;
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) my_thr = (g == gg) ? thr[4 * gg + r] : my_thr;
            unsigned long long m = __ballot(s > my_thr);
            while (m) {
                const int srcl = __builtin_ctzll(m);
                m &= m - 1;
                const float cv = __shfl(s, srcl, 64);
                const int q = 4 * (srcl >> 4) + r;
                float *lsq = ls + q * k;
                int *liq = li + q * k;
                // wave-uniform per-query state (static indexing through the unrolled select)
                int nq = 0;
                float tq = -INFINITY;
#pragma unroll
                for (int gg = 0; gg < 4; ++gg)
                    if (q == 4 * gg + r) { nq = n_in[4 * gg + r]; tq = thr[4 * gg + r]; }
                if (!(cv > tq)) continue;
                const int new_n = stream_list_insert(lsq, liq, nq, k, cv, (int)(n0 + (srcl & 15)), lane);
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
    // write this wave's lists: part[q][wid][k]
    const int nlists = gridDim.x * WAVES;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (q >= Q) continue;
        const int64_t o = ((int64_t)q * nlists + wid) * k;
        // the list's entries and ONE terminator (-inf, -1): what follows the first negative index is unspecified (contract
        // of skyemb_cosine_topk; with a pruning floor a wave keeps a handful of rows, and 2048 lists x 16 queries x k padded
        // slots were 39 MB written here and read back by the merge)
        const int n_out = n_in[q] < k ? n_in[q] + 1 : k;
        for (int e = lane; e < n_out; e += 64) {
            const bool have = e < n_in[q];
            part_s[o + e] = have ? ls[q * k + e] : -INFINITY;
            part_i[o + e] = have ? idx_offset + (int64_t)li[q * k + e] : -1;
        }
    }
}

// Exact scores of a (small) set of rows for Q <= 16 queries, same arithmetic as the kernel above: one wave per 16 rows,
// rows straight from HBM into registers.  Serves the pruning floor's row sample (25,600 rows: 1,600 waves) -- the tiled
// score kernel took 50 us for it on 100 workgroups.
template <int WAVES, bool TILEMAX>
__global__ __launch_bounds__(WAVES * 64) void cosine_scores_stream_kernel(const float *__restrict__ tw, const float *__restrict__ qn,
                                                                          const float *__restrict__ bank, const float *__restrict__ xn,
                                                                          int Q, int64_t N, int D, float eps, float *__restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nchunk = D >> 4;
    float4 *imgA = (float4 *)lds;
    build_imgA<WAVES>(imgA, tw, Q, D, nchunk, tid);
    __syncthreads();
    const int n_lane = lane & 15, g = lane >> 4;
    float qn4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) qn4[r] = (4 * g + r) < Q ? qn[4 * g + r] : 0.f;
    const int64_t ntile = (N + 15) / 16;
    for (int64_t t = (int64_t)blockIdx.x * WAVES + wave; t < ntile; t += (int64_t)gridDim.x * WAVES) {
        const int64_t n0 = t * 16;
        int64_t row = n0 + n_lane;
        const bool row_ok = row < N;
        if (!row_ok) row = N - 1;
        const float *src = bank + row * D + 4 * g;
        const f32x4 acc = stream_dot16(src, imgA, nchunk, lane);
        const float xnv = xn[row];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = 4 * g + r;
            float sc = (row_ok && q < Q) ? finish_score(acc[r], qn4[r], xnv, eps) : -INFINITY;
            if (!TILEMAX) {
                if (row_ok && q < Q) scores[(int64_t)q * N + n0 + n_lane] = sc;
            } else {
                // maximum over the tile's 16 rows (the 16 lanes of this lane group): scores[q][tile]
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) sc = fmaxf(sc, __shfl_xor(sc, o, 64));
                if (n_lane == 0 && q < Q) scores[(int64_t)q * ntile + t] = sc;
            }
        }
    }
}

}  // namespace

bool skyemb_topk_stream_applicable(int Q, int D, int k) { return Q <= 16 && k <= 128 && D % (16 * UNROLL) == 0 && D <= 1024; }

// 8 waves per workgroup when their private lists fit next to the A image in 160 KiB of LDS, else 4
static int stream_waves(int D, int k) {
    const size_t img = (size_t)(D >> 4) * 64 * 16;
    return img + (size_t)2 * 8 * 16 * k * 4 <= 160 * 1024 ? 8 : 4;
}

int skyemb_topk_stream_lists(int64_t N, int D, int k) {
    const int waves = stream_waves(D, k);
    int64_t blocks = 256;
    while (blocks > 1 && blocks * waves * 64 > N) blocks >>= 1;   // at least 64 rows per wave
    return (int)(blocks * waves);
}

bool skyemb_scores_stream_applicable(int Q, int64_t N, int D) { return Q <= 16 && D % (16 * UNROLL) == 0 && D <= 1024 && N <= (1 << 20); }

int skyemb_scores_stream_launch(const float *tw, const float *qn, const float *bank, const float *xn, int Q, int64_t N, int D,
                                float eps, float *scores, hipStream_t st) {
    const size_t smem = (size_t)(D >> 4) * 64 * 16;
    int64_t blocks = ceil_div64(ceil_div64(N, 16), 4);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL((cosine_scores_stream_kernel<4, false>), dim3((unsigned)blocks), dim3(256), smem, st, tw, qn, bank, xn, Q, N, D, eps, scores);
    SKY_LAUNCH_CHECK("skyemb_cosine_scores(stream)");
    return 0;
}

int skyemb_scores_stream_tilemax_launch(const float *tw, const float *qn, const float *bank, const float *xn, int Q, int64_t N, int D,
                                        float eps, float *tile_max, hipStream_t st) {
    const size_t smem = (size_t)(D >> 4) * 64 * 16;
    int64_t blocks = ceil_div64(ceil_div64(N, 16), 4);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL((cosine_scores_stream_kernel<4, true>), dim3((unsigned)blocks), dim3(256), smem, st, tw, qn, bank, xn, Q, N, D, eps, tile_max);
    SKY_LAUNCH_CHECK("skyemb_cosine_sample_floor(scores)");
    return 0;
}

int skyemb_topk_stream_launch(const float *tw, const float *qn, const float *bank, const float *xn, int Q, int64_t N, int D,
                              int k, float eps, int64_t idx_offset, int nlists, float *part_s, int64_t *part_i,
                              const float *thr0, hipStream_t st) {
    const int waves = stream_waves(D, k);
    const int blocks = nlists / waves;
    const size_t smem = sizeof(float) * ((size_t)(D >> 4) * 64 * 4 + 2 * (size_t)waves * 16 * k);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void *)cosine_topk_stream_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           160 * 1024);
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void *)cosine_topk_stream_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024);
        if (e != hipSuccess) {
            skyemb_set_error("skyemb_cosine_topk(stream): hipFuncSetAttribute: %s", hipGetErrorString(e));
            return 2;
        }
        attr_set = true;
    }
    int64_t rows_per_wave = ceil_div64(ceil_div64(N, nlists), 16) * 16;
    if (waves == 8)
        hipLaunchKernelGGL(cosine_topk_stream_kernel<8>, dim3(blocks), dim3(512), smem, st, tw, qn, bank, xn, Q, N, D, k, eps,
                           idx_offset, rows_per_wave, part_s, part_i, thr0);
    else
        hipLaunchKernelGGL(cosine_topk_stream_kernel<4>, dim3(blocks), dim3(256), smem, st, tw, qn, bank, xn, Q, N, D, k, eps,
                           idx_offset, rows_per_wave, part_s, part_i, thr0);
    SKY_LAUNCH_CHECK("skyemb_cosine_topk(stream)");
    return 0;
}
