// Multi-tensor AdamW: ONE launch steps any set of segments of a flat buffer, every segment with the scalars of its parameter group
// (the downstream predictor: layer-wise lr decay gives every layer two groups with a rate of their own, a linear probe steps a few
// scattered tensors -- neither fits the [decayed | not decayed] layout skyemb_adamw steps in one launch).  The host plans a table
// of work items once (skyemb_adamw_segments_plan: sort, join, cut); the kernel walks it.  The element update is adamw_math.h's, so
// the result is bit-identical to one skyemb_adamw launch per segment.  HBM-bound like adamw_kernel, whose memory pattern it keeps.
#include <algorithm>
#include <vector>

#include "common.h"
#include "adamw_math.h"

// elements of one work item (DESIGN.md section 7 records the sizes that were tried); -DSKY_ADAMW_CHUNK=... builds the variants
#ifndef SKY_ADAMW_CHUNK
#define SKY_ADAMW_CHUNK 8192
#endif
#define SKY_ADAMW_MAX_GROUPS 64     // 64 x 32 B = 2 KB of the 4 KB of kernel arguments
#define SKY_ADAMW_MAX_GRID 4096     // adamw_kernel's cap: 16 workgroups per compute unit

static_assert(sizeof(skyemb_adamw_group) == 32, "skyemb_adamw_group is 32 bytes (include/skyemb.h)");
static_assert(sizeof(skyemb_adamw_segment) == 24, "skyemb_adamw_segment is 24 bytes (include/skyemb.h)");
static_assert(sizeof(skyemb_adamw_work) == 16, "skyemb_adamw_work is 16 bytes (include/skyemb.h)");
static_assert(SKY_ADAMW_CHUNK > 0 && SKY_ADAMW_CHUNK % 2048 == 0, "a chunk is whole trips of 256 lanes x 2 float4");

namespace {

struct SegGroups {
    skyemb_adamw_group g[SKY_ADAMW_MAX_GROUPS];
};

template <typename T>
__global__ __launch_bounds__(256) void adamw_segments_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                             float *__restrict__ v, T *__restrict__ p_lp,
                                                             const skyemb_adamw_work *__restrict__ table, int n_work,
                                                             const SegGroups groups, float grad_scale,
                                                             const uint32_t *__restrict__ skip) {
    // overflow guard, as adamw_kernel's: one word read by every thread, a uniform branch
    if (skip && *skip) return;
    for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
        // the item and its group are the same for the whole workgroup: scalar loads (the groups sit in the kernel arguments)
        const skyemb_adamw_work it = table[w];
        const skyemb_adamw_group &gr = groups.g[it.group];
        const SkyAdamScalars sc = sky_adam_scalars(gr.lr, gr.bc1, gr.bc2, gr.beta1, gr.beta2, gr.eps, gr.wd, grad_scale);
        const bool decayed = gr.decayed != 0;
        const int n4 = it.n / 4;
        float *pw = p + it.offset, *mw = m + it.offset, *vw = v + it.offset;
        const float *gw = g + it.offset;
        T *lw = p_lp + it.offset;
        // two float4 groups per lane and trip, as adamw_kernel; a lane past the end of the item touches nothing
        for (int i0 = threadIdx.x; i0 < n4; i0 += 2 * 256) {
            f32x4 pv[2], gv[2], mv[2], vv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int i = i0 + u * 256;
                if (i < n4) {
                    pv[u] = *(const f32x4 *)(pw + 4 * i);
                    gv[u] = *(const f32x4 *)(gw + 4 * i);
                    mv[u] = *(const f32x4 *)(mw + 4 * i);
                    vv[u] = *(const f32x4 *)(vw + 4 * i);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int i = i0 + u * 256;
                if (i >= n4) break;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float pj = pv[u][j], mj = mv[u][j], vj = vv[u][j];
                    sky_adamw_update(gv[u][j], pj, mj, vj, decayed, sc);
                    pv[u][j] = pj; mv[u][j] = mj; vv[u][j] = vj;
                }
                *(f32x4 *)(pw + 4 * i) = pv[u];
                *(f32x4 *)(mw + 4 * i) = mv[u];
                *(f32x4 *)(vw + 4 * i) = vv[u];
                store4<T>(lw + 4 * i, pv[u][0], pv[u][1], pv[u][2], pv[u][3]);
            }
        }
    }
}

struct Run {
    int64_t offset, n;
    int32_t group, index;
};

}  // namespace

#define SEG_REFUSE(cond, ...)                   \
    do {                                        \
        if (!(cond)) {                          \
            skyemb_set_error(__VA_ARGS__);      \
            return 1;                           \
        }                                       \
    } while (0)

extern "C" int skyemb_adamw_segments_limits(int32_t *max_groups, int32_t *chunk_elems, int32_t *max_grid) {
    if (max_groups) *max_groups = SKY_ADAMW_MAX_GROUPS;
    if (chunk_elems) *chunk_elems = SKY_ADAMW_CHUNK;
    if (max_grid) *max_grid = SKY_ADAMW_MAX_GRID;
    return 0;
}

// host only: no HIP call, no globals (runs on a machine without a GPU)
extern "C" int skyemb_adamw_segments_plan(const skyemb_adamw_segment *segs, int n_segs, int n_groups, int64_t buffer_n,
                                          void *table_host, int64_t table_bytes, int64_t *need_bytes, int32_t *n_work) {
    const char *who = "skyemb_adamw_segments_plan";
    SEG_REFUSE(segs != nullptr && need_bytes != nullptr && n_work != nullptr, "%s: null argument", who);
    SEG_REFUSE(n_segs > 0, "%s: n_segs = %d: expected at least one segment", who, n_segs);
    SEG_REFUSE(n_groups >= 1 && n_groups <= SKY_ADAMW_MAX_GROUPS, "%s: n_groups = %d: expected 1 .. %d", who, n_groups,
               SKY_ADAMW_MAX_GROUPS);
    std::vector<Run> runs((size_t)n_segs);
    for (int i = 0; i < n_segs; ++i) {
        const skyemb_adamw_segment &s = segs[i];
        SEG_REFUSE(s.offset >= 0 && s.offset % 4 == 0, "%s: segment %d: offset %lld is not a non-negative multiple of 4", who, i,
                   (long long)s.offset);
        SEG_REFUSE(s.n > 0 && s.n % 4 == 0, "%s: segment %d: length %lld is not a positive multiple of 4", who, i, (long long)s.n);
        SEG_REFUSE(s.offset < buffer_n && s.n <= buffer_n - s.offset, "%s: segment %d: [%lld, %lld) leaves the buffer [0, %lld)", who, i,
                   (long long)s.offset, (long long)s.offset + (long long)s.n, (long long)buffer_n);
        SEG_REFUSE(s.group >= 0 && s.group < n_groups, "%s: segment %d: group %d outside [0, %d)", who, i, s.group, n_groups);
        runs[(size_t)i] = Run{s.offset, s.n, s.group, i};
    }
    // 1. by offset (the input index breaks ties, which are overlaps and refused below)
    std::sort(runs.begin(), runs.end(), [](const Run &a, const Run &b) { return a.offset != b.offset ? a.offset < b.offset : a.index < b.index; });
    for (size_t i = 1; i < runs.size(); ++i)
        SEG_REFUSE(runs[i - 1].offset + runs[i - 1].n <= runs[i].offset, "%s: segment %d: [%lld, %lld) overlaps segment %d: [%lld, %lld)", who,
                   runs[i].index, (long long)runs[i].offset, (long long)(runs[i].offset + runs[i].n), runs[i - 1].index,
                   (long long)runs[i - 1].offset, (long long)(runs[i - 1].offset + runs[i - 1].n));
    // 2. neighbours that touch and share a group become one run
    size_t n_runs = 0;
    for (size_t i = 0; i < runs.size(); ++i) {
        if (n_runs && runs[n_runs - 1].group == runs[i].group && runs[n_runs - 1].offset + runs[n_runs - 1].n == runs[i].offset)
            runs[n_runs - 1].n += runs[i].n;
        else
            runs[n_runs++] = runs[i];
    }
    // 3. every run in items of at most SKY_ADAMW_CHUNK elements, the short one last
    int64_t items = 0;
    for (size_t i = 0; i < n_runs; ++i) items += (runs[i].n + SKY_ADAMW_CHUNK - 1) / SKY_ADAMW_CHUNK;
    SEG_REFUSE(items <= INT32_MAX, "%s: %lld work items: more than 2^31 - 1", who, (long long)items);
    *need_bytes = items * (int64_t)sizeof(skyemb_adamw_work);
    *n_work = (int32_t)items;
    if (!table_host) return 0;
    SEG_REFUSE(table_bytes >= *need_bytes, "%s: table of %lld bytes: %lld work items need %lld", who, (long long)table_bytes, (long long)items,
               (long long)*need_bytes);
    skyemb_adamw_work *out = (skyemb_adamw_work *)table_host;
    for (size_t i = 0; i < n_runs; ++i)
        for (int64_t o = 0; o < runs[i].n; o += SKY_ADAMW_CHUNK) {
            const int64_t left = runs[i].n - o;
            *out++ = skyemb_adamw_work{runs[i].offset + o, (int32_t)(left < SKY_ADAMW_CHUNK ? left : SKY_ADAMW_CHUNK), runs[i].group};
        }
    return 0;
}

extern "C" int skyemb_adamw_segments(float *p, const float *g, float *m, float *v, void *p_lp, int dtype, const void *table_dev,
                                     int32_t n_work, const skyemb_adamw_group *groups, int n_groups, float grad_scale,
                                     const uint32_t *skip, void *stream) {
    const char *who = "skyemb_adamw_segments";
    SKY_CHECK_ARG(p && g && m && v && p_lp && table_dev && groups, "%s: null pointer", who);
    SKY_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(table_dev) &&
                      (((uintptr_t)p_lp) & (dtype == SKYEMB_F32 ? 15 : 7)) == 0 && (((uintptr_t)skip) & 3) == 0,
                  "%s: unaligned buffers", who);
    SKY_CHECK_ARG(n_work > 0, "%s: n_work = %d: expected at least one work item", who, n_work);
    SKY_CHECK_ARG(n_groups >= 1 && n_groups <= SKY_ADAMW_MAX_GROUPS, "%s: n_groups = %d: expected 1 .. %d", who, n_groups,
                  SKY_ADAMW_MAX_GROUPS);
    SKY_CHECK_ARG(dtype == SKYEMB_F32 || sky_is_lp(dtype), "%s: bad dtype %d", who, dtype);
    // the groups travel by value in the kernel arguments: no host-to-device copy in front of the step (adamw.hip, skyemb_set_scalars)
    SegGroups gs;
    memset(&gs, 0, sizeof(gs));
    memcpy(gs.g, groups, (size_t)n_groups * sizeof(skyemb_adamw_group));
    const dim3 grid((unsigned)(n_work < SKY_ADAMW_MAX_GRID ? n_work : SKY_ADAMW_MAX_GRID)), block(256);
    const skyemb_adamw_work *table = (const skyemb_adamw_work *)table_dev;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == SKYEMB_BF16)
        hipLaunchKernelGGL((adamw_segments_kernel<bf16_t>), grid, block, 0, st, p, g, m, v, (bf16_t *)p_lp, table, n_work, gs, grad_scale, skip);
    else if (dtype == SKYEMB_F16)
        hipLaunchKernelGGL((adamw_segments_kernel<f16_t>), grid, block, 0, st, p, g, m, v, (f16_t *)p_lp, table, n_work, gs, grad_scale, skip);
    else
        hipLaunchKernelGGL((adamw_segments_kernel<float>), grid, block, 0, st, p, g, m, v, (float *)p_lp, table, n_work, gs, grad_scale, skip);
    SKY_LAUNCH_CHECK(who);
    return 0;
}
