// Launch plan of the attention core (skyemb_mha_fwd / skyemb_mha_bwd): which kernel family a shape runs on and with what geometry.
// sky_mha_plan is a function of its arguments alone -- no HIP call, no environment, no state -- so skyemb_mha_plan can answer on a
// machine without a device and tests/test_attention_reference_cpu.py can hold the Python restatement (tests/attention_reference.py)
// against it.  The kernels live in attention.hip (lds, stream: every dtype, fp32 arithmetic) and attention_mfma.hip (the rest:
// bf16 / fp16 at head dim 32 / 64); their drivers launch what the plan says and decide nothing.
#pragma once
#include <stdint.h>

#include "../../include/skyemb.h"

constexpr int MHA_LDS_BLOCK = 65536;          // lds: as many waves (heads) per workgroup as fit this, at most 4, at least 1
constexpr int MHA_LDS_LIMIT = 160 * 1024;     // a workgroup's LDS: a whole-head plan past it goes to the streaming kernels
constexpr int MHA_STREAM_MAX_HD = 512;        // the streaming kernels' widest head (SH_MAXHD)
constexpr int MHA_MAX_NT = 4;                 // strips: one wave per 32 tokens, up to 128 tokens
constexpr int MHA_LB = 64, MHA_LW = 4;        // long: key / query blocks of 64 token rows, four waves per workgroup

enum { MHA_OK = 0, MHA_BAD_SHAPE, MHA_TOO_LONG, MHA_HEAD_TOO_WIDE };    // sky_mha_plan's answer; attention.hip holds the texts

inline int sky_mha_plan(bool bwd, int dtype, int B, int N, int H, int hd, int switches, skyemb_mha_plan_t *p) {
    if (!(B > 0 && N > 0 && H > 0 && hd > 0 && hd % 8 == 0)) return MHA_BAD_SHAPE;
    if (N > SKYEMB_MHA_MAX_N) return MHA_TOO_LONG;
    *p = skyemb_mha_plan_t{};
    p->grid_x = B * H;
    p->grid_y = 1;
    const bool lp = dtype == SKYEMB_BF16 || dtype == SKYEMB_F16;
    if (lp && (hd == 32 || hd == 64) && !(switches & SKYEMB_MHA_SW_NO_MFMA)) {
        p->hd = hd;
        if (N > 32 * MHA_MAX_NT) {
            p->family = SKYEMB_MHA_MFMA_LONG;
            p->waves = MHA_LW;
            if (!bwd) p->grid_y = (N + 32 * MHA_LW - 1) / (32 * MHA_LW);
            else p->lds_bytes = 2 * MHA_LB * (hd + 8) * 2 + 8 * (int64_t)((N + MHA_LB - 1) / MHA_LB * MHA_LB);
        } else if (N > 32) {
            p->family = SKYEMB_MHA_MFMA_STRIP;
            p->waves = (N + 31) / 32;
            p->lds_bytes = (bwd ? 4 : 2) * (((N + 3) & ~3) + 4) * (hd + 8) * 2;
            if (p->lds_bytes > 65536) p->lds_limit = 4 * (32 * p->waves + 4) * (hd + 8) * 2;    // the longest sequence of this instance
        } else {
            const int P = N <= 16 ? 32 / N : 1;                   // samples packed into one wave's 32-row tile
            p->family = P > 1 ? SKYEMB_MHA_MFMA_PACKED : SKYEMB_MHA_MFMA_SINGLE;
            p->nheads = ((B + P - 1) / P) * H;
            // fewer four-wave workgroups than twice the compute units: one tile per workgroup, so that the tiles spread over every CU
            const bool one = switches & SKYEMB_MHA_SW_WPB1 ? true : switches & SKYEMB_MHA_SW_WPB4 ? false : (p->nheads + 3) / 4 < 512;
            p->waves = one ? 1 : 4;
            p->grid_x = one ? p->nheads : (p->nheads + 3) / 4;
        }
        p->block = 64 * p->waves;
        return MHA_OK;
    }
    const int pitch = hd + 4, NP = N + 1;
    p->per_wave_floats = ((bwd ? 4 : 3) * N * pitch + (bwd ? 2 : 1) * N * NP + 3) & ~3;
    const int64_t per = (int64_t)p->per_wave_floats * 4;
    const int fit = (int)(MHA_LDS_BLOCK / per), w = fit > 4 ? 4 : fit < 1 ? 1 : fit;
    if (per * w > MHA_LDS_LIMIT) {         // the head does not fit: the streaming kernel
        if (hd > MHA_STREAM_MAX_HD) return MHA_HEAD_TOO_WIDE;
        p->family = SKYEMB_MHA_STREAM;
        p->per_wave_floats = 0;
        p->waves = 4;
        if (!bwd) p->grid_y = (N + 3) / 4;                         // one wave per query row
        else p->lds_bytes = 4 * (8 * MHA_STREAM_MAX_HD + 4 * 128 + 2 * (int64_t)N);
    } else {
        p->family = SKYEMB_MHA_LDS;
        p->waves = w;
        p->grid_x = (B * H + w - 1) / w;
        p->lds_bytes = per * w;
        if (p->lds_bytes > 65536) p->lds_limit = MHA_LDS_LIMIT;
    }
    p->block = 64 * p->waves;
    return MHA_OK;
}
