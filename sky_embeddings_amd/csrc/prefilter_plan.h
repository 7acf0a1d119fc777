// Launch plan of the two-stage many-query searches (topk_prefilter.hip): everything their host layer decides -- the variant, the slice
// schedule, the stage-1 instance family, the LDS bytes, the constants handed to the kernels.  sky_prefilter_plan is a function of its
// request alone -- no HIP call, no environment, no state -- so skyemb_prefilter_plan answers without a device and
// tests/test_prefilter_plan_cpu.py holds the Python restatements of the schedule against it.  topk_prefilter.hip holds the kernels, the
// refusal texts and ONE driver that launches what the plan says and decides nothing.
#pragma once
#include <algorithm>
#include <math.h>
#include <stdint.h>

#include "../../include/skyemb.h"

namespace pfplan {

// the geometry of the kernels (topk_prefilter.hip static_asserts that its own constants agree)
constexpr int BT = 256, BK = 32, QPAD = 256, NSTAGE = 4, STAGE_BYTES = 32768, SCAP = 2048, RESCORE_MAX = 256, TOK_KMAX = 256;
constexpr int qtile(bool lo) { return lo ? 128 : 256; }
constexpr int cap_of(int k) { return k <= 128 ? 4096 : 8192; }                  // slots of a query's candidate list
constexpr int lds_stage1(bool lo) { return NSTAGE * STAGE_BYTES + (qtile(lo) + BT) * 16 + SCAP * 8 + 16; }
constexpr int LDS_STAGE1_LIMIT = lds_stage1(false);                               // the larger of the two variants
constexpr int LDS_SELECT_LIMIT = 2 * 8192 * 4 + 272 * 4;                          // select_kernel at cap 8192
constexpr int LDS_TOKEN_RESCORE_LIMIT = (2 * TOK_KMAX + 8192) * 8 + 4096 * 4 + 264 * 4;    // token re-score at cap 8192, D 4096
// which of its two variants a bf16 search runs when SKYEMB_PREFILTER_LO is unset: the one measured faster
constexpr bool BF16_DEFAULT_LO = false;

// sky_prefilter_plan's answer; topk_prefilter.hip holds the texts
enum { PF_OK = 0, PF_BAD_REQUEST, PF_ROWS_SHAPE, PF_MEAN_COMBINE, PF_MEAN_SHAPE, PF_TOPT_MEAN, PF_TOKENS_COMBINE, PF_TOKENS_SHAPE,
       PF_TOPT_RANGE, PF_SEL_INFO, PF_SEL_ONLY_TAIL, PF_SEL_DIRECT, PF_TOO_LARGE };

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the shape limits of the three routes (skyemb_topk_prefilter_applicable, skyemb_token_prefilter_applicable, skyemb_token_mean_
// prefilter_applicable).  Rows: the fp16 pass pays from a few query tiles on; the re-score list must leave room above k
inline bool rows_shape_ok(int Q, int64_t N, int D, int k) {
    return Q >= 17 && D % BK == 0 && D >= 4 * BK && D <= 4096 && k >= 1 && k <= RESCORE_MAX - 64 && N >= 8 * BT && N < (1ll << 31);
}
inline bool token_common_ok(int Q, int64_t N, int P, int D, int k) {
    return Q >= 1 && N >= 1 && N < (1ll << 31) && P >= 1 && P <= 64 && 64 % P == 0 && D % BK == 0 && D >= 4 * BK && D <= 4096 && k >= 1 &&
           k <= TOK_KMAX && k <= N && N * P < (1ll << 31);
}
inline bool tokens_shape_ok(int Q, int64_t N, int P, int D, int k) { return token_common_ok(Q, N, P, D, k) && N * P >= 8 * BT; }
inline bool mean_shape_ok(int Q, int64_t N, int P, int D, int k) { return token_common_ok(Q, N, P, D, k) && N >= 8 * BT; }

// The proven relative error bound of stage 1's dot products: restates topk_prefilter.hip's eps_a_of, eps_a_bf16_of and eps_m_of (the eps exports,
// the preparation calls).  They MUST MOVE TOGETHER, same order of summation: tests/test_prefilter_plan_cpu.py holds them bit-equal at every D.
inline double eps_of(int kind, int bank, int D, bool lo) {
    const double acc = 6.06 * D * 0x1p-24;
    if (kind == SKYEMB_PF_TOKENS_MEAN)      // eps_m: the pooled image is a ROUNDED 16-bit image, as the fp32 bank's fp16 image is
        return bank == SKYEMB_PF_BANK_BF16 ? (lo ? 0x1p-9 + 0x1p-17 : 0x1p-8 + 0x1p-17) + acc + D * 0x1p-37 : eps_of(SKYEMB_PF_ROWS, SKYEMB_PF_BANK_F32, D, lo);
    if (bank == SKYEMB_PF_BANK_BF16) return (lo ? 0x1p-18 : 0x1p-9) + acc + D * 0x1p-38;
    if (bank == SKYEMB_PF_BANK_F16) return (lo ? 0x1p-21 : 0x1p-11 + 0x1p-21) + acc + sqrt((double)D) * 0x1p-27;
    return (lo ? 0x1p-11 + 0x1p-21 : 0x1p-10 + 0x1p-21) + acc + 2.0 * sqrt((double)D) * 0x1p-27;
}

inline int sky_prefilter_plan(const skyemb_prefilter_request_t &r, skyemb_prefilter_plan_t *p) {
    const bool rows = r.kind == SKYEMB_PF_ROWS, mean = r.kind == SKYEMB_PF_TOKENS_MEAN, sel = r.sel != 0;
    if (!(rows || mean || r.kind == SKYEMB_PF_TOKENS) || r.bank < SKYEMB_PF_BANK_F32 || r.bank > SKYEMB_PF_BANK_BF16 ||
        (!rows && r.bank == SKYEMB_PF_BANK_F32) || r.lo < 0 || r.lo > SKYEMB_PF_LO_UNSET || (mean && sel) || (rows && sel && r.has_thr0))
        return PF_BAD_REQUEST;               // no entry point takes such a call
    const int Q = r.Q, P = rows ? 1 : r.P, D = r.D, k = r.k;
    const int64_t N = r.N, R = rows || mean || N >= (1ll << 31) ? N : N * P;      // R: stage 1's rows -- token rows (whole images, P | 64 | BT); mean: images
    int top_t = rows || mean ? 0 : r.top_t;
    if (rows) {
        if (!rows_shape_ok(Q, N, D, k)) return PF_ROWS_SHAPE;
    } else if (mean) {
        if (r.combine != SKYEMB_COMBINE_MEAN) return PF_MEAN_COMBINE;
        if (!mean_shape_ok(Q, N, P, D, k)) return PF_MEAN_SHAPE;
    } else {
        if (top_t != 0 && r.combine == SKYEMB_COMBINE_MEAN) return PF_TOPT_MEAN;
        if (r.combine != SKYEMB_COMBINE_MIN && r.combine != SKYEMB_COMBINE_MAX) return PF_TOKENS_COMBINE;
        if (!tokens_shape_ok(Q, N, P, D, k)) return PF_TOKENS_SHAPE;
        if (top_t < 0 || top_t > (P < 16 ? P : 16)) return PF_TOPT_RANGE;
    }
    *p = skyemb_prefilter_plan_t{};
    const bool resident = r.bank != SKYEMB_PF_BANK_F32, bf = r.bank == SKYEMB_PF_BANK_BF16;
    if (r.combine == SKYEMB_COMBINE_MAX || top_t == P) top_t = 0;     // d[0] is the max and d[P - 1] the min: the plain search
    // stage 1 under 'min' with 1 <= top_t < P: top_t == 1 is the OR fold of 'max', else the CNT instances count
    p->top_t = top_t, p->sel = sel, p->bf = bf, p->tok = !rows && !mean, p->cnt = top_t > 1, p->rows = R;
    // The variant: three rules.
    //   rows / tokens, fp16 operands  one pass (hi only) unless SKYEMB_PREFILTER_LO=1: half the matrix work, intervals ~1.6x wider
    //   bf16 operands                 =0 and =1 are both obeyed; unset, BF16_DEFAULT_LO
    //   mean                          hi + lo unless =0 -- stage 1 is P times smaller than the token route's and stage 2, P rows per
    //                                 candidate, is what the search costs: the tighter bound pays (whatever the operand format)
    const bool lo = mean ? r.lo != 0 : bf && r.lo == SKYEMB_PF_LO_UNSET ? BF16_DEFAULT_LO : r.lo == 1;
    p->use_lo = lo, p->cap = cap_of(k), p->q_padded = (Q + QPAD - 1) / QPAD * QPAD;
    // positions the slices walk: the whole tiles -- of a resident bank; the last R % BT rows follow from the tail tile (an fp32
    // bank's image is padded to whole tiles: its last tile is a position like any other).  Under a selection: the live-tile list's.
    const bool ragged = resident && R % BT != 0;
    p->T_tail = (int)(R / BT);
    if (sel) {
        if (!(r.n_live >= 1 && r.n_live <= ceil_div(R, BT) && (r.last_live == 0 || r.last_live == 1))) return PF_SEL_INFO;
        p->has_tail = ragged && r.last_live;
        p->T = r.n_live - p->has_tail;
        if (p->T < 1) return PF_SEL_ONLY_TAIL;
        if (!rows && !(r.direct_sel >= 1 && r.direct_sel <= r.n_live)) return PF_SEL_DIRECT;
    } else {
        p->has_tail = ragged;
        p->T = resident ? p->T_tail : (int)ceil_div(R, BT);
    }
    const int T = p->T;
    // stage 1 counts an XCD's work items (its bank tiles x the query tiles) and a workgroup's k-steps in 32-bit integers
    if (!(ceil_div(ceil_div(R, BT), 8) * ceil_div(Q, qtile(lo)) * (D / BK) < (1ll << 31))) return PF_TOO_LARGE;
    p->eps_a = eps_of(r.kind, r.bank, D, lo);
    const double raised = p->eps_a * (1.0 + 1e-6);
    p->eps_a_f32 = (float)raised;
    // mean: eps / eps_m, raised (the query's third test parameter is N_q eps / qn = (eps_m N_q) gfac / qn); NaN flags every query
    p->gfac = !mean ? -1.0f : r.eps >= 0.f && r.eps < INFINITY ? (float)((double)r.eps / raised * (1.0 + 1e-6)) : NAN;
    while ((1 << p->lgp) < P) ++p->lgp;
    p->fold = mean ? 2 : r.combine == SKYEMB_COMBINE_MAX ? 1 : 0;
    // (the instances without CNT read every bit above bit 7 as "is max": top_t travels only to those that count)
    p->tok_word = rows ? 0 : p->lgp | ((p->fold == 1 || top_t == 1 ? 1 : 0) << 8) | (p->cnt ? top_t << 16 : 0);
    p->lds_stage1 = lds_stage1(lo), p->lds_stage1_limit = LDS_STAGE1_LIMIT;
    p->lds_close = rows ? 2 * p->cap * 4 + 272 * 4 : (TOK_KMAX + p->cap + TOK_KMAX) * 8 + D * 4 + 264 * 4;
    p->lds_close_limit = rows ? LDS_SELECT_LIMIT : LDS_TOKEN_RESCORE_LIMIT;
    p->lds_rescore = rows ? D * 4 + RESCORE_MAX * 8 : 0;
    // The slice ends.  Rows: [0, first) is taken whole (<= cap / 2 rows: slot = row) unless a floor came in.  The slice after it meets
    // a threshold that still passes ~5 % of the pairs, so it is kept short -- ~96 k rows or 1/128 of the tiles -- and appends
    // directly; from then on, ends at 1/32, 1/8, 1/2 and all of the tiles, staged.  Token routes: no take-all slice (first = 0); the
    // direct slice is counted in images (96 k of them).
    // The two routes compute direct_end by different rules, kept as they are:
    //   rows             max(ceil(96 k / BT), T / 128, first + 1), NOT clipped to T (the loop below clips)
    //   tokens / mean    max(min(ceil(96 k rows-per-image / BT), T), T / 128, 1)
    //   tokens, selected min(direct_sel, T): the caller has counted the 96 k SELECTED images (search.py) -- no T / 128 floor here
    if (rows) {
        p->first = std::min(p->cap / 2 / BT, T);
        // (under a selection the slots are positions in the live list x BT: all of them are written)
        p->first_rows = sel || (int64_t)p->first * BT < N ? p->first * BT : (int)N;
        p->direct_end = std::max({(int)ceil_div((int64_t)96 * k, BT), T / 128, p->first + 1});
    } else {
        const int64_t want = ceil_div((int64_t)96 * k * (mean ? 1 : P), BT);
        p->direct_end = sel ? std::min(r.direct_sel, T) : std::max({(int)std::min<int64_t>(want, T), T / 128, 1});
    }
    const int ends[SKYEMB_PF_MAX_SLICES] = {p->first, p->direct_end, T / 32, T / 8, T / 2, T};
    // rows: a caller's floor (256 k sampled rows) is tight enough to stage at once; tokens: the first slice appends directly regardless
    bool direct_done = rows && r.has_thr0, tail_done = false;
    int t0 = 0;
    for (int e = 0; e < SKYEMB_PF_MAX_SLICES; ++e) {
        int t1 = p->ends[e] = ends[e];
        if (e == 0 && r.has_thr0) continue;                    // a valid floor is as good as the take-all slice: skipped
        if (t1 <= t0) continue;
        // An end is clipped to T only AFTER it was compared with t0.  Rows with T == first: direct_end = first + 1 passes the
        // comparison and is clipped to T = t0 -- ONE EMPTY direct launch over [T, T) and a second final select.  (No other end can
        // exceed T, so nothing else is ever clipped.)
        if (t1 > T) t1 = T;
        skyemb_prefilter_slice_t &s = p->slice[p->n_slices++];
        s.t0 = t0, s.t1 = t1, s.mode = e == 0 ? 0 : !direct_done ? 1 : 2, s.bucket = s.mode == 2;
        if (e != 0) direct_done = true;
        // The last R % BT rows of a resident bank ride behind the first slice that ends at T (a later, empty one may end there once
        // more), before the selection that closes it.  Two conventions, kept as they are:
        //   rows (selected or not)   the non-SEL instance over bank tile T_tail = R / BT itself: its masked constants are all it needs
        //   tokens, selected         the SEL instance over the list's own last position, n_live - 1 = T, which holds T_tail
        if (p->has_tail && t1 == T && !tail_done) {
            tail_done = true, s.tail = 1, s.tail_sel = !rows && sel, s.tail_pos = s.tail_sel ? T : p->T_tail;
        }
        s.final = t1 == T, t0 = t1;
    }
    return PF_OK;
}

}  // namespace pfplan
