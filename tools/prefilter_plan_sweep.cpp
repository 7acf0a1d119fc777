// Stand-alone sweep of sky_prefilter_plan (csrc/prefilter_plan.h) for a sanitizer build of HOST code only -- the header makes no HIP call:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Isky_embeddings_amd/csrc \
//       tools/prefilter_plan_sweep.cpp -o /tmp/prefilter_plan_sweep && /tmp/prefilter_plan_sweep
// Every combination below is planned or refused; a plan's slices must tile [0, T) in order, end in a final one and carry a tail launch
// only where the plan says a tail exists.  Refused requests (bad kinds, banks, shapes, selections) are part of the sweep.
#include "prefilter_plan.h"

#include <initializer_list>
#include <stdio.h>

int main() {
    long plans = 0, refused = 0, slices = 0;
    const int64_t Ns[] = {0, 64, 511, 1024, 1027, 2047, 2048, 2092, 2304, 2404, 2560, 2597, 4096, 8193, 81920, 81927, (1ll << 31) - 1, 1ll << 31, 1ll << 40};
    for (int kind = -1; kind <= 3; ++kind)
    for (int bank = -1; bank <= 3; ++bank)
    for (int64_t N : Ns)
    for (int k : {0, 5, 128, 129, 193, 257})
    for (int P : {0, 1, 3, 4, 64, 128})
    for (int lo = -1; lo <= 3; ++lo)
    for (int thr0 = 0; thr0 <= 1; ++thr0)
    for (int Q : {0, 17, 257, 600000})
    for (int D : {96, 128, 4096})
    for (int combine = 0; combine <= 3; ++combine)
    for (int top_t : {-1, 0, 1, 2, 4, 17}) {
        if (kind != SKYEMB_PF_TOKENS && (top_t > 0 || combine == 3 || P > 4) && N != 4096) continue;      // fields the route does not read
        for (int sel = 0; sel <= 1; ++sel) {
            const int64_t R = kind == SKYEMB_PF_TOKENS && P > 0 && N < (1ll << 33) ? N * P : N;
            const int tiles = (int)((R + 255) / 256 > 100000 ? 100000 : (R + 255) / 256);
            for (int n_live : {sel ? -1 : 0, 0, 1, tiles / 2, tiles, tiles + 1})
            for (int last = sel ? -1 : 0; last <= (sel ? 2 : 0); ++last)
            for (int direct : {sel ? -3 : 0, 0, 1, n_live, n_live + 1}) {
                if (!sel && (n_live != 0 || direct != 0)) continue;
                const skyemb_prefilter_request_t r = {kind, bank, Q, P, D, k, N, combine, top_t, thr0, sel, n_live, last, direct, lo,
                                                      (lo & 1) ? 1e-6f : -1.f};
                skyemb_prefilter_plan_t p;
                if (pfplan::sky_prefilter_plan(r, &p) != pfplan::PF_OK) {
                    ++refused;
                    continue;
                }
                ++plans;
                if (p.n_slices < 1 || p.n_slices > SKYEMB_PF_MAX_SLICES) return printf("n_slices = %d\n", p.n_slices), 1;
                int t0 = 0;
                for (int i = 0; i < p.n_slices; ++i, ++slices) {
                    const skyemb_prefilter_slice_t &s = p.slice[i];
                    if (s.t0 != t0 || s.t1 < s.t0 || s.t1 > p.T || s.mode < 0 || s.mode > 2 || (s.tail && !p.has_tail)) return printf("a bad slice\n"), 1;
                    t0 = s.t1;
                }
                if (t0 != p.T || !p.slice[p.n_slices - 1].final) return printf("the slices do not end at T\n"), 1;
            }
        }
    }
    printf("%ld plans, %ld refusals, %ld slices: clean\n", plans, refused, slices);
    return 0;
}
