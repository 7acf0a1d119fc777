#!/usr/bin/env python3
"""Per-query feature weights in the patch-token bank search: what one pass for 16 targets costs.  Run by hand on an MI355X:

    python tools/bench_token_pq.py [--out profiles/r14_token_pq.json]

16 targets with 16 different weight vectors over a [65536, 16, 768] token bank (1 M / 16 images), fp32 and fp16, k = 100, the
cosine metric (combine min) and MAE (combine mean), each timed three ways:
  (a) the single call with ``weights`` [16, D];
  (b) the route without per-query weights: 16 x (TokenBank.set_weights + a Q = 1 search) for cosine -- a norm pass and a search
      pass per target -- and 16 x a Q = 1 search with that target's weights for MAE.  The baseline;
  (c) the Q = 16 call with ONE shared weight vector: the same bytes and, for cosine, half the MFMA work -- a lower bound.
One process, warm-up first, the three legs interleaved within every repetition, device time from events, the median reported.
Those figures are end to end (query preparation, pass, merge, and the host's launch gaps).  Next to them the list kernels of
(a) and (c) are timed ALONE -- queries prepared, outputs allocated, ten launches back to back between two events -- which is
what says whether the second MFMA chain costs anything per bank byte (``kernel_*`` fields).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sky_embeddings_amd import ops, search  # noqa: E402

N, P, D, Q, K = 65536, 16, 768, 16, 100


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r14_token_pq.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(Q, D, device="cuda", generator=g)
    W = (torch.rand(Q, D, device="cuda", generator=g) + 0.05) * torch.randn(Q, D, device="cuda", generator=g).exp()
    results = []
    for dtype in (torch.float32, torch.float16):
        bank = torch.empty(N, P, D, device="cuda", dtype=dtype)
        for lo in range(0, N, 4096):
            bank[lo:lo + 4096] = torch.randn(4096, P, D, device="cuda", generator=g).to(dtype)
        tb = search.TokenBank(bank, W[0])               # (c)'s bank: norms under the one shared vector, computed once
        tb_b = search.TokenBank(bank, W[0])             # (b)'s bank: its norms are recomputed for every target
        nbytes = bank.numel() * bank.element_size()

        def cos_a():
            return search.cosine_topk_tokens(q, bank, K, "min", weights=W)

        def cos_b():
            out = []
            for i in range(Q):
                tb_b.set_weights(W[i])
                out.append(search.cosine_topk_tokens(q[i:i + 1], tb_b, K, "min"))
            return out

        def cos_c():
            return search.cosine_topk_tokens(q, tb, K, "min")

        def mae_a():
            return search.distance_topk_tokens(q, bank, K, "MAE", "mean", weights=W)

        def mae_b():
            return [search.distance_topk_tokens(q[i:i + 1], bank, K, "MAE", "mean", weights=W[i]) for i in range(Q)]

        def mae_c():
            return search.distance_topk_tokens(q, bank, K, "MAE", "mean", weights=W[0])

        # the list kernels alone: everything they need prepared once
        tw_a, qn_a = search.prepare_queries_pq(q, W)
        tw_c, qn_c = search.prepare_queries(q, W[0])
        c_a, c_c = search.prepare_distance_weights(W, D, bank.device), search.prepare_distance_weights(W[0], D, bank.device)
        nl = ops.cosine_token_topk_chunks(N, P, Q, D, K)
        ps, pi = torch.empty(Q, nl, K, device="cuda"), torch.empty(Q, nl, K, device="cuda", dtype=torch.int64)
        cmin, cmean, mae = ops.COMBINE_CODES["min"], ops.COMBINE_CODES["mean"], ops.METRIC_CODES["MAE"]
        kernels = {"cosine": (lambda: ops.cosine_token_topk_pq(tw_a, qn_a, bank, W, K, cmin, 1e-6, 0, nl, ps, pi),
                              lambda: ops.cosine_token_topk(tw_c, qn_c, bank, tb.norms, K, cmin, 1e-6, 0, nl, ps, pi)),
                   "MAE": (lambda: ops.distance_token_topk_pq(c_a, q, bank, mae, cmean, K, 0, nl, ps, pi),
                           lambda: ops.distance_token_topk(c_c, q, bank, mae, cmean, K, 0, nl, ps, pi))}

        def ten(fn):
            return lambda: [fn() for _ in range(10)]

        for metric, legs in (("cosine", (cos_a, cos_b, cos_c)), ("MAE", (mae_a, mae_b, mae_c))):
            # (a) is (b), target by target: bit for bit for MAE; for cosine within gamma(2 D + 9), the two bank-norm chains'
            # distance (tests/token_pq_reference.py) -- the shared-weights search is not bit-equal to per-query weights
            got_a, got_b = legs[0](), legs[1]()
            u = 2.0 ** -24
            tol = (2 * D + 9) * u / (1 - (2 * D + 9) * u) if metric == "cosine" else 0.0
            for i in range(Q):
                assert float((got_a[0][i] - got_b[i][0][0]).abs().max()) <= tol, (metric, i)
                assert metric == "cosine" or torch.equal(got_a[1][i], got_b[i][1][0]), (metric, i)
            times = ([], [], [])
            for rep in range(args.warmup + args.reps):
                for j, leg in enumerate(legs):
                    ms = timed(leg)
                    if rep >= args.warmup:
                        times[j].append(ms)
            a, b, c = (statistics.median(t) for t in times)
            ktimes = ([], [])
            for rep in range(args.warmup + args.reps):
                for j, kern in enumerate(kernels[metric]):
                    ms = timed(ten(kern)) / 10
                    if rep >= args.warmup:
                        ktimes[j].append(ms)
            ka, kc = (statistics.median(t) for t in ktimes)
            row = dict(metric=metric, bank_dtype=str(dtype)[6:], N=N, P=P, D=D, Q=Q, k=K, bank_bytes=nbytes, reps=args.reps,
                       a_single_call_ms=round(a, 3), b_sixteen_single_target_searches_ms=round(b, 3), c_shared_weights_q16_ms=round(c, 3),
                       a_over_c=round(a / c, 3), b_over_a=round(b / a, 2), a_bank_bytes_per_s=round(nbytes / (a * 1e-3), 0),
                       a_all_ms=[round(t, 3) for t in times[0]], kernel_a_ms=round(ka, 4), kernel_c_ms=round(kc, 4),
                       kernel_a_over_c=round(ka / kc, 3), kernel_a_bank_bytes_per_s=round(nbytes / (ka * 1e-3), 0),
                       kernel_c_bank_bytes_per_s=round(nbytes / (kc * 1e-3), 0))
            print(json.dumps(row))
            results.append(row)
        del bank, tb, tb_b
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/bench_token_pq.py", device=torch.cuda.get_device_name(0), results=results), f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
