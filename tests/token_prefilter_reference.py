"""numpy restatement of the IMAGE-level stage-1 test of the two-stage many-query patch-token search (csrc/topk_prefilter.hip,
"Patch-token banks"), the schedule that maintains its threshold, and the inputs of the bit-exact GPU cases (shared by
tests/test_token_prefilter_cpu.py and tests/test_token_prefilter_gpu.py).

Row test (exact arithmetic; the kernel's constants only add slack): row i passes for query q at threshold tau iff
    dot^ + eps_a ||q'|| nx_i >= tau (qn 2^-f xn_i + eps 2^-f)
or the row is unboundable.  Image test: every row passes ('min') / some row passes ('max').  dot^ comes from the row search's
restatements (prefilter_lp_reference / prefilter_bf16_reference: ``scale_query``, ``stage1_dots``, the flush models)."""
import functools
import itertools

import numpy as np
import torch

from tests import prefilter_bf16_reference as pbr
from tests import prefilter_lp_reference as plr
from tests import token_search_reference as tsr

BT, SCAP, QT = 256, 2048, {False: 256, True: 128}      # rows per tile, staged candidates per item, queries per tile (hi / hi + lo)


def list_cap(k):
    return 4096 if k <= 128 else 8192


def to16(x, dtype):
    """fp32 array -> (the 16-bit torch tensor, the fp32 array it widens to)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype)
    return t, t.float().numpy()


def flush_models(dtype):
    """Every combination of what the matrix core may flush: fp16 (query, rows), bf16 (query, rows, products)."""
    return list(itertools.product((False, True), repeat=2 if dtype == torch.float16 else 3))


def prepared(q, xw, w):
    """(tw [Q, D] fp32, qn [Q], xn [R]) of queries q against the widened rows xw [R, D] under weights w (None: ones)."""
    w64 = np.ones(q.shape[1]) if w is None else w.astype(np.float64)
    tw = (q.astype(np.float64) * w64).astype(np.float32)
    qn = np.sqrt((w64 * q.astype(np.float64) ** 2).sum(axis=1))
    with np.errstate(over="ignore", invalid="ignore"):
        xn = np.sqrt((w64 * xw.astype(np.float64) ** 2).sum(axis=1))
    return tw, qn, xn


def row_margins(q, xw, w, dtype, lo, flush, eps_a, eps=1e-6):
    """(lhs [Q, R], coef [Q, R], unboundable [R]): row i passes for query q at tau iff lhs >= tau * coef or it is unboundable."""
    ref = plr if dtype == torch.float16 else pbr
    tw, qn, xn = prepared(q, xw, w)
    R, D = xw.shape
    x64 = xw.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        norm = np.sqrt((x64 * x64).sum(axis=1)) * (1.0 + D * 2.0 ** -22)
        if dtype == torch.float16:
            import sky_embeddings_amd.ops as ops
            nsub = plr.count_subnormals(xw.astype(np.float16))
            nx = norm + np.sqrt(nsub) * 2.0 ** -14 / ops.topk_prefilter_eps_a_resident(D, torch.float16, lo=True)
            ub = ~np.isfinite(x64).all(axis=1)
        else:
            nx = norm
            ub = pbr.unboundable(xw) | ~np.isfinite(xn)
    lhs = np.empty((q.shape[0], R))
    coef = np.empty((q.shape[0], R))
    xs = np.where(ub[:, None], 0.0, xw).astype(np.float32)          # (their dot^ is not looked at)
    for i in range(q.shape[0]):
        qp, qh, ql, s = ref.scale_query(tw[i])
        x16 = xs.astype(np.float16) if dtype == torch.float16 else xs
        dots = ref.stage1_dots(qh, ql, x16, lo, *flush)
        nq = np.sqrt((qp.astype(np.float64) ** 2).sum())
        lhs[i] = dots + eps_a * nq * np.where(ub, 0.0, nx)
        coef[i] = qn[i] * s * np.where(ub, 0.0, xn) + eps * s
    return lhs, coef, ub


def image_pass(lhs, coef, ub, tau, P, combine):
    """[Q, N] bool: the image test at per-query thresholds tau [Q]."""
    with np.errstate(invalid="ignore"):
        rows = (lhs >= tau[:, None] * coef) | ub[None, :]
    rows = rows.reshape(rows.shape[0], -1, P)
    return rows.all(axis=2) if combine == "min" else rows.any(axis=2)


def bootstrap_images(N, k):
    """The strided sample of whole images whose k-th best combined score is the first threshold."""
    S = min(N, max(16 * k, 256))
    return np.arange(S) * (N // S)


def slices(R, P, k):
    """[(first row, end row, 'direct' | 'staged')] of the schedule: the slices of whole tiles; the tail rows ride with the last."""
    T = R // BT
    direct_end = max(min(-(-96 * k * P // BT), T), T // 128, 1)
    out, t0, first = [], 0, True
    for t1 in (direct_end, T // 32, T // 8, T // 2, T):
        if t1 <= t0:
            continue
        out.append((t0 * BT, R if t1 == T else t1 * BT, "direct" if first else "staged"))
        t0, first = t1, False
    return out


def kth_best(sc, k):
    """[Q] the k-th largest of every row of sc [Q, M] (-inf when M < k)."""
    if sc.shape[1] < k:
        return np.full(sc.shape[0], -np.inf, np.float32)
    return -np.partition(-sc, k - 1, axis=1)[:, k - 1]


def simulate(exact, lhs, coef, ub, P, k, combine, lo):
    """The search as the design runs it: tau from the bootstrap sample, then per slice the candidates at the running tau and the
    exact k-th best over the images decided so far.  -> (counts [phases, Q] candidates per query and slice, flagged [Q] bool:
    queries with a full list, or with a candidate in a staged (query tile x bank tile) item that holds more than SCAP)."""
    Q, N = exact.shape
    tau = kth_best(exact[:, bootstrap_images(N, k)], k)
    counts, flagged = [], np.zeros(Q, bool)
    for r0, r1, mode in slices(N * P, P, k):
        i0, i1 = r0 // P, r1 // P
        cand = np.zeros((Q, N), bool)
        cand[:, i0:i1] = image_pass(lhs[:, r0:r1], coef[:, r0:r1], ub[r0:r1], tau, P, combine)
        counts.append(cand.sum(axis=1))
        flagged |= counts[-1] > list_cap(k)
        if mode == "staged":
            whole = (r1 // BT) * BT                                    # (the tail tile appends directly)
            for t in range(r0 // BT, whole // BT):
                for qt in range(0, Q, QT[lo]):
                    item = cand[qt:qt + QT[lo], t * BT // P:(t + 1) * BT // P]
                    if item.sum() > SCAP:
                        flagged[qt:qt + QT[lo]] |= item.any(axis=1)
        tau = np.maximum(tau, kth_best(exact[:, :i1], k))
    return np.array(counts), flagged


# ---- the bit-exact GPU cases: (P, combine, dtype, lo) x shapes that meet every boundary ----------------------------------------------
def _shape(P, n):
    """The n-th shape at P tokens: (Q, tail rows, D, k, weighted, idx_offset).  N P = 2048 + tail rows, just above the route's
    minimum, with tails of 0, one image and 256 - P (255 at P = 1) rows; k <= N = 2048 / P + a few."""
    Q = (17, 130, 257)[n % 3]
    tail = (0, P, 256 - P if P > 1 else 255)[(n + P) % 3]
    N = (2048 + tail) // P
    k = [kk for kk in (1, 7, 100, 150) if kk <= N][(n + (P > 2)) % len([kk for kk in (1, 7, 100, 150) if kk <= N])]
    return Q, tail, 128, k, n % 2 == 0, (0, 1000003)[(n // 2) % 2]


def _grid():
    out, n = [], 0
    for combine in ("min", "max"):
        for P in (1, 2, 4, 8, 16, 32, 64):                             # every P once per combine
            out.append((P, combine, "f16", False) + _shape(P, n))
            n += 1
    for P in (4, 16, 64):                                              # every dtype and variant
        for dt, lo in (("f16", True), ("bf16", False), ("bf16", True)):
            for combine in ("min", "max"):
                out.append((P, combine, dt, lo) + _shape(P, n))
                n += 1
    Q, tail, _, k, weighted, off = _shape(16, n)
    out.append((16, "min", "f16", False, 130, 16, 768, 100, True, 7))  # one case at D = 768
    return out


CASES = _grid()
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def case_id(c):
    P, combine, dt, lo, Q, tail, D, k, weighted, off = c
    return f"P{P}-{combine}-{dt}-{'hilo' if lo else 'hi'}-Q{Q}-tail{tail}-D{D}-k{k}-{'w' if weighted else 'u'}-off{off}"


@functools.lru_cache(maxsize=None)
def case_inputs(P, tail, D, Q, weighted, dt):
    """(q fp32 [Q, D], bank 16-bit [N, P, D] torch, its widened fp32 array, w or None): images of very different scale whose
    tokens share a direction (so that images, not only tokens, differ), and planted exact ties between images."""
    N = (2048 + tail) // P
    rng = np.random.default_rng(P * 1000 + tail + D + Q)
    q = rng.standard_normal((Q, D), dtype=np.float32)
    centre = rng.standard_normal((N, 1, D))
    x = (centre + 0.7 * rng.standard_normal((N, P, D))) * rng.uniform(0.2, 5.0, size=(N, 1, 1))
    w = None
    if weighted:
        w = (1.0 / (rng.random(D, dtype=np.float32) + 0.05) ** 2).astype(np.float32)
        w /= w.sum()
    _, xw = to16(x, DTYPES[dt])
    for combine in ("min", "max"):                                     # exact ties: copies of query 0's best images
        best = np.argsort(-tsr.combined_scores(q[:1], xw, combine, w)[0])[:2]
        a, b = (N - 1, N // 2 + 1) if combine == "min" else (0, N // 3)
        if a not in best and b not in best:
            xw[a], xw[b] = xw[best[0]], xw[best[1]]
    bank, xw = to16(xw, DTYPES[dt])                                    # (already 16-bit values: exact)
    return q, bank, xw, w
