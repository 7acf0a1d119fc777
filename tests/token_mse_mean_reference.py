"""NumPy restatement of the two-stage weighted-MSE token search under combine 'mean' (csrc/topk_prefilter.hip, "Weighted MSE under
combine 'mean'"; include/skyemb.h, skyemb_distance_topk_tokens_mean_prefiltered): the pooled row, the row constants
{Bbar_dn 2^-e, R1, 2^-e, 0}, eps and gamma, the stage-1 test, and the contract's mean via token_mse_prefilter_reference's chain and
the token-order fold.  Used by tests/test_token_mse_mean_cpu.py and tests/test_token_mse_mean_gpu.py.

The pooled row is restated bit for bit (fp32 sum in token order, exact scales, one round-to-nearest-even).  Norms and Bbar are
taken in fp64, so a device constant may differ from them by the slack the kernels state, never beyond the fp64 value on the unsafe
side: the checkers below say which side that is."""
import numpy as np

from tests import token_mse_prefilter_reference as base

BT = 256
R_HI = 2.0 ** 60                      # R1 and R2 = 2^-e stay below it, or the image is unboundable
FLT_MAX = float(np.finfo(np.float32).max)


def eps_m(D, lo, dt):
    """eps_m of the pooled image (topk_prefilter.hip's eps_m_of), same order of summation."""
    if dt == "bf16":
        return (2.0 ** -9 + 2.0 ** -17 if lo else 2.0 ** -8 + 2.0 ** -17) + 6.06 * D * 2.0 ** -24 + D * 2.0 ** -37
    return (2.0 ** -11 + 2.0 ** -21 if lo else 2.0 ** -10 + 2.0 ** -21) + 6.06 * D * 2.0 ** -24 + 2.0 * np.sqrt(float(D)) * 2.0 ** -27


def eps(D, lo, dt):
    """eps_m + 2^-22 for fl(c o t)."""
    return eps_m(D, lo, dt) + 2.0 ** -22


def mean_roundings(P):
    """Rounded additions of the contract's mean fold: (((0 + d_0) + d_1) + ...) -- the first is exact; the division by P is too."""
    return P - 1


def gamma(D, P):
    """The token chain's gamma widened by the fold's roundings, as the kernel states it: (chain_roundings(D) + 3 + P) 2^-24."""
    return base.gamma(D) + P * 2.0 ** -24


def gamma_needed(D, P):
    """What any valid gamma must reach: (1 - 2^-24)^-(n + P - 1) - 1 in fp64 (n the token chain's roundings)."""
    n = base.chain_roundings(D) + mean_roundings(P)
    return float((1.0 - 2.0 ** -24) ** -n - 1.0)


def check_gamma(g, D, P):
    """True iff ``g`` pays for the token chain AND the mean fold."""
    return g >= gamma_needed(D, P)


def kappa(P):
    return 1.01 * P * 2.0 ** -24


def pooled_rows(x, dt):
    """x [N, P, D] fp32 (the widened bank) -> dict: pooled fp32 [N, D] (the values of the stored 16-bit row), s = 2^-e [N] fp32,
    R1_64 [N] the fp64 value the norm slot must reach, bad [N] bool: unboundable by the bank alone (pooled row zero)."""
    x = np.asarray(x, np.float32)
    N, P, D = x.shape
    mag = np.abs(x)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if dt == "bf16":
            bad = np.any(~(mag < 2.0 ** base.BF_ROW_HI) | ((mag > 0) & (mag < 2.0 ** -base.BF_ROW_LO)), axis=(1, 2))
        else:
            bad = np.any(~(mag < np.inf), axis=(1, 2))
        acc = np.zeros((N, D), np.float32)
        for p in range(P):                                  # token order, one fp32 rounding per addition
            acc = (acc + x[:, p]).astype(np.float32)
        m = (acc * np.float32(1.0 / P)).astype(np.float32)  # exact: a power of two
        mx = np.where(bad, 0.0, np.abs(np.where(np.isfinite(m), m, 0.0)).max(axis=1))
        e = np.zeros(N, np.int64)
        ok = mx > 0
        e[ok] = np.frexp(mx[ok])[1] - 14
        s = np.ldexp(np.float32(1.0), -e).astype(np.float32)
        a = (m * s[:, None]).astype(np.float32)             # exact
        if dt == "bf16":
            a = np.where(np.abs(a) < 2.0 ** -40, np.float32(0), a)
        x64 = np.where(np.isfinite(x), x, 0).astype(np.float64)
        ss = (x64 * x64).sum(axis=2)                        # [N, P]
        tok = np.where(ss >= FLT_MAX, np.inf, np.sqrt(ss))  # (the kernel's fp32 sum of squares overflows there)
        c1 = tok.mean(axis=1)
        a64 = (m.astype(np.float64) * s.astype(np.float64)[:, None])
        R1 = np.sqrt((np.where(bad[:, None], 0.0, a64) ** 2).sum(axis=1)) + kappa(P) / eps_m(D, True, dt) * c1 * s
        bad = bad | ~(R1 < R_HI) | ~(s < R_HI)
        pooled = np.where(bad[:, None], np.float32(0), base.to16(a, dt)).astype(np.float32)
        s = np.where(bad, np.float32(1), s).astype(np.float32)
    return dict(pooled=pooled, s=s, R1_64=np.where(bad, np.inf, R1), bad=bad)


def check_pooled(dev_pooled, x, dt):
    """True iff the device's pooled image (as fp32) equals the restatement bit for bit."""
    want = pooled_rows(x, dt)["pooled"]
    got = np.asarray(dev_pooled, np.float32)
    return got.shape == want.shape and bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))


LANES, PER_LANE = 64, 8               # the row-constants kernel: one wave per image, 8 consecutive elements per lane and load


def bbar_chain(P, D):
    """Roundings along the longest path of the kernel's fp32 sum of the P D terms c_d x_pd^2, counted from how the work is laid out:
    lane l takes elements [8 l + 512 s, 8 l + 512 s + 8) of every token row, s = 0, 1, ..., one fused multiply-add each into ONE
    accumulator, tokens in order; then a butterfly over the 64 lanes, log2(64) additions.  The busiest lane is lane 0."""
    per_row = sum(1 for d in range(D) if (d % (LANES * PER_LANE)) // PER_LANE == 0)      # elements of one row that lane 0 adds
    return P * per_row + int(np.log2(LANES))


def bbar_slack_needed(P, D):
    """What any valid lowering must reach: non-negative terms, each rounding moves a partial sum by at most 2^-24 relative, so
    the fp32 sum is below the real one times (1 + 2^-24)^n; + one rounding for the lowering's own product."""
    return float((1.0 + 2.0 ** -24) ** (bbar_chain(P, D) + 1) - 1.0)


def bbar_slack(P, D):
    """The relative amount the kernel lowers Bbar^ by, as it states it: (n_B + 8) 2^-23, n_B = 8 P ceil(D / 512)."""
    return (8 * P * ((D + 511) // 512) + 8) * 2.0 ** -23


def bbar_kernel_order(c, x):
    """Bbar^ [N] fp32 as the kernel's layout sums it (bbar_chain): per lane one fused multiply-add per element -- c_d x_pd^2 is exact
    in fp64 for 16-bit x, so ``float32(float64 sum)`` is the fma's single rounding --, a butterfly over the lanes, the exact scale."""
    c64, x = np.asarray(c, np.float32).astype(np.float64), np.asarray(x, np.float32)
    N, P, D = x.shape
    acc = np.zeros((N, LANES), np.float32)
    for p in range(P):
        for d in range(D):
            lane = (d % (LANES * PER_LANE)) // PER_LANE
            acc[:, lane] = (acc[:, lane].astype(np.float64) + c64[d] * x[:, p, d].astype(np.float64) ** 2).astype(np.float32)
    o = LANES // 2
    j = np.arange(LANES)
    while o:
        acc = (acc + acc[:, j ^ o]).astype(np.float32)
        o //= 2
    return (acc[:, 0] * np.float32(1.0 / P)).astype(np.float32)


def check_bbar_slack(slack, P, D):
    """True iff lowering Bbar^ by ``slack`` (relative) keeps it at or below the real Bbar whatever the terms are."""
    return slack >= bbar_slack_needed(P, D)


def row_constants(c, x, dt):
    """-> dict: Bbar64 [N], Bbar_dn [N] (fp64 sum rounded to fp32, lowered as the kernel lowers it), R1_64, s, unboundable [N]."""
    pr = pooled_rows(x, dt)
    x = np.asarray(x, np.float32)
    N, P, D = x.shape
    c64 = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        x64 = x.astype(np.float64)
        Bbar = (c64 * x64 * x64).sum(axis=(1, 2)) / P
        B32 = Bbar.astype(np.float32).astype(np.float64)
        Bdn = np.where(Bbar < 2.0 ** -100, 0.0, B32 * (1.0 - bbar_slack(P, D)))
        hi = 2.0 ** base.MSE_B_HI[dt]
        r0 = Bdn * pr["s"].astype(np.float64)
        ub = pr["bad"] | ~((Bbar >= 0) & (Bbar < hi)) | ~(r0 < hi)
    return dict(Bbar64=Bbar, Bbar_dn=Bdn, R1_64=pr["R1_64"], s=pr["s"], unboundable=ub, pooled=pr["pooled"])


def check_rowp(dev_rowp, c, x, dt):
    """True iff every image's device constants {R0, R1, R2, 0} lie on the safe side of the fp64 values and within the stated slack:
    R0 <= Bbar 2^-e (never raised) and >= Bbar (1 - 2 slack) 2^-e, R1 >= the fp64 norm slot and <= it (1 + 2^-9), R2 == 2^-e;
    an unboundable image holds {0, inf, 1, 0}."""
    rc = row_constants(c, x, dt)
    N, P, D = np.asarray(x).shape
    r = np.asarray(dev_rowp, np.float64)[:N]
    ub = rc["unboundable"]
    ok_ub = (r[:, 0] == 0) & np.isposinf(r[:, 1]) & (r[:, 2] == 1) & (r[:, 3] == 0)
    s = rc["s"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        top = rc["Bbar64"] * s
        ok = (r[:, 0] <= top) & (r[:, 0] >= top * (1.0 - 2.0 * bbar_slack(P, D)) - 2.0 ** -126)
        ok &= (r[:, 1] >= rc["R1_64"]) & (r[:, 1] <= rc["R1_64"] * (1.0 + 2.0 ** -9) + 2.0 ** -126)
        ok &= (r[:, 2] == s) & (r[:, 3] == 0)
    return bool(np.all(np.where(ub, ok_ub, ok)))


def query_constants(c, t, dt, lo):
    """token_mse_prefilter_reference.query_constants with this route's eps in the query's error slot."""
    qc = base.query_constants(c, t, dt, lo)
    D = np.asarray(t).shape[1]
    qc = dict(qc)
    qc["cq"] = qc["cq"] / base.eps_mse(D, lo, dt) * eps(D, lo, dt)
    qc["flagged"] = qc["flagged"] | ~((qc["cq"] > 0) & (qc["cq"] < 2.0 ** 60))
    return qc


def lower_bounds(c, t, x, dt, lo, dot=None, rowp=None):
    """-> (L [Q, N] fp64, trusted [Q, N] bool, dot [Q, N]): L <= D x the real mean distance for every trusted pair.  ``dot``: stage
    1's dot^ (default: the exact sum of the 16-bit operands' products rounded to fp32); ``rowp``: the device's row constants
    (default: the restatement's, R1 raised by its slack)."""
    qc = query_constants(c, t, dt, lo)
    rc = row_constants(c, x, dt)
    s = rc["s"].astype(np.float64)
    if rowp is None:
        R0, R1 = rc["Bbar_dn"] * s, rc["R1_64"] * (1.0 + 2.0 ** -10)
    else:
        R0, R1 = np.asarray(rowp, np.float64)[:len(s), 0], np.asarray(rowp, np.float64)[:len(s), 1]
    with np.errstate(invalid="ignore", over="ignore"):
        if dot is None:
            dot = ((qc["qh"].astype(np.float64) + qc["ql"].astype(np.float64)) @ rc["pooled"].astype(np.float64).T)
            dot = dot.astype(np.float32).astype(np.float64)
        inv_q, inv_s = (1.0 / qc["s"])[:, None], (1.0 / s)[None, :]
        L = qc["A_dn"][:, None] + (R0 * inv_s[0])[None, :] - 2.0 * inv_q * inv_s * (dot + qc["cq"][:, None] * R1[None, :])
    return L, ~qc["flagged"][:, None] & ~rc["unboundable"][None, :], dot


def stage1_pass(L, theta, D, P, g=None):
    """The candidate test: L <= D theta (1 + gamma) + 2^-126 (theta [Q] the distance thresholds)."""
    g = gamma(D, P) if g is None else g
    return L <= (np.asarray(theta, np.float64) * D * (1.0 + g) + 2.0 ** -126)[:, None]


def contract_mean(c, t, x):
    """-> [Q, N] fp32: the contract's mean distance of every image -- the token distances by the contract's chain, then in KEY space
    (key = -dist, a NaN distance is key -inf) (((0 + k_0) + k_1) + ...) / float32(P) in token order, a sum that is not a number is
    key -inf; returned as distances (+inf for such an image)."""
    x = np.asarray(x, np.float32)
    N, P, D = x.shape
    d = base.contract_distances(c, t, x.reshape(N * P, D)).reshape(-1, N, P)
    with np.errstate(invalid="ignore", over="ignore"):
        key = np.where(d == d, -d, np.float32(-np.inf)).astype(np.float32)
        acc = np.zeros(key.shape[:2], np.float32)
        for p in range(P):
            acc = (acc + key[:, :, p]).astype(np.float32)
        k = (acc / np.float32(P)).astype(np.float32)
        k = np.where(k == k, k, np.float32(-np.inf))
    return (-k).astype(np.float32)


def topk(dist, k, idx_offset=0):
    """(distances [Q, k] ascending, indices) in the order (distance asc, image asc); an image at +inf is never returned: (+inf, -1)."""
    Q, N = dist.shape
    out_d = np.full((Q, k), np.inf, np.float32)
    out_i = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        order = np.lexsort((np.arange(N), dist[q]))
        order = order[np.isfinite(dist[q][order]) | (dist[q][order] == -np.inf)][:k]
        out_d[q, :len(order)] = dist[q][order]
        out_i[q, :len(order)] = order + idx_offset
    return out_d, out_i
