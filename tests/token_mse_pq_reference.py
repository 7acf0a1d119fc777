"""NumPy restatement of the two-stage weighted-MSE token search with PER-QUERY weights (csrc/topk_prefilter.hip, "Weighted MSE with
PER-QUERY weights"; include/skyemb.h, skyemb_distance_topk_tokens_prefiltered_pq): the second image [x ; r16(x o x)] of the bank and
its row constants {0, ny, 1, 0}, the query images of u_q = [c_q o t_q ; -c_q / 2] and their constants {A_dn, eps_pq ||u'||, 2^-f,
flag}, eps_pq, the row test, and the contract distance under per-query c in the contract's summation order.  Used by
tests/test_token_mse_pq_cpu.py (soundness of the bound) and tests/test_token_mse_pq_gpu.py (the image and constants read back).

Sums are taken in fp64 and then lowered / raised by the slack the kernels state, as tests/token_mse_prefilter_reference.py does."""
import numpy as np

from tests import token_mse_prefilter_reference as mpr

# the unit roundoff of one round-to-nearest-even: fp16 has 11 significant bits, bf16 8 (tests/test_token_mse_pq_cpu.py measures both
# on the formats themselves)
RHO = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
SQ_LO, SQ_HI = 2.0 ** -mpr.BF_ROW_LO, 2.0 ** mpr.BF_ROW_HI      # bf16: the window of a nonzero element's stored square


def kappa(lo, dt):
    """bf16: what the query split's own roundings cost at the unit roundoff 2^-8 beyond the 2^-9 (hi only) / 2^-18 (hi + lo) that the
    resident eps_a prices them at; fp16: nothing."""
    if dt != "bf16":
        return 0.0
    return 2.0 ** -16 - 2.0 ** -18 if lo else 2.0 ** -9


def eps_pq(D, lo, dt):
    """topk_prefilter.hip's eps_pq_of, same order of summation: eps_a at 2 D, the rounding of the squares, fl(c o t); bf16: kappa."""
    rho = RHO[dt]
    eps = mpr.eps_a_resident(2 * D, lo, dt) + rho * (1.0 + rho) + 2.0 ** -22
    return eps + kappa(lo, dt) if dt == "bf16" else eps


def image(x, dt):
    """-> (y [R, 2 D] fp32: the stored image rows widened, unboundable rows zero; unboundable [R] bool) for widened 16-bit rows x."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        sq = mpr.to16((x * x).astype(np.float32), dt)
        mag = np.abs(x)
        if dt == "f16":
            bad = np.any(~(mag < 2.0 ** 8), axis=1)
        else:
            bad = np.any((x != 0) & ~((sq >= SQ_LO) & (sq < SQ_HI)), axis=1)
    y = np.concatenate([x, sq], axis=1)
    y[bad] = 0.0
    return y, bad


def row_constants(x, dt):
    """-> (ny64 [R]: the fp64 value the norm slot must reach, unboundable [R] bool)."""
    y, bad = image(x, dt)
    D = x.shape[1]
    y64, mag = y.astype(np.float64), np.abs(np.asarray(x, np.float32).astype(np.float64))
    ny = np.sqrt((y64 * y64).sum(axis=1))
    if dt == "f16":
        nsub = ((np.abs(y64) > 0) & (np.abs(y64) < 2.0 ** -14)).sum(axis=1)
        nsq = ((mag > 0) & (mag < 2.0 ** -7)).sum(axis=1)
        ny = ny + (np.sqrt(nsub) * 2.0 ** -14 + np.sqrt(nsq) * 2.0 ** -25) / eps_pq(D, True, "f16")
    return np.where(bad, np.inf, ny), bad


def query_constants(c, t, dt, lo):
    """c, t [Q, D] -> dict: u fp32 [Q, 2 D]; s = 2^-f; qh, ql (the 16-bit operands as fp32, ql zero without lo); A64, A_dn;
    cq = eps_pq ||u'|| (raised as the kernel raises it); flagged [Q] bool."""
    c32, t32 = np.asarray(c, np.float32), np.asarray(t, np.float32)
    Q, D = t32.shape
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        tw = (c32 * t32).astype(np.float32)
        u = np.concatenate([tw, (np.float32(-0.5) * c32).astype(np.float32)], axis=1)
        mw = np.nanmax(np.abs(tw), axis=1, initial=0.0)
        mx = np.nanmax(np.abs(u), axis=1, initial=0.0)
        e = np.zeros(Q, np.int64)
        ok = (mx > 0) & np.isfinite(mx)
        e[ok] = np.frexp(mx[ok])[1] - (mpr.BF_QMAX_EXP if dt == "bf16" else 14)
        e = np.maximum(e, -126)
        if dt == "bf16":
            e = np.minimum(e, mpr.BF_SCALE_LO)
        s = np.ldexp(np.float32(1.0), -e).astype(np.float32)
        qp = (u * s[:, None]).astype(np.float32)
        qh = mpr.to16(qp, dt)
        ql = mpr.to16((qp - qh).astype(np.float32), dt) if lo else np.zeros_like(qh)
        A64 = (c32.astype(np.float64) * t32.astype(np.float64) ** 2).sum(axis=1)
        A32 = A64.astype(np.float32).astype(np.float64)
        A_dn = np.where(~(A64 >= 2.0 ** -100), 0.0, A32 * (1.0 - D * 2.0 ** -22))
        nq = np.sqrt((qp.astype(np.float64) ** 2).sum(axis=1)) * (1.0 + 2 * D * 2.0 ** -22)
        cq = eps_pq(D, lo, dt) * (1.0 + 1e-6) * nq
        lo_s, hi_s = (2.0 ** -mpr.BF_SCALE_LO, 2.0 ** mpr.BF_SCALE_HI) if dt == "bf16" else (0.0, 2.0 ** mpr.MSE_SCALE_HI_F16)
        cbad = np.any(~((c32 >= 0) & (c32 <= mpr.C_MAX)), axis=1)                 # the query's OWN row only
        flagged = cbad | ~(mw > 0) | ~np.isfinite(A32) | (s >= hi_s) | (s <= lo_s) | ~((cq > 0) & (cq < 2.0 ** 60))
    return dict(u=u, s=s.astype(np.float64), qh=qh, ql=ql, A64=A64, A_dn=A_dn, cq=cq, flagged=flagged)


def row_test(dot, qc, ny, D, theta):
    """mse_test_row + the instruction of prefilter_kernel with B = 0: [Q, R] bool, True = the pair is a candidate under the distance
    thresholds theta [Q].  dot [Q, R]: stage 1's dot products; qc: ``query_constants``; ny [R]: the norm slots."""
    with np.errstate(invalid="ignore", over="ignore"):
        T = np.asarray(theta, np.float64) * D
        T = T + np.abs(T) * (mpr.gamma(D) * (1.0 + 1e-6)) + 2.0 ** -126
        h = 0.5 * qc["s"]
        g = h * (T - qc["A_dn"])
        g = g + np.abs(g) * 2.0 ** -19
        cr = qc["cq"] * (1.0 + 2.0 ** -19)
        return dot + cr[:, None] * np.asarray(ny, np.float64)[None, :] + g[:, None] >= 0


def contract_distances(c, t, x):
    """[Q, R] fp32 MSE distances by the contract's chain, query q under its own row of c [Q, D]."""
    c, t = np.asarray(c, np.float32), np.asarray(t, np.float32)
    return np.concatenate([mpr.contract_distances(c[q], t[q:q + 1], x) for q in range(t.shape[0])], axis=0)
