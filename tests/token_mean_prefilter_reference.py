"""NumPy statement of stage 1 of the two-stage token search under combine 'mean' (csrc/topk_prefilter.hip, "combine 'mean'"):
the pooled row and its constants (token_mean_pool_kernel), the query's test parameters (mean_test_row), dot^ and the bound U.

Notation (per image, tokens p = 0 .. P-1; x_p the widened rows, n_p their weighted norms xn):
  u_p = x_p / n_p      m = (1/P) sum_p u_p      c1 = mean_p ||u_p||_2      c2 = mean_p ||u_p||_2 / n_p
  m_fl   the kernel's fp32 value: fl(fl(sum_p fl(x_p / n_p)) / P), p ascending -- restated here bit for bit
  m'     m_fl 2^-e, largest element in [2^13, 2^14), rounded to the bank's 16-bit format (bf16: |m'| < 2^-40 stored as zero)
  rowp = {R0, R1, R2, 0} = {2^-e, ||m'||_2 + (kappa / eps_m) c1 2^-e, c2 2^-e, 0}, norms and constants rounded up
  qpar = {-a, c, g, 0}: a = tau qn 2^-f (lowered), c = eps_m ||q'|| (raised), g = ||q'|| eps / qn (raised)
  U    = (dot^ + c R1 + g R2) / (R0 qn 2^-f)        and the pair is a candidate iff dot^ - a R0 + c R1 + g R2 >= 0.
The derivation (points (a) .. (e) of the design) is in the kernel file; the claim tested here is  contract mean <= U  for every
boundable image and every query stage 1 accepts, the contract mean being tests.token_search_reference's.

Looseness.  Under unit weights c1 = 1 and U - mean is eps_m ||m|| + kappa + (rounding slack) in cosine units: the median over
random banks is held to 4 eps_m by tests/test_token_mean_prefilter_cpu.py (measured there: 0.13 .. 0.56 eps_m for random tokens,
whose pooled row is short, ||m|| ~ 1 / sqrt(P); 1.0 eps_m for images of near-parallel tokens).
"""
import math

import numpy as np

from tests import prefilter_stage1_reference as sr

U32 = 2.0 ** -24
INF = float("inf")
N_LO, N_HI = 2.0 ** -40, 2.0 ** 40          # window of a token norm
U_LO, U_HI = 2.0 ** -20, 2.0 ** 20          # window of ||u_p||
BF_LO, BF_HI = 2.0 ** -60, 2.0 ** 120       # window of a nonzero bf16 element (the resident route's (R))
R_MAX = 2.0 ** 60                           # R1, R2, c, g stay below
QN_LO, QN_HI = 2.0 ** -20, 2.0 ** 20
SC_LO, SC_HI = 2.0 ** -34, 2.0 ** 34


def eps_m(fmt, D, lo):
    """eps_m_of of the kernel file, restated (the CPU test holds it to the library's value)."""
    if fmt == "bf16":
        return (2.0 ** -9 + 2.0 ** -17 if lo else 2.0 ** -8 + 2.0 ** -17) + 6.06 * D * 2.0 ** -24 + D * 2.0 ** -37
    return sr.eps_a("fp32", D, lo)          # the fp32 bank's fp16 image: the pooled row is exactly that


def kappa(D, P):
    return (1.02 * D + 2.03 * P + 4.0) * 2.0 ** -24


def error_c(P):
    """Term (c): ||m_fl - m||_2 <= error_c(P) c1."""
    return 1.01 * P * 2.0 ** -24


def round16(a, fmt):
    """Round-to-nearest-even of float32 values to the 16-bit format, as float32 values."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if fmt == "fp16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def pool(x, xn, fmt):
    """x [N, P, D] float32 (the widened bank), xn [N * P] float32 -> dict:
    m_fl [N, D] f32 (bit for bit the kernel's), e [N], m16 [N, D] f32 (values of the stored row), unboundable [N] bool,
    c1, c2 [N] float64 (exact from the fp32 u_p), nrm [N] float64 (||m_fl 2^-e||), and the least / largest constants the derivation
    accepts: R1_lo / R1_hi, R2_lo / R2_hi (float64)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    N, P, D = x.shape
    n = np.asarray(xn, dtype=np.float32).reshape(N, P)
    with np.errstate(all="ignore"):
        n_ok = (n >= N_LO) & (n <= N_HI)
        nn = np.where(n_ok, n, np.float32(1.0)).astype(np.float32)
        u = (x / nn[:, :, None]).astype(np.float32)                     # IEEE division, one rounding
        acc = np.zeros((N, D), np.float32)
        for p in range(P):
            acc = (acc + u[:, p]).astype(np.float32)
        m_fl = (acc * np.float32(1.0 / P)).astype(np.float32)
        mag = np.abs(x)
        elem_bad = ~np.isfinite(x)
        if fmt == "bf16":
            elem_bad |= ~(mag < BF_HI) | ((mag > 0) & (mag < BF_LO))
        nu = np.sqrt((u.astype(np.float64) ** 2).sum(axis=2))           # [N, P]
        c1 = nu.mean(axis=1)
        c2 = (nu / nn.astype(np.float64)).mean(axis=1)
        mx = np.abs(m_fl).max(axis=1)
        bad = elem_bad.any(axis=(1, 2)) | ~n_ok.all(axis=1) | ~((nu >= U_LO) & (nu <= U_HI)).all(axis=1)
        bad |= ~np.isfinite(mx) | ((mx > 0) & (mx < 2.0 ** -40))
        # images within a factor 1 +- 2^-10 of a window's edge may fall on either side in the kernel (its norms are fp32): `edge`
        edge = ((np.abs(np.log2(np.where(nu > 0, nu, 1.0))) > 19.99) & (np.abs(np.log2(np.where(nu > 0, nu, 1.0))) < 20.01)).any(axis=1)
    e = np.zeros(N, np.int64)
    ok = ~bad & (mx > 0)
    e[ok] = np.frexp(mx[ok])[1] - 14
    s = np.ldexp(1.0, -e)
    with np.errstate(all="ignore"):
        ms = (m_fl.astype(np.float64) * s[:, None]).astype(np.float32)  # exact (powers of two; no subnormals inside the windows)
        if fmt == "bf16":
            ms = np.where(np.abs(ms) < 2.0 ** -40, np.float32(0), ms)
        m16 = round16(ms, fmt)
        nrm = np.sqrt((m_fl.astype(np.float64) ** 2).sum(axis=1)) * s
    m16[bad] = 0
    kf = kappa(D, P) / eps_m(fmt, D, True)
    R1_lo = nrm + kf * c1 * s
    R2_lo = c2 * s
    slack = (1 + (D + 64) * 2.0 ** -22) * (1 + 2.0 ** -19) ** 2 * (1 + 2e-6)
    bad |= ~(R1_lo * slack < R_MAX) | ~(R2_lo * slack < R_MAX)
    return dict(N=N, P=P, D=D, fmt=fmt, m_fl=m_fl, e=e, s=s, m16=m16, unboundable=bad, edge=edge, c1=c1, c2=c2, nrm=nrm,
                R1_lo=R1_lo, R1_hi=R1_lo * slack, R2_lo=R2_lo, R2_hi=R2_lo * slack)


def model_rowp(ref, rows_padded=None):
    """rowp [rows_padded, 4] float32 as a device that rounds every constant UP to the next float would leave it."""
    N = ref["N"]
    rows = N if rows_padded is None else rows_padded
    out = np.zeros((rows, 4), np.float32)
    out[N:] = (0, np.nan, 0, 0)

    def up(v):
        f = v.astype(np.float32)
        return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(INF)), f)
    out[:N, 0] = ref["s"]
    out[:N, 1] = up(ref["R1_lo"] * (1 + 2.0 ** -22))
    out[:N, 2] = up(ref["R2_lo"] * (1 + 2.0 ** -22))
    out[:N][ref["unboundable"]] = (0, INF, 1, 0)
    return out


def check_pool(pooled_bits, rowp, ref):
    """The device's pooled image (uint16 patterns [N, D]) and constants [>= N, 4] against the statement: the 16-bit row exact (the
    fp32 value it rounds is restated bit for bit, which is inside error term (c) by construction -- asserted against float64 too),
    R0 exact, R1 / R2 within [lo, hi], unboundable images and padding rows by their sentinels."""
    N, fmt = ref["N"], ref["fmt"]
    sure = ~ref["edge"]
    want = sr.bits16(ref["m16"], fmt)
    got = np.asarray(pooled_bits).view(np.uint16).reshape(N, -1)
    same = ((got == want) | ((got & 0x7FFF) == 0) & ((want & 0x7FFF) == 0)).all(axis=1)          # (+0 and -0 are the same zero row)
    assert same[sure].all(), f"pooled rows differ from the statement: images {np.nonzero(~same & sure)[0][:8]}"
    rp = np.asarray(rowp, dtype=np.float32)
    ub = ref["unboundable"]
    assert (rp[:N][ub & sure] == np.array([0, INF, 1, 0], np.float32)).all(), "an unboundable image without the keep-for-every-query constants"
    b = ~ub & sure
    assert (rp[:N][b][:, 0] == ref["s"][b].astype(np.float32)).all() and (rp[:N][b][:, 3] == 0).all()
    for col, lo, hi in ((1, "R1_lo", "R1_hi"), (2, "R2_lo", "R2_hi")):
        v = rp[:N][b][:, col].astype(np.float64)
        assert (v >= ref[lo][b]).all(), f"rowp[:, {col}] below what the derivation needs"
        assert (v <= ref[hi][b]).all(), f"rowp[:, {col}] looser than stated"
    pad = rp[N:]
    assert (pad[:, 0] == 0).all() and np.isnan(pad[:, 1]).all() and (pad[:, 2:] == 0).all()


def check_error_c(x, xn, ref):
    """||m_fl - m||_2 <= error_c(P) c1 for every boundable image, m in float64."""
    N, P, D = ref["N"], ref["P"], ref["D"]
    n = np.asarray(xn, np.float32).astype(np.float64).reshape(N, P)
    b = ~ref["unboundable"]
    with np.errstate(all="ignore"):
        m = (np.asarray(x, np.float32).astype(np.float64) / n[:, :, None]).mean(axis=1)
        err = np.sqrt(((ref["m_fl"].astype(np.float64) - m) ** 2).sum(axis=1))
    assert (err[b] <= error_c(P) * ref["c1"][b]).all()


def query_side(tw, qn, fmt, D, lo, eps):
    """The query's stage-1 operands and constants: sr.query_constants (query16_kernel is the row search's) under eps_m, plus
    g_lo = ||q'|| eps / qn (the least the proof accepts), the modelled float32 c and g, and `flagged` by the mean bound's windows."""
    em32 = np.float32(eps_m(fmt, D, lo) * (1.0 + 1e-6))
    ref = sr.query_constants(tw, qn, fmt, D, em32)
    qb = sr.model_qbase(ref)
    qn64 = ref["qn"].astype(np.float64)
    with np.errstate(all="ignore"):
        ref["g_lo"] = ref["norm"] * float(np.float32(eps)) / qn64
        gfac = np.float32(float(np.float32(eps)) / (eps_m(fmt, D, lo) * (1.0 + 1e-6)) * (1.0 + 1e-6))
        g = ((qb[:, 1] * gfac).astype(np.float32) / ref["qn"]).astype(np.float32)
        ref["g"] = (g * np.float32(1 + 2.0 ** -19)).astype(np.float32)
        ref["c"] = (qb[:, 1] * np.float32(1 + 2.0 ** -19)).astype(np.float32)
    s = ref["s"].astype(np.float64)
    ref["flagged"] = (ref["flagged"] | ~((qn64 >= QN_LO) & (qn64 <= QN_HI)) | ~((s >= SC_LO) & (s <= SC_HI))
                      | ~(ref["y_lo"] > 0) | ~np.isfinite(ref["g"]) | ~(ref["g"] < R_MAX) | ~(ref["c"] < R_MAX) | np.bool_(not eps >= 0))
    ref["qbase"], ref["lo"] = qb, lo
    return ref


def dot_hat(qref, pref):
    """dot^ [Q, N]: the 16-bit operands' products (exact in fp32), accumulated in fp32 in BLAS's order."""
    ofmt = "bf16" if qref["fmt"] == "bf16" else "fp16"
    qa = sr.widen16(qref["qh"], ofmt)
    if qref["lo"]:
        # hi and lo are multiplied separately and meet in the accumulator
        return (qa @ pref["m16"].T + sr.widen16(qref["ql"], ofmt) @ pref["m16"].T).astype(np.float32)
    return (qa @ pref["m16"].T).astype(np.float32)


def upper_bound(dot, qref, rowp):
    """U [Q, N] in float64 from the float32 constants: (dot^ + c R1 + g R2) / (R0 qn 2^-f); inf for an unboundable image."""
    rp = rowp.astype(np.float64)
    with np.errstate(all="ignore"):
        num = dot.astype(np.float64) + qref["c"].astype(np.float64)[:, None] * rp[None, :, 1] + qref["g"].astype(np.float64)[:, None] * rp[None, :, 2]
        U = num / (rp[None, :, 0] * qref["qn_s"].astype(np.float64)[:, None])
    return np.where(rp[None, :, 1] == INF, INF, U)


def passes(dot, qref, rowp, tau):
    """The candidate test as the matrix instruction computes it, t = fma chain of {-a, c, g, 0} x {R0, R1, R2, 0} onto dot^ in fp32
    (each step: exact in float64, rounded to fp32), with a = tau qn 2^-f lowered as mean_test_row lowers it.  tau: float32 [Q], or
    [Q, N] to give every pair a threshold of its own."""
    tau = np.asarray(tau, np.float32)
    t32 = np.maximum(tau if tau.ndim == 2 else tau[:, None], np.float32(-3.0e38))
    with np.errstate(all="ignore"):
        a = (t32 * qref["qn_s"][:, None]).astype(np.float32)
        a = (a - (np.abs(a) * np.float32(2.0 ** -19)).astype(np.float32)).astype(np.float32)
        a = np.where(a > np.float32(-3.0e38), a, np.float32(-3.0e38))
        t = dot.astype(np.float32)
        for coef, col in ((-a, 0), (qref["c"][:, None], 1), (qref["g"][:, None], 2)):
            t = (coef.astype(np.float64) * rowp[None, :, col].astype(np.float64) + t.astype(np.float64)).astype(np.float32)
    return t >= 0


def eps_m_cosine(qref, fmt, D):
    """eps_m in cosine units for each query: eps_m ||tw|| / qn (= eps_m under unit weights)."""
    return eps_m(fmt, D, qref["lo"]) * qref["norm"] / qref["qn_s"].astype(np.float64)


def staged_worst(N, Q, k):
    """Can a candidate list or staging region fill for a bank of N images?  Stage 1 appends at most N images to a query's list
    (cap 4096 / 8192) and at most 256 x 256 pairs per item to a staging list of 2048: a list cannot fill while N <= cap; the
    staging list can only when more than 2048 of an item's pairs pass, which the GPU test rules out by counting them."""
    return N <= sr.cap_of(k)
