"""NumPy restatement of the two-stage weighted-MSE token search's constants (csrc/topk_prefilter.hip, "Weighted MSE";
include/skyemb.h, skyemb_distance_topk_tokens_prefiltered): the row constants {B_dn, nx, 1, 0}, the query constants
{A_dn, eps_mse ||q'||, 2^-f, flag}, the hi / lo split of q' = fl(c o t) 2^-f and the interval [L, U] that must hold D x the
contract's distance.  Used by tests/test_token_mse_prefilter_cpu.py (the interval against tests/token_distance_reference.py) and
tests/test_token_mse_prefilter_gpu.py (the constants read back from the device).

Sums are taken in fp64 and then lowered / raised by the slack the kernels state (D 2^-22 relative), so a device value may differ
from these by that slack, never beyond the fp64 value on the unsafe side."""
import numpy as np

BT = 256
BF_ROW_LO, BF_ROW_HI, BF_SCALE_LO, BF_SCALE_HI, BF_QMAX_EXP = 60, 120, 100, 30, -20
MSE_SCALE_HI_F16, MSE_B_HI = 90, {"f16": 36, "bf16": 96}
C_MAX = 2.0 ** 10


def eps_a_resident(D, lo, dt):
    """The resident banks' eps_a (topk_prefilter.hip's eps_a_of(.., resident) / eps_a_bf16_of), same order of summation."""
    if dt == "bf16":
        return (2.0 ** -18 if lo else 2.0 ** -9) + 6.06 * D * 2.0 ** -24 + D * 2.0 ** -38
    return (2.0 ** -21 if lo else 2.0 ** -11 + 2.0 ** -21) + 6.06 * D * 2.0 ** -24 + np.sqrt(float(D)) * 2.0 ** -27


def eps_mse(D, lo, dt):
    return eps_a_resident(D, lo, dt) + 2.0 ** -22


def gamma(D):
    """The widening of the distance threshold: the contract's chain rounds n = chain_roundings(D) times along its longest path,
    + 3 for the second order."""
    return (chain_roundings(D) + 3) * 2.0 ** -24


def chain_roundings(D):
    """Roundings between a token's real distance and the contract's value, longest path: the subtraction (its error is squared: 2),
    the square, the product with c, the additions into a partial (partial j holds the m = 4 ceil(D / 64) elements with
    (d >> 2) & 15 == j: at most m rounded additions), four folds, one division."""
    m = 4 * ((D + 63) // 64)
    return 2 + 1 + 1 + m + 4 + 1


def bf16_round(a):
    """fp32 -> the nearest bf16 (ties to even), as fp32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    return np.where(np.isfinite(a), out, a).astype(np.float32)


def to16(a, dt):
    with np.errstate(over="ignore"):
        return a.astype(np.float16).astype(np.float32) if dt == "f16" else bf16_round(a)


def contract_distances(c, t, x):
    """[Q, R] fp32 MSE distances by the contract's chain for any D % 4 == 0 (tests/token_distance_reference.token_distances states
    it for D % 64 == 0; the CPU test holds the two bit-equal there): partial j takes the elements with (d >> 2) & 15 == j in
    ascending d, four folds, one division."""
    c, t, x = np.asarray(c, np.float32), np.asarray(t, np.float32), np.asarray(x, np.float32)
    R, D = x.shape
    out = np.empty((t.shape[0], R), np.float32)
    j = np.arange(16)
    with np.errstate(invalid="ignore", over="ignore"):
        for qi in range(t.shape[0]):
            p = np.zeros((R, 16), np.float32)
            for d0 in range(0, D, 4):
                for e in range(4):
                    d = x[:, d0 + e] - t[qi, d0 + e]
                    p[:, (d0 >> 2) & 15] = p[:, (d0 >> 2) & 15] + c[d0 + e] * (d * d)
            for f in (8, 4, 2, 1):
                p = p + p[:, j ^ f]
            out[qi] = p[:, 0] / np.float32(D)
    return out


def weights_flagged(c):
    """True when the weights flag EVERY query: a c_d negative, NaN or above 2^10."""
    c = np.asarray(c, np.float32)
    return bool(np.any(~((c >= 0) & (c <= C_MAX))))


def row_constants(c, x, dt):
    """-> (B64 [R] the fp64 value of B_r, B_dn [R], nx64 [R] the fp64 value the norm slot must reach, unboundable [R] bool) for
    the widened 16-bit rows x [R, D]."""
    c64, x64 = np.asarray(c, np.float32).astype(np.float64), np.asarray(x, np.float32).astype(np.float64)
    D = x.shape[1]
    mag = np.abs(x64)
    with np.errstate(invalid="ignore", over="ignore"):
        if dt == "bf16":
            bad = np.any(~(mag < 2.0 ** BF_ROW_HI) | ((mag > 0) & (mag < 2.0 ** -BF_ROW_LO)), axis=1)
        else:
            bad = np.any(~(mag < np.inf), axis=1)
        B64 = (c64 * x64 * x64).sum(axis=1)
        bad |= ~((B64 >= 0) & (B64 < 2.0 ** MSE_B_HI[dt]))
        nsub = ((mag > 0) & (mag < 2.0 ** -14)).sum(axis=1) if dt == "f16" else np.zeros(len(x))
        nx64 = np.sqrt((x64 * x64).sum(axis=1)) + np.sqrt(nsub) * 2.0 ** -14 / eps_mse(D, True, "f16")
        B_dn = np.where(B64 < 2.0 ** -100, 0.0, B64.astype(np.float32).astype(np.float64) * (1.0 - D * 2.0 ** -22))
    return B64, B_dn, nx64, bad


def query_constants(c, t, dt, lo):
    """-> dict: tw fp32 [Q, D]; s = 2^-f [Q]; qh, ql (the 16-bit operands as fp32, ql zero without lo); A64, A_dn; cq = eps_mse ||q'||
    (raised as the kernel raises it); flagged [Q] bool."""
    c32, t32 = np.asarray(c, np.float32), np.asarray(t, np.float32)
    Q, D = t32.shape
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        tw = (c32[None, :] * t32).astype(np.float32)
        mx = np.abs(tw).max(axis=1)
        e = np.zeros(Q, np.int64)
        ok = (mx > 0) & np.isfinite(mx)
        e[ok] = np.frexp(mx[ok])[1] - (BF_QMAX_EXP if dt == "bf16" else 14)
        e = np.maximum(e, -126)
        if dt == "bf16":
            e = np.minimum(e, BF_SCALE_LO)
        s = np.ldexp(np.float32(1.0), -e).astype(np.float32)
        qp = (tw * s[:, None]).astype(np.float32)
        qh = to16(qp, dt)
        ql = to16((qp - qh).astype(np.float32), dt) if lo else np.zeros_like(qh)
        A64 = (c32.astype(np.float64) * t32.astype(np.float64) ** 2).sum(axis=1)
        A32 = A64.astype(np.float32).astype(np.float64)
        A_dn = np.where(~(A64 >= 2.0 ** -100), 0.0, A32 * (1.0 - D * 2.0 ** -22))
        nq = np.sqrt((qp.astype(np.float64) ** 2).sum(axis=1)) * (1.0 + D * 2.0 ** -22)
        cq = eps_mse(D, lo, dt) * (1.0 + 1e-6) * nq
        lo_s, hi_s = (2.0 ** -BF_SCALE_LO, 2.0 ** BF_SCALE_HI) if dt == "bf16" else (0.0, 2.0 ** MSE_SCALE_HI_F16)
        flagged = weights_flagged(c32) | ~np.isfinite(A32) | (s >= hi_s) | (s <= lo_s) | ~((cq > 0) & (cq < 2.0 ** 60))
    return dict(tw=tw, s=s.astype(np.float64), qh=qh, ql=ql, A64=A64, A_dn=A_dn, cq=cq, flagged=flagged)


def interval(c, t, x, dt, lo):
    """-> (L, U [Q, R] fp64, trusted [Q, R] bool): bounds of D x dist for the pairs the route trusts (query not flagged, row
    boundable).  dot^ is taken as the exact sum of the 16-bit operands' products rounded to fp32 -- one of the values the matrix
    cores may return; any other differs by less than the accumulation term of eps_a."""
    qc = query_constants(c, t, dt, lo)
    B64, B_dn, nx64, ub = row_constants(c, x, dt)
    D = x.shape[1]
    x64 = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dot = ((qc["qh"].astype(np.float64) + qc["ql"].astype(np.float64)) @ np.where(np.isfinite(x64), x64, 0.0).T).astype(np.float32).astype(np.float64)
        err = qc["cq"][:, None] * (nx64 * (1.0 + D * 2.0 ** -22))[None, :]
        inv = (1.0 / qc["s"])[:, None]
        L = qc["A_dn"][:, None] + B_dn[None, :] - 2.0 * inv * (dot + err)
        A_up = qc["A64"] * (1.0 + D * 2.0 ** -22)
        U = A_up[:, None] + (B64 * (1.0 + D * 2.0 ** -22))[None, :] - 2.0 * inv * (dot - err)
    return L, U, ~qc["flagged"][:, None] & ~ub[None, :]


def contains(L, U, dist32, D):
    """The statement the kernel's test relies on, per pair: L <= D dist^ (1 + gamma) + 2^-126, and the mirror image for U."""
    dd = dist32.astype(np.float64) * D
    g = gamma(D)
    return (L <= dd * (1.0 + g) + 2.0 ** -126) & (dd <= U * (1.0 + g) + 2.0 ** -126)
