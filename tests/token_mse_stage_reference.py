"""Plain statements (numpy, float64, exact rationals) of what the weighted-MSE forms of the two-stage token search must do PAIR BY
PAIR and IMAGE BY IMAGE -- the test row mse_test_row publishes, the flags of mse_state_kernel, the instruction's test value, the
lower bound L, the classes of tokens and images at a known threshold, inputs whose dot^ has one admissible value -- for
tests/test_token_mse_stage_{cpu,gpu}.py.  The code under test is csrc/topk_prefilter.hip, "Weighted MSE" and "Weighted MSE with
PER-QUERY weights".  Built on tests/token_mse_prefilter_reference.py and tests/token_mse_pq_reference.py (constants, eps, gamma, the
contract's chain), tests/token_distance_reference.py (the combine and the top-k), tests/token_prefilter_stage_reference.py (the
schedule, slice_taus, the list keys) and tests/prefilter_stage1_reference.py (check_sandwich, the integer grid): none of those is
restated here.

Key space throughout: key = -distance, tau a key threshold, theta = -tau the distance threshold."""
import functools
from fractions import Fraction

import numpy as np

from tests import prefilter_stage1_reference as sr
from tests import token_distance_reference as tdr
from tests import token_mse_pq_reference as pqr
from tests import token_mse_prefilter_reference as mpr
from tests import token_prefilter_stage_reference as tr

BT, INF = sr.BT, float("inf")
F = np.float32
OPEN = 3.0e38                                                           # the kernel's "no threshold": fp32(3.0e38f)
FMT = {"f16": "fp16", "bf16": "bf16"}                                   # the names tests/prefilter_stage1_reference.py uses
slice_taus = tr.slice_taus                                              # fits unchanged: scores are keys, a +inf distance is key -inf


def eps_f32(D, lo, dt, pq):
    """The float the driver hands to the query kernel: eps_mse or eps_pq raised by 1e-6, rounded once."""
    return F((pqr.eps_pq(D, lo, dt) if pq else mpr.eps_mse(D, lo, dt)) * (1.0 + 1e-6))


def gamma_f32(D):
    return F(mpr.gamma(D) * (1.0 + 1e-6))


# ------------------------------------------------------------------------------------------------------------- fp32, one rounding
def round_f32(x):
    """A rational -> the nearest fp32 (ties to even; subnormals; overflow to inf), as a Python float."""
    x = Fraction(x)
    if x == 0:
        return 0.0
    sign, a = (-1.0 if x < 0 else 1.0), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()          # 2^(e-1) <= a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1                                                         # 2^e <= a < 2^(e+1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = a / quantum
    r = n.numerator // n.denominator
    rem = n - r
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and r % 2):
        r += 1
    v = r * quantum
    return sign * INF if v >= Fraction(2) ** 128 else sign * float(v)


def _fma32(a, b, c):
    """fmaf(a, b, c) of three fp32 numbers with ONE rounding (exact rationals; inf / NaN by IEEE's rules through float64, which
    holds a product of two floats exactly)."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    return round_f32(Fraction(a) * Fraction(b) + Fraction(c))


def model_mse_qpar(tau, qbase, D, gamma32):
    """mse_test_row restated in fp32, one operation per line: tau [Q] (key space), qbase [Q, 4] = {A_dn, eps ||q'||, 2^-f, flag}
    -> (qpar float32 [Q, 4] = {-a, c, g, 0}, bad bool [Q]).
      theta = -tau, or 3e38 when tau is not above -3e38 (no threshold yet);   T = theta D;   T = fmaf(|T|, gamma, T) + 2^-126;
      T above 3e38 is 3e38 (a T that is not a number -- theta = -inf, a floor of +inf -- stays: the query is refused);
      h = 0.5 qb.z;   g = h (T - qb.x);   g += |g| 2^-19;   g above 3e38 is 3e38;   bad: g is not a number >= -3e38;
      -a = -(h - h 2^-19);   c = qb.y (1 + 2^-19)."""
    tau, qb = np.asarray(tau, F), np.asarray(qbase, F)
    Q = len(tau)
    out, bad = np.zeros((Q, 4), F), np.zeros(Q, bool)
    g32, fD, two19 = F(gamma32), F(D), F(2.0 ** -19)
    with np.errstate(all="ignore"):
        for q in range(Q):
            theta = F(-tau[q]) if tau[q] > F(-OPEN) else F(OPEN)
            T = F(theta * fD)
            T = F(F(_fma32(abs(T), g32, T)) + F(2.0 ** -126))
            if T > F(OPEN):
                T = F(OPEN)
            h = F(F(0.5) * qb[q, 2])
            g = F(h * F(T - qb[q, 0]))
            g = F(_fma32(abs(g), two19, g))                            # (the product is exact: with or without contraction)
            if g > F(OPEN):
                g = F(OPEN)
            bad[q] = not (g >= F(-OPEN))
            a = F(h - F(h * two19))
            out[q] = (-a, F(qb[q, 1] * F(1.0 + 2.0 ** -19)), g, 0.0)
    return out, bad


def model_mse_flags(qbase, bad, dt):
    """mse_state_kernel's overflow rule -> bool [Q]: the test row left fp32's range, qb.w (a weight outside [0, 2^10], A^ not
    finite; per-query weights: c o t = 0), the scale outside (0, 2^90) (fp16) / (2^-100, 2^30) (bf16), or eps ||q'|| not in
    (0, 2^60)."""
    qb = np.asarray(qbase, F)
    lo_s, hi_s = (2.0 ** -mpr.BF_SCALE_LO, 2.0 ** mpr.BF_SCALE_HI) if dt == "bf16" else (0.0, 2.0 ** mpr.MSE_SCALE_HI_F16)
    with np.errstate(invalid="ignore"):
        return np.asarray(bad, bool) | (qb[:, 3] != 0) | (qb[:, 2] >= hi_s) | (qb[:, 2] <= lo_s) | ~((qb[:, 1] > 0) & (qb[:, 1] < 2.0 ** 60))


def first_tau(thr0, Q):
    """mse_state_kernel's first threshold: the floor, a NaN or a missing one counting as -inf."""
    tau = np.full(Q, -INF, F) if thr0 is None else np.asarray(thr0, F).copy()
    tau[np.isnan(tau)] = -INF
    return tau


# --------------------------------------------------------------------------------------------------------- the test and the bound
def pair_test_value(dot_hat, qpar, rowp):
    """The instruction's t = dot^ + qpar.x R0 + qpar.y R1 + qpar.z R2 for every pair, in float64 -> [Q, R]."""
    qp, rp = np.asarray(qpar, np.float64), np.asarray(rowp, np.float64)
    with np.errstate(all="ignore"):
        return (np.asarray(dot_hat, np.float64) + qp[:, 0:1] * rp[None, :, 0] + qp[:, 1:2] * rp[None, :, 1] + qp[:, 2:3] * rp[None, :, 2])


def lower_bound(dot_hat, qbase, rowp):
    """L = A_dn + B_dn - 2 2^f (dot^ + qbase.y rowp.y) [Q, R] in float64 (per-query weights: B_dn = rowp.x = 0)."""
    qb, rp = np.asarray(qbase, np.float64), np.asarray(rowp, np.float64)
    with np.errstate(all="ignore"):
        return qb[:, 0:1] + rp[None, :, 0] - 2.0 / qb[:, 2:3] * (np.asarray(dot_hat, np.float64) + qb[:, 1:2] * rp[None, :, 1])


def operand_dot(qh, ql, y):
    """sum_d (qh_d + ql_d) y_d in float64: the exact product of the 16-bit operands (22-bit products, at most 4096 of them)."""
    with np.errstate(all="ignore"):
        y64 = np.asarray(y, np.float64)
        return (np.asarray(qh, np.float64) + np.asarray(ql, np.float64)) @ np.where(np.isfinite(y64), y64, 0.0).T


def real_dot(tw, s, x, c=None):
    """2^-f sum_d tw_d x_d in float64 over the fp32 tw [Q, D]; with c [Q, D] (per-query weights): 2^-f u_q . y_x, u = [tw ; -c / 2],
    y_x = [x ; x o x] with the REAL squares."""
    x64 = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        d = np.asarray(tw, np.float64) @ x64.T
        if c is not None:
            d = d - 0.5 * np.asarray(c, np.float64) @ (x64 * x64).T
        return d * np.asarray(s, np.float64)[:, None]


def check_pair_bound(dot_hat, real, qbase, rowp, ok):
    """(i) |dot^ - real| <= qbase.y rowp.y for the pairs in `ok`, no tolerance -> (reason or None, largest error / bound)."""
    qb, rp = np.asarray(qbase, np.float64), np.asarray(rowp, np.float64)
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(dot_hat, np.float64) - real)
        bound = qb[:, 1:2] * rp[None, :, 1]
        use = ok & np.isfinite(bound) & (bound > 0)
        bad = use & ~(err <= bound)
        ratio = float((err[use] / bound[use]).max()) if use.any() else 0.0
    if bad.any():
        q, r = np.argwhere(bad)[0]
        return f"{int(bad.sum())} pairs outside the bound, first (query {q}, row {r}): |{dot_hat[q, r]!r} - {real[q, r]!r}| > {bound[q, r]!r}", ratio
    return None, ratio


def check_lower_bound(L, dist32, D, ok, gamma=None):
    """(ii) L <= D dist^ (1 + gamma) + 2^-126 for the pairs in `ok` with a finite contract distance, no tolerance (gamma: the
    statement's, unless the CPU file plants another) -> (reason or None, the largest L / right-hand side over the pairs whose
    right-hand side is positive)."""
    with np.errstate(all="ignore"):
        rhs = np.asarray(dist32, np.float64) * D * (1.0 + (mpr.gamma(D) if gamma is None else gamma)) + 2.0 ** -126
        use = ok & np.isfinite(rhs)
        bad = use & ~(L <= rhs)
        pos = use & (rhs > 2.0 ** -100)
        ratio = float((L[pos] / rhs[pos]).max()) if pos.any() else 0.0
    if bad.any():
        q, r = np.argwhere(bad)[0]
        return f"{int(bad.sum())} pairs with L above the widened distance, first (query {q}, row {r}): {L[q, r]!r} > {rhs[q, r]!r}", ratio
    return None, ratio


def check_query_constants(qbase, qc, D, eps, ok, D_sum=None):
    """qbase [Q, 4] against the constants modules' query_constants `qc` for the queries in `ok`: the scale exactly; A_dn never above
    the fp64 sum, within 2 D 2^-22 below it where the sum is above 2^-99 and 0 where it is below 2^-101; qbase.y never below
    eps ||q'|| in fp64 (eps: the statement's, before the raise) and within the same slack above (D_sum: the length of q', 2 D under
    per-query weights).  -> reason or None."""
    qb = np.asarray(qbase, np.float64)
    Ds = D if D_sum is None else D_sum
    if not np.array_equal(qb[ok, 2], qc["s"][ok]):
        return "the scale 2^-f differs"
    if not (qb[ok, 3] == 0).all():
        return "an unflagged query carries a flag"
    slack = 2.0 * Ds * 2.0 ** -22
    big, tiny = ok & (qc["A64"] >= 2.0 ** -99), ok & (qc["A64"] < 2.0 ** -101)
    if not (qb[tiny, 0] == 0).all():
        return "A_dn of a sum below 2^-100 is not 0"
    if not (qb[big, 0] <= qc["A64"][big]).all():
        return f"A_dn is above the fp64 sum (query {int(np.flatnonzero(big)[np.argmax(qb[big, 0] > qc['A64'][big])])}): not a lower bound"
    if not (qb[big, 0] >= qc["A64"][big] * (1.0 - slack)).all():
        return "A_dn is further below the fp64 sum than the stated slack"
    with np.errstate(all="ignore"):
        src = qc["u"] if "u" in qc else qc["tw"]
        qp = (src * qc["s"][:, None].astype(F)).astype(F).astype(np.float64)
    need = eps * np.sqrt((qp * qp).sum(axis=1))
    if not (qb[ok, 1] >= need[ok]).all():
        return f"qbase.y is below eps ||q'|| (query {int(np.flatnonzero(ok)[np.argmax(qb[ok, 1] < need[ok])])}): the half-width is not a bound"
    if not (qb[ok, 1] <= need[ok] * (1.0 + slack)).all():
        return "qbase.y is further above eps ||q'|| than the stated slack"
    return None


# ------------------------------------------------------------------------------------------------------------------- the classes
def token_classes(tau, qbase, rowp, dot16, dist32, D):
    """For key thresholds tau [Q] the kernels KNEW: (must_in, must_out) boolean [Q, R] per token.
      must-in    the contract's fp32 distance is <= theta (theta = -tau, 3e38 with no threshold): the token reaches the threshold.
      must-out   the test expression, in float64 with the test row of model_mse_qpar(tau, qbase) and the exact product of the
                 16-bit operands in place of dot^, stays negative after dot^ is moved up by TWICE the proven bound b = qbase.y
                 rowp.y (dot^ and the operands' product each lie within b of the real sum) plus the slack of the instruction's own
                 fp32 chain, 2^-17 (|a R0| + c R1 + |g| + |dot| + 2 b) -- four times the 2^-19 per term the kernel's comment
                 grants it.  A listed pair passed t >= 0, so t + 2 b + slack < 0 with the operands' product means it cannot have.
    A pair whose bound is not finite (an unboundable row) or whose query's test row is not a number is never must-out."""
    qpar, _ = model_mse_qpar(tau, qbase, D, gamma_f32(D))
    tau = np.asarray(tau, F)
    theta = np.where(tau > F(-OPEN), -tau, F(OPEN)).astype(F)
    with np.errstate(all="ignore"):
        must_in = np.asarray(dist32, F) <= theta[:, None]
        qp, rp, qb = qpar.astype(np.float64), np.asarray(rowp, np.float64), np.asarray(qbase, np.float64)
        b = qb[:, 1:2] * rp[None, :, 1]
        aR, cR, g = qp[:, 0:1] * rp[None, :, 0], qp[:, 1:2] * rp[None, :, 1], qp[:, 2:3] * rp[None, :, 2]
        t = dot16 + aR + cR + g
        slack = 2.0 ** -17 * (np.abs(aR) + np.abs(cR) + np.abs(g) + np.abs(dot16) + 2 * b)
        must_out = t + 2 * b + slack < 0
    assert not (must_in & must_out).any()
    return must_in, must_out


def image_classes(tin, tout, P, combine, top_t=None, flags=None):
    """The token classes [Q, N P] folded into images [Q, N]; combine is the DISTANCE combine.
      min                 in when any token is in, out when all tokens are out
      max                 in when all tokens are in, out when any token is out
      max under top_t = t in when at least t tokens are in, out when more than P - t tokens are out
    A deselected image (flags) is in neither class."""
    Q = tin.shape[0]
    ti, to = np.asarray(tin, bool).reshape(Q, -1, P), np.asarray(tout, bool).reshape(Q, -1, P)
    if combine == "min":
        must_in, must_out = ti.any(axis=2), to.all(axis=2)
    elif top_t is None or top_t == P:
        assert combine == "max"
        must_in, must_out = ti.all(axis=2), to.any(axis=2)
    else:
        assert combine == "max" and 1 <= top_t < P
        must_in, must_out = ti.sum(axis=2) >= top_t, to.sum(axis=2) > P - top_t
    assert not (must_in & must_out).any()
    if flags is not None:
        must_in, must_out = must_in & flags[None, :], must_out & flags[None, :]
    return must_in, must_out


def fold_pass_bits(row_pass, P, combine, top_t=None, wrong=None, skip=None, off_by=0):
    """Candidate images [Q, N] from per-token pass bits [Q, N P] as stage 1 folds them (distance combine).  The planted defects of
    the CPU file: wrong -- OR and AND swapped; skip = p -- token p left out of the fold; off_by -- the counting fold's threshold
    moved by that much."""
    r = np.asarray(row_pass, bool).reshape(row_pass.shape[0], -1, P)
    if combine == "max" and top_t is not None and top_t != P:
        return r.sum(axis=2) >= top_t + off_by
    use_and = (combine == "max") != (wrong is not None)
    if skip is not None:
        r = r.copy()
        r[:, :, skip] = use_and
    return r.all(axis=2) if use_and else r.any(axis=2)


def undecided_share(must_in, must_out, scope=None):
    """Per query the share of images (inside the boolean scope [N]) that are neither must-in nor must-out."""
    care = ~must_in & ~must_out
    return care.mean(axis=1) if scope is None else care[:, scope].mean(axis=1)


# ------------------------------------------------------------------------------------------------------- inputs on an integer grid
@functools.lru_cache(maxsize=None)
def exact_grid_case(dt, lo, Q, R, D, pq, seed=0):
    """Inputs on which every product and every partial sum of stage 1 is exact, so dot^ has ONE admissible value.  The queries'
    tw = (H + L) 2^(..+f) and the rows m 2^g, m in -3 .. 3, are those of tests/prefilter_stage1_reference.exact_grid_case (its bit
    budget holds for them and is asserted there); here they are turned into the MSE search's inputs:
      shared weights     c_d = 2^-j_d, j in 0 .. 3, t_d = tw_d 2^j_d: fl(c o t) = tw without rounding.
      per-query weights  the rows are redrawn with g in 0 .. 2 -- so that x o x = m^2 2^(2 g) is a number of the operand format and a
                         multiple of the row's unit 2^g --, and -c_qd / 2 = -v_d 2^f with v a power of two on the operand grid
                         below the first half's binade (fp16: 1, 2, 4; bf16: 2^-24, 2^-23, 2^-22): qh holds it, ql is zero, the
                         scale is set by the first half; t = tw / c, exact.  The budget of the sum over 2 D elements is asserted.
    -> dict(c, t, x (float32 [R, D]), dot (float32 [Q, R], the exact dot^ under lo))."""
    fmt = FMT[dt]
    g0 = sr.exact_grid_case(fmt, lo, Q, R, D, 100 + seed)
    rng = np.random.default_rng(7 + seed)
    tw, f = g0["tw"], g0["f"]
    if not pq:
        j = rng.integers(0, 4, size=D)
        c = np.ldexp(F(1.0), -j).astype(F)
        t = np.ldexp(tw, j[None, :]).astype(F)
        assert np.array_equal((c[None, :] * t).astype(F), tw)
        return dict(c=c, t=t, x=g0["x"], dot=g0["dot"])
    bf = dt == "bf16"
    m = rng.integers(-3, 4, size=(R, D))
    m[np.arange(R), rng.integers(0, D, size=R)] = 3
    g = rng.integers(0, 3, size=R)
    x = np.ldexp(m.astype(F), g[:, None]).astype(F)
    vexp = rng.integers(-24, -21, size=D) if bf else rng.integers(0, 3, size=D)
    qexp = -32 if bf else 0                                             # the unit of q' (sr.exact_grid_case)
    q1 = (g0["H"].astype(np.float64) + (g0["L"].astype(np.float64) if lo else 0.0)) * 2.0 ** -qexp       # integers: the first half
    v = np.ldexp(1.0, vexp - qexp)                                      # integers: the second half's magnitudes
    assert (q1 == np.rint(q1)).all() and (v == np.rint(v)).all()
    full = np.abs(g0["H"].astype(np.float64) * 2.0 ** -qexp) + np.abs(g0["L"].astype(np.float64) * 2.0 ** -qexp)
    worst = float(full.max(axis=0).sum()) * 3 + float(v.sum()) * 9 * 2.0 ** int(g.max())
    assert worst < 2 ** 24, (dt, D, worst)                              # in units of 2^qexp 2^g_row: every partial sum is an fp32 number
    d = q1 @ m.T.astype(np.float64) - v[None, :] @ ((m * m).T.astype(np.float64) * np.ldexp(1.0, g)[None, :])
    assert float(np.abs(d).max()) < 2 ** 24 and (d == np.rint(d)).all()
    dot = np.ldexp(d, (g + qexp)[None, :]).astype(F)
    assert (dot.astype(np.float64) == np.ldexp(d, (g + qexp)[None, :])).all()
    c = np.ldexp(F(1.0), (vexp[None, :] + 1 + f[:, None])).astype(F)     # c_qd = 2 v_d 2^f_q
    t = (tw / c).astype(F)
    assert np.array_equal((c * t).astype(F), tw) and (c <= mpr.C_MAX).all()
    assert np.array_equal(mpr.to16((x * x).astype(F), dt), (x * x).astype(F))
    return dict(c=c, t=t, x=x, dot=dot)


# ------------------------------------------------------------------------------------------------------------- ordinary inputs
def scaled_bank(rng, N, P, D, dt, decades):
    """The bank of tests/test_token_mse_prefilter_gpu.py -- images whose tokens share a direction -- with every ROW scaled by
    10^u, u uniform over `decades`; -> the float32 values the 16-bit bank holds [N, P, D]."""
    x = rng.standard_normal((N, 1, D)) * rng.uniform(0.3, 2.0, (N, 1, 1)) + 0.7 * rng.standard_normal((N, P, D))
    x = x * 10.0 ** rng.uniform(decades[0], decades[1], (N, P, 1))
    return mpr.to16(x.astype(F), dt)


def weights_pq(rng, Q, D):
    """Per-query weight rows (tests/test_token_mse_pq_gpu.py's): rows scaled by 2^-20 .. 2^9, elements spread over 2^-10 .. 1, / D."""
    w = (rng.random((Q, D)).astype(F) + F(0.05)) * np.exp2(-10.0 * rng.random((Q, D))).astype(F)
    w = (w * np.exp2(rng.integers(-20, 10, (Q, 1))).astype(F)).astype(F)
    return np.minimum(w / F(D), F(2.0 ** 9)).astype(F)


def weights_shared(rng, D):
    c = (rng.random(D).astype(F) + F(0.05))
    return (c / c.sum()).astype(F)


def contract(c, t, x):
    """[Q, R] fp32 contract distances under shared c [D] or per-query c [Q, D]."""
    with np.errstate(all="ignore"):
        return pqr.contract_distances(c, t, x) if np.ndim(c) == 2 else mpr.contract_distances(c, t, x)


def model_constants(c, t, x, dt, lo):
    """A model of what the device leaves -- qbase [Q, 4], rowp [R, 4], the operands (qh, ql, y) -- from the statements of the two
    constants modules: the material of the CPU file, and of the conditions asserted on the GPU file's inputs."""
    pq = np.ndim(c) == 2
    D = x.shape[1]
    if pq:
        qc = pqr.query_constants(c, t, dt, lo)
        y, ub = pqr.image(x, dt)
        ny, _ = pqr.row_constants(x, dt)
        ny = np.where(ub, INF, ny * (1.0 + 2 * D * 2.0 ** -22))
        rowp = np.stack([np.zeros(len(x)), ny, np.ones(len(x)), np.zeros(len(x))], axis=1)
    else:
        qc = mpr.query_constants(c, t, dt, lo)
        _, B_dn, nx, ub = mpr.row_constants(c, x, dt)
        y = np.where(ub[:, None], 0.0, x)
        rowp = np.stack([np.where(ub, 0.0, B_dn), np.where(ub, INF, nx * (1.0 + D * 2.0 ** -22)), np.ones(len(x)), np.zeros(len(x))], axis=1)
    up = lambda a: np.where(a.astype(F).astype(np.float64) < a, np.nextafter(a.astype(F), F(INF)), a.astype(F))      # fp32, never below
    dn = lambda a: np.where(a.astype(F).astype(np.float64) > a, np.nextafter(a.astype(F), F(-INF)), a.astype(F))     # fp32, never above
    with np.errstate(all="ignore"):
        qbase = np.stack([np.where(qc["flagged"], 0.0, dn(qc["A_dn"])), up(qc["cq"]), qc["s"].astype(F), qc["flagged"].astype(F)], axis=1).astype(F)
        rowp32 = np.stack([dn(rowp[:, 0]), up(rowp[:, 1]), rowp[:, 2], rowp[:, 3]], axis=1).astype(F)
    return dict(qc=qc, qbase=qbase, rowp=rowp32, y=y, ub=ub, dot16=operand_dot(qc["qh"], qc["ql"], y))


def keys_of(dist, P, combine, top_t=None, flags=None):
    """[Q, N] float32 combined KEYS of the token distances [Q, N P]; a deselected image is -inf."""
    Q = dist.shape[0]
    d = tdr.combine_distances(np.ascontiguousarray(dist, F).reshape(Q, -1, P), combine, top_t)
    keys = (-d).astype(F)
    return keys if flags is None else np.where(flags[None, :], keys, F(-INF))


def topk_of_keys(keys, k, idx_offset=0):
    """(keys [Q, k] descending, images [Q, k]) with ties to the lower image and (-inf, -1) for missing entries."""
    d, i = tdr.topk_of_distances((-keys).astype(F), k, idx_offset)
    return (-d).astype(F), i


# -------------------------------------------------------------------------------------------------- the image-by-image cases
QSTAR = 3
DELTA = 0.15                                                            # a probe token's distance is theta (1 -+ DELTA)


def schedule_of(N, P, k, pq=False):
    """tr.token_schedule for the MSE entries; per-query weights plan over the image's rows padded to whole tiles (no tail tile), the
    masks cut back to the N real images."""
    if not pq:
        return tr.token_schedule(N, P, k)
    sched = tr.token_schedule(-(-N * P // BT) * BT // P, P, k)
    sched["images"] = [m[:N] for m in sched["images"]]
    return sched


def probe_slots(P, N, variant):
    """(token position, kind) of the probe images: every token position with an 'in' and an 'out' probe, twice (the images land on
    both ends of their tiles); P = 64 has room for 16 probes: positions 4 j + variant, kinds alternating."""
    if 4 * P <= N // 2:
        return [(p, kind) for p in range(P) for kind in ("in", "out") for _ in range(2)]
    return [(4 * j + variant % 4, ("in", "out")[(j + variant) % 2]) for j in range(min(16, N // 2))]


@functools.lru_cache(maxsize=8)
def stage_case(P, combine, dt, lo, N, k, Q=130, D=128, pq=False, top_t=None, seed=0, dup=False):
    """An ordinary token bank (images of mixed scale) with probe images for query QSTAR planted in the second half of the images,
    and everything the image-by-image checks need, computed once.
    A probe image is built around t* = t[QSTAR] along random directions u: a token at distance theta (1 -+ DELTA) from t*, theta the
    distance threshold of the floor, is x = t* + r u with r from sum c (r u)^2 = D theta (1 -+ DELTA).  'in' probe at position p: the
    one token that decides the image is just INSIDE theta -- under 'min' every other token lies at 9 theta (out), under 'max' every
    other token at theta / 4 (in) and token p at theta (1 - DELTA); under top_t = t, t - 1 other tokens are in and the rest out.
    'out' probe: the same with token p just OUTSIDE.  So the lane of token p decides the image on its own.
    thr0 [Q]: the k-th best combined key over the first half of the images (ordinary ones), from the contract's distances.
    dup: the best image of query 0 is copied, bit for bit, over an ordinary image of the last slice."""
    rng = np.random.default_rng(1000 * seed + 10 * P + (combine == "max") + 2 * (dt == "bf16") + 4 * lo + 8 * pq + 16 * (top_t or 0) + N)
    R = N * P
    t = rng.standard_normal((Q, D)).astype(F)
    c = weights_pq(rng, Q, D) if pq else weights_shared(rng, D)
    if pq:
        c = (c / c.sum(axis=1, keepdims=True)).astype(F)               # rows as prepare_distance_weights leaves them
    x = rng.standard_normal((N, 1, D)) * rng.uniform(0.3, 2.0, (N, 1, 1)) + 0.7 * rng.standard_normal((N, P, D))
    xw = mpr.to16(x.astype(F), dt)
    half = (N * P // BT) * (BT // P) // 2                              # half of the images of the whole tiles
    sched = schedule_of(N, P, k, pq)
    with np.errstate(all="ignore"):
        d0 = contract(c, t, xw[:half].reshape(half * P, D))
    thr0 = tr.kth_finite(keys_of(d0, P, combine, top_t), k)
    assert (thr0 > -INF).all()
    # ---- the probes of QSTAR
    theta = float(-thr0[QSTAR])
    cs = (c[QSTAR] if pq else c).astype(np.float64)
    kind = np.zeros(N, np.int64)                                        # 0 ordinary, 1 'in' probe, 2 'out' probe
    probe_p = np.full(N, -1, np.int64)
    ipt = BT // P
    order = [v for pair in zip(range(ipt), range(ipt - 1, -1, -1)) for v in pair][:ipt]       # 0, ipt-1, 1, ipt-2, ...
    first_tile = -(-half // ipt)
    tiles_free = max((N // ipt) - first_tile, 1)
    variant = 2 * (dt == "bf16") + (combine == "max")

    def token(scale):
        u = rng.standard_normal(D)
        r = np.sqrt(D * theta * scale / (cs * u * u).sum())
        return t[QSTAR].astype(np.float64) + r * u

    slots = probe_slots(P, N, variant)
    if N * P % BT:                                                      # a ragged bank: one probe of each kind in the tail tile
        slots = slots + [(P - 1, "in"), (0, "out")]
    for s, (p, what) in enumerate(slots):
        if s >= len(slots) - 2 and N * P % BT:
            i = (N * P // BT) * ipt + (s - (len(slots) - 2))
        else:
            i = (first_tile + s % min(tiles_free, 4)) * ipt + order[s // min(tiles_free, 4)]
        assert half <= i < N and kind[i] == 0, (i, s)
        n_in = 0 if combine == "min" else (P - 1 if top_t in (None, P) else top_t - 1)      # the other tokens that are in
        others = np.array([True] * n_in + [False] * (P - 1 - n_in))
        rng.shuffle(others)
        img, o = np.zeros((P, D)), 0
        for pp in range(P):
            if pp == p:
                img[pp] = token(1.0 - DELTA if what == "in" else 1.0 + DELTA)
            else:
                img[pp] = token(0.25 if others[o] else 9.0)
                o += 1
        xw[i] = mpr.to16(img.astype(F), dt)
        kind[i], probe_p[i] = (1 if what == "in" else 2), p
    flat = np.ascontiguousarray(xw.reshape(R, D))
    with np.errstate(all="ignore"):
        dist = contract(c, t, flat)
    tie = None
    if dup:
        keys0 = keys_of(dist[:1], P, combine, top_t)[0]
        g = int(np.argmax(keys0))                                       # query 0's best image, and its copy in the last slice
        dst = int(np.flatnonzero(sched["images"][-1] & (kind == 0) & (np.arange(N) != g))[-1])
        xw[dst] = xw[g]
        flat = np.ascontiguousarray(xw.reshape(R, D))
        dist[:, dst * P:(dst + 1) * P] = dist[:, g * P:(g + 1) * P]
        tie = (min(g, dst), max(g, dst))
        assert sched["images"][-1][tie[1]]
    keys = keys_of(dist, P, combine, top_t)
    mc = model_constants(c, t, flat, dt, lo)
    return dict(P=P, combine=combine, dt=dt, lo=lo, N=N, k=k, Q=Q, D=D, pq=pq, top_t=top_t, c=c, t=t, xw=xw, flat=flat, dist=dist, keys=keys,
                thr0=thr0, kind=kind, probe_p=probe_p, sched=sched, model=mc, tie=tie)


def case_classes(case, tau, qbase=None, rowp=None, flags=None):
    """(must_in, must_out) [Q, N] of a stage_case at key thresholds tau [Q], with the device's constants when given, else the
    model's; a flagged query of the model is in no class (the route hands it back)."""
    mc = case["model"]
    qbase = mc["qbase"] if qbase is None else qbase
    rowp = mc["rowp"] if rowp is None else np.asarray(rowp)[:case["N"] * case["P"]]
    ti, to = token_classes(tau, qbase, rowp, mc["dot16"], case["dist"], case["D"])
    return image_classes(ti, to, case["P"], case["combine"], case["top_t"], flags)


def check_probes(case, have, flags=None):
    """QSTAR's probes one by one against the candidate mask have [N]: every 'in' probe present, every 'out' probe absent."""
    on = np.ones(case["N"], bool) if flags is None else flags
    lost = np.flatnonzero((case["kind"] == 1) & on & ~have)
    if len(lost):
        return f"'in' probes not listed: images {lost[:8].tolist()}, token positions {case['probe_p'][lost[:8]].tolist()}"
    wrong = np.flatnonzero((case["kind"] == 2) & on & have)
    if len(wrong):
        return f"'out' probes listed: images {wrong[:8].tolist()}, token positions {case['probe_p'][wrong[:8]].tolist()}"
    return None


# the parameter sets of the GPU file, pinned here so that the CPU file checks the conditions for every one of them
#   (P, combine, dt, lo, N): N P = 2048 and one ragged bank; lo spread over the cases (P = 64: hi + lo, where one image is 3 % of a list)
SANDWICH = [(1, "min", "f16", 0, 2048), (1, "max", "bf16", 1, 2048), (4, "min", "bf16", 0, 512), (4, "max", "f16", 1, 512),
            (16, "min", "f16", 1, 128), (16, "max", "bf16", 0, 128), (64, "min", "bf16", 1, 32), (64, "max", "f16", 1, 32),
            (4, "max", "bf16", 1, 523), (16, "min", "f16", 0, 139)]
SANDWICH_K = 8
#   (combine, dt, lo, N, pq)
STAGED = [("min", "f16", 0, 2048, False), ("max", "bf16", 1, 2059, False), ("max", "f16", 1, 2048, True), ("min", "f16", 0, 2059, True)]
STAGED_P, STAGED_K = 4, 5
#   (top_t, dt, lo)
TOPT = [(2, "f16", 0), (16, "bf16", 1)]
TOPT_P, TOPT_N, TOPT_K = 16, 128, 8
SELECTED = [("min", "f16", 0), ("max", "bf16", 1)]
SELECTED_P, SELECTED_N, SELECTED_K = 4, 1024, 2


def sandwich_case(P, combine, dt, lo, N):
    return stage_case(P, combine, dt, lo, N, SANDWICH_K)


def staged_case(combine, dt, lo, N, pq):
    return stage_case(STAGED_P, combine, dt, lo, N, STAGED_K, pq=pq, dup=True)


def topt_case(top_t, dt, lo):
    return stage_case(TOPT_P, "max", dt, lo, TOPT_N, TOPT_K, top_t=top_t)


def selected_case(combine, dt, lo):
    return stage_case(SELECTED_P, combine, dt, lo, SELECTED_N, SELECTED_K)


def selection_of(case, seed=5):
    """A 50 % random selection of the case's images with one dead tile (tile 2); QSTAR's probes stay selected."""
    rng = np.random.default_rng(seed)
    f = rng.random(case["N"]) < 0.5
    ipt = BT // case["P"]
    f[2 * ipt:3 * ipt] = False
    f[case["kind"] != 0] = True
    return f


def selected_schedule(case, flags):
    """(tiles, cum, last_live, direct_end, schedule) under the selection, from the restatement of the preparation."""
    from tests import token_prefilter_select_reference as tps
    N, P, k = case["N"], case["P"], case["k"]
    R = N * P
    _, tiles, cum, last_live = tps.prepare(np.zeros((-(-R // BT) * BT, 4), F), flags, P)
    de = tps.direct_end(cum, len(tiles), k)
    return tiles, cum, last_live, de, tr.token_schedule(N, P, k, len(tiles), de, last_live, tiles)


def selected_floor(case, flags):
    thr0 = tr.kth_finite(case["keys"][:, (case["kind"] == 0) & flags & (np.arange(case["N"]) < case["N"] * case["P"] // BT * (BT // case["P"]) // 2)], case["k"])
    assert (thr0 > -INF).all()
    return thr0
