"""NumPy statements of the five pieces of the device linear probe (sky_embeddings_amd/csrc/probe.hip, include/skyemb.h "linear-probe
fits") with their error bars: standard scaling, the softmax-regression objective and gradient (fp32 as the kernel computes it, and
fp64), the fp64 Gram, cyclic coordinate descent on the Gram, and the duality gap.  Pinned on the CPU against scikit-learn's recorded
results (tests/golden/probe.npz) by tests/test_probe_cpu.py; the kernels are compared with the fp64 statements element by element
in tests/test_probe_gpu.py.

Notation: u = 2^-24, e = 2^-53.  A sum of n terms accumulated in one format in ANY order errs by at most n (unit roundoff)
sum|terms| (first order); E_DIV = 5 u, E_EXP = E_LOG = 4 u are the allowances for fp32 division, expf and logf (2 ulp each).

Scaling (x [n, F] fp32 -> mean, var, scale fp64; out fp32).  A = sum_i |x_i| / n per column.
    mean:   n additions and a division in fp64:                     e_mean = (n + 1) e A
    var:    the kernel subtracts ITS mean; var(c) = var(mean) + (c - mean)^2 exactly, so the mean's error enters squared:
                                                                     e_var = (n + 4) e var + e_mean^2
    scale:  sqrt (half the relative error) and its own rounding:     e_scale = scale (e_var / (2 var) + 2 e), 0 where var == 0
    out:    r = (x - mean) / scale in fp64 (3 e |r| and the inputs' errors), then ONE fp32 rounding:
                                                                     e_out = u |r| + (e_mean + |r| e_scale) / scale + 4 e |r| + 2^-149
Softmax objective (X [m, F], W [K, F], b, y, l2; fp32 until the row losses).  T_ik = sum_f |x_if w_kf| + |b_k|.
    z_ik:   F fused multiply-adds in a fixed order, 6 butterfly additions, the bias:   e_z = (F + 8) u T_ik
    p_ik:   d_i = 2 max_k e_z,ik + u max_k |z_ik - mx_i| + E_EXP is the relative error of every exponential of the row; the sum of K
            of them adds K u, the division E_DIV:                    rel_p = 2 d_i + (K + 5) u
    R_ik = (p - onehot) / m:                                         e_R = (p rel_p + (1 + 5) u |p - onehot|) / m
    row loss = (log s + mx) - z_y:  log s errs by s's relative error d_i + K u and E_LOG |log s|:
                                                                     e_row = d_i + K u + E_LOG |log s| + 2 max_k e_z + 3 u (|log s| + |mx| + |z_y|)
    loss:   row losses rounded to fp32 (u |row loss|), summed and scaled in fp64:      e_loss = mean_i (e_row + u |row loss|) + small fp64 terms
    gW_kf:  chunks of ceil(m / 32) rows accumulate R x in fp32 (fmaf), the 32 partial sums are added in fp64, + l2 W, one fp32
            rounding:                  e_gW = sum_i e_R,ik |x_if| + (ceil(m / 32) + 1) u sum_i |R_ik x_if| + u |gW_kf| + 2^-149
    gb_k:   fp64 sum of the stored fp32 R, one rounding:             e_gb = sum_i e_R,ik + u |gb_k| + 2^-149
Gram (Xc [m, F] fp32, yc [m] fp32 -> G, q, ynorm2 fp64).  Inputs widen exactly; a chain of m fma's:
                                                                     e_G,ij = (m + 1) e sum_r |x_ri x_rj|   (q, ynorm2 alike)
Coordinate descent.  `enet_cd` below and the kernel perform the same fp64 operations in the same order on the same G and q (no fused
multiply-add in either; IEEE division), so every sweep is expected to agree exactly; only the reductions of the gap and of max|w|
are ordered differently, and they do not enter w.  The bar allows one unit roundoff per coordinate update of the whole fit:
                                                                     e_w = 4 sweeps F e max|w|
    and the sweep count must be equal.  gap: five sums of F terms in another order, with cancellation between them:
                                                                     e_gap = 8 F e (ynorm2 + |w.H| + 2 |q.w| + a1 |w|_1 + b2 w.w)
End to end against scikit-learn (a bar that is MEASURED, tests/golden/make_probe_golden.py): the fp64 statement of this file
(fp64 Gram of the fp32 centred features, `enet_cd`) against ElasticNet.coef_ on the golden inputs, times 4; recorded per case in
probe.npz as `<case>_enet_w_bar` = max(4 x measured, 1e-7): measured 1.2e-8 (a, 245 sweeps), 1.5e-7 (b, 8638 sweeps), 3.7e-9 and
7.3e-9 (max_iter = 3); the coefficients are O(0.1), and the sweep counts of statement and scikit-learn are equal in all four.
"""
import numpy as np

U = 2.0 ** -24
E = 2.0 ** -53
E_DIV, E_EXP, E_LOG = 5 * U, 4 * U, 4 * U
CHUNKS = 32          # SKYEMB_PROBE_CHUNKS


# ---------------------------------------------------------------------------------------------------------------- scaling
def scale_reference(x):
    """x fp32 [n, F] -> (mean, var, scale, out) in fp64 (out NOT rounded) with StandardScaler's rule scale = 1 where var == 0."""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    scale = np.where(var == 0.0, 1.0, np.sqrt(var))
    return mean, var, scale, (x - mean) / scale


def scale_bars(x):
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    mean, var, scale, r = scale_reference(x)
    e_mean = (n + 1) * E * np.abs(x).mean(axis=0)
    e_var = (n + 4) * E * var + e_mean ** 2
    e_scale = np.where(var == 0.0, 0.0, scale * (e_var / (2 * np.where(var == 0, 1, var)) + 2 * E))
    e_out = U * np.abs(r) + (e_mean + np.abs(r) * e_scale) / scale + 4 * E * np.abs(r) + 2.0 ** -149
    return e_mean, e_var, e_scale, e_out


def apply_scale_reference(x, mean, scale):
    return (np.asarray(x, np.float64) - mean) / scale


# ------------------------------------------------------------------------------------------------------ softmax objective
def softmax_objective(X, W, b, y, l2, dtype=np.float64):
    """loss = mean_i CE_i + 0.5 l2 ||W||^2 and its gradient (gW [K, F], gb [K]); the intercept is not penalised.  ``dtype`` is the
    arithmetic of the logits, softmax and residual (np.float32: as the kernel; the row losses and the gradient sums are then
    accumulated in fp64 like the kernel's).  Returns (loss, gW, gb, R)."""
    X, W, b = np.asarray(X, dtype), np.asarray(W, dtype), np.asarray(b, dtype)
    m, K = X.shape[0], W.shape[0]
    z = X @ W.T + b
    mx = z.max(axis=1, keepdims=True)
    ex = np.exp(z - mx)
    s = ex.sum(axis=1, keepdims=True)
    onehot = (np.arange(K)[None, :] == np.asarray(y)[:, None]).astype(dtype)
    R = ((ex / s - onehot) / dtype(m)).astype(dtype)
    zy = np.take_along_axis(z, np.asarray(y, np.int64)[:, None], axis=1)
    rows = ((np.log(s) + mx) - zy).astype(dtype)[:, 0]
    W64 = W.astype(np.float64)
    loss = float(rows.astype(np.float64).sum() / m + 0.5 * l2 * (W64 * W64).sum())
    gW = R.astype(np.float64).T @ X.astype(np.float64) + l2 * W64
    gb = R.astype(np.float64).sum(axis=0)
    return loss, gW, gb, R


def softmax_bars(X, W, b, y, l2):
    """(e_loss, e_gW [K, F], e_gb [K]) of the kernel against softmax_objective(..., np.float64), from the inputs alone."""
    X, W, b = np.asarray(X, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    m, F = X.shape
    K = W.shape[0]
    z = X @ W.T + b
    T = np.abs(X) @ np.abs(W).T + np.abs(b)
    e_z = (F + 8) * U * T
    mx = z.max(axis=1, keepdims=True)
    ex = np.exp(z - mx)
    s = ex.sum(axis=1, keepdims=True)
    p = ex / s
    onehot = (np.arange(K)[None, :] == np.asarray(y)[:, None]).astype(np.float64)
    d = 2 * e_z.max(axis=1, keepdims=True) + U * np.abs(z - mx).max(axis=1, keepdims=True) + E_EXP
    rel_p = 2 * d + (K + 5) * U
    e_R = (p * rel_p + 6 * U * np.abs(p - onehot)) / m
    zy = np.take_along_axis(z, np.asarray(y, np.int64)[:, None], axis=1)
    logs = np.log(s)
    rows = logs + mx - zy
    e_row = d + K * U + E_LOG * np.abs(logs) + 2 * e_z.max(axis=1, keepdims=True) + 3 * U * (np.abs(logs) + np.abs(mx) + np.abs(zy))
    e_loss = float((e_row + U * np.abs(rows)).mean() + 16 * E * (abs(rows.mean()) + l2 * (W * W).sum()))
    R = (p - onehot) / m
    gW = R.T @ X + l2 * W
    rpc = -(-m // CHUNKS)
    e_gW = e_R.T @ np.abs(X) + (rpc + 1) * U * (np.abs(R).T @ np.abs(X)) + U * np.abs(gW) + 2.0 ** -149
    e_gb = e_R.sum(axis=0) + U * np.abs(R.sum(axis=0)) + 2.0 ** -149
    return e_loss, e_gW, e_gb


# ------------------------------------------------------------------------------------------------------------------ Gram
def gram_reference(Xc, yc, dtype=np.float64):
    """(G, q, ynorm2) of the fp32 inputs; dtype = np.float32 is the statement the issue warns about (an fp32 Gram)."""
    Xc, yc = np.asarray(Xc, np.float32).astype(dtype), np.asarray(yc, np.float32).astype(dtype)
    return (Xc.T @ Xc).astype(np.float64), (Xc.T @ yc).astype(np.float64), float(yc.astype(np.float64) @ yc.astype(np.float64))


def gram_bars(Xc, yc):
    A, y = np.abs(np.asarray(Xc, np.float64)), np.abs(np.asarray(yc, np.float64))
    m = A.shape[0]
    return (m + 1) * E * (A.T @ A), (m + 1) * E * (A.T @ y), (m + 1) * E * float(y @ y)


# ---------------------------------------------------------------------------------------------------- coordinate descent
def enet_gap(G, q, ynorm2, w, H, a1, b2):
    """The duality gap of scikit-learn's enet_coordinate_descent_gram (alpha = a1, beta = b2)."""
    qw = float(w @ q)
    dn = float(np.abs((q - H) - b2 * w).max())
    R2 = (ynorm2 + float(w @ H)) - 2.0 * qw
    if dn > a1:
        c = a1 / dn
        gap = 0.5 * (R2 + R2 * (c * c))
    else:
        c = 1.0
        gap = R2
    return gap + (((a1 * float(np.abs(w).sum()) - c * ynorm2) + c * qw) + (0.5 * b2) * (1.0 + c * c) * float(w @ w))


def enet_gap_bar(G, q, ynorm2, w, H, a1, b2):
    F = w.size
    return 8 * F * E * (ynorm2 + abs(float(w @ H)) + 2 * abs(float(w @ q)) + a1 * float(np.abs(w).sum()) + b2 * float(w @ w))


def enet_cd(G, q, ynorm2, a1, b2, max_iter, tol):
    """Cyclic coordinate descent from w = 0 on (G, q) in fp64, the kernel's operations in the kernel's order.
    -> (w, sweeps, converged, gap)."""
    G, q = np.asarray(G, np.float64), np.asarray(q, np.float64)
    F = q.size
    w, H = np.zeros(F), np.zeros(F)
    dg = np.diag(G).copy()
    gap, tolg = tol + 1.0, tol * ynorm2
    for it in range(max_iter):
        dwmax = 0.0
        for j in range(F):
            d = dg[j]
            if d == 0.0:
                continue
            wj = w[j]
            t = (q[j] - H[j]) + wj * d
            at = abs(t) - a1
            wn = np.copysign(at, t) / (d + b2) if at > 0.0 else 0.0
            if wn != wj:
                dlt = wn - wj
                w[j] = wn
                H = H + dlt * G[j]
                dwmax = max(dwmax, abs(dlt))
        wmax = float(np.abs(w).max())
        if wmax == 0.0 or dwmax / wmax < tol or it == max_iter - 1:
            gap = enet_gap(G, q, ynorm2, w, H, a1, b2)
            if gap < tolg:
                return w, it + 1, True, gap
    return w, max_iter, False, gap


def enet_w_bar(w, sweeps):
    return 4 * sweeps * w.size * E * float(np.abs(w).max()) + 2.0 ** -1074


def enet_fit_reference(X, y, alpha, l1_ratio, max_iter, tol, gram_dtype=np.float64):
    """ElasticNet(fit_intercept=True) restated: centre in fp64, round the centred data to fp32 (what the device path stores), Gram,
    coordinate descent, intercept.  -> (coef, intercept, sweeps, converged, gap)."""
    X64, y64 = np.asarray(X, np.float64), np.asarray(y, np.float64)
    m = X64.shape[0]
    xm, ym = X64.mean(axis=0), y64.mean()
    Xc, yc = (X64 - xm).astype(np.float32), (y64 - ym).astype(np.float32)
    G, q, yn = gram_reference(Xc, yc, gram_dtype)
    w, sweeps, conv, gap = enet_cd(G, q, yn, alpha * l1_ratio * m, alpha * (1.0 - l1_ratio) * m, max_iter, tol)
    return w, float(ym - xm @ w), sweeps, conv, gap


# ------------------------------------------------------------------------------------------------------- softmax fit
def fit_softmax_reference(X, y, K, C=0.01, max_iter=10000, tol=1e-4, dtype=np.float32):
    """scikit-learn's optimiser call on the statement above, from zeros.  -> (W [K, F], b [K], iterations)."""
    from scipy.optimize import minimize
    m, F = X.shape
    l2 = 1.0 / (C * m)

    def fun(p):
        W, b = p[:K * F].reshape(K, F), p[K * F:]
        if dtype == np.float32:
            W, b = W.astype(np.float32), b.astype(np.float32)
        loss, gW, gb, _ = softmax_objective(X, W, b, y, l2, dtype)
        return loss, np.concatenate([gW.ravel(), gb]).astype(np.float64)
    res = minimize(fun, np.zeros(K * F + K), method="L-BFGS-B", jac=True,
                   options=dict(maxiter=max_iter, maxls=50, gtol=tol, ftol=64 * np.finfo(float).eps))
    return res.x[:K * F].reshape(K, F), res.x[K * F:], int(res.nit)


def r2_score(y, pred):
    y, pred = np.asarray(y, np.float64), np.asarray(pred, np.float64)
    return float(1.0 - ((y - pred) ** 2).sum() / ((y - y.mean()) ** 2).sum())
