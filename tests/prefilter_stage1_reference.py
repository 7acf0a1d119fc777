"""Plain statements (numpy, float64 and integers) of what STAGE 1 of the two-stage many-query search must compute, quantity by
quantity -- the row constants and the fp16 image, the query images and constants, every matrix-core dot product, the candidate
lists at a known threshold, the thresholds -- for the per-pair tests of tests/test_prefilter_stage1_{cpu,gpu}.py.  The file under
test is csrc/topk_prefilter.hip; its header derives the bound these statements serve.  The token route is covered image by image in
tests/token_prefilter_stage_reference.py, which builds on this file.

Formats (``fmt``): 'fp32' an fp32 bank searched through its scaled fp16 image (bank16_kernel), 'fp16' a resident fp16 bank
(bank16_rowp_lp_kernel), 'bf16' a resident bf16 bank (bankbf16_rowp_kernel).  A 16-bit value is carried as the float32 it widens
to; images are compared as 16-bit patterns.  Checkers return None or a reason string."""
import functools
import math

import numpy as np
import torch

from tests import prefilter_bf16_reference as bfr
from tests import prefilter_lp_reference as lpr

FMTS = ("fp32", "fp16", "bf16")
BT, QPAD, GQ, RESCORE_MAX, SCAP = 256, 256, 5, 256, 2048
EPS = 1e-6
U = 2.0 ** -24                       # one fp32 rounding to nearest, relative
INF = float("inf")


def qtile(lo):
    return 128 if lo else 256


def cap_of(k):
    return 4096 if k <= 128 else 8192


def eps_a(fmt, D, lo):
    """eps_a_of / eps_a_bf16_of of the file under test, restated (the CPU test holds it to the library's own value)."""
    acc = 6.06 * D * 2.0 ** -24
    if fmt == "bf16":
        return (2.0 ** -18 if lo else 2.0 ** -9) + acc + D * 2.0 ** -38
    if fmt == "fp16":
        return (2.0 ** -21 if lo else 2.0 ** -11 + 2.0 ** -21) + acc + math.sqrt(D) * 2.0 ** -27
    return (2.0 ** -11 + 2.0 ** -21 if lo else 2.0 ** -10 + 2.0 ** -21) + acc + 2.0 * math.sqrt(D) * 2.0 ** -27


def eps_a_f32(fmt, D, lo):
    """The float the driver hands to query16_kernel: eps_a raised by 1e-6, rounded once."""
    return np.float32(eps_a(fmt, D, lo) * (1.0 + 1e-6))


def sum_roundings(D):
    """fp32 roundings on the way to a wave's sum of squares: a lane owns 4 elements of every 256 (one fma each), then the wave
    reduction adds six times.  All terms are >= 0, so the sum is within (1 + U) ** sum_roundings of the exact one, either way."""
    return 4 * ((D + 255) // 256) + 6


def bits16(a, fmt):
    """16-bit patterns of an operand array: fp16 as stored; bf16 = the upper half of the float32 it is carried as."""
    if fmt == "bf16":
        return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def widen16(u, fmt):
    """float32 values of 16-bit patterns."""
    u = np.ascontiguousarray(u, dtype=np.uint16)
    if fmt == "bf16":
        return (u.astype(np.uint32) << 16).view(np.float32)
    return u.view(np.float16).astype(np.float32)


def f32bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------- the driver's schedule
def schedule(N, k, thr0, resident, n_live=None, last_live=0):
    """topk_prefiltered's launches as a pure function of (N, k, thr0 given?, resident?, the selection's live tiles): a list of
    ('mode0' | 'mode1' | 'mode2', t0, t1), ('tail', tile) and ('select', final) in launch order, and the inputs the issue names:
    first, direct_end, ends, has_tail, T.  (t0 == t1 is a launch over no tile: the driver clips a slice's end to T only AFTER it
    has compared it with t0, so a bank of exactly `first` tiles gets one empty direct launch and a second final select.)"""
    cap = cap_of(k)
    sel = n_live is not None
    ragged = resident and N % BT != 0
    T_tail = N // BT
    has_tail = ragged and (not sel or bool(last_live))
    T = n_live - (1 if ragged and last_live else 0) if sel else (T_tail if resident else -(-N // BT))
    first = min(max(cap // 2 // BT, 1), T)
    direct_end = max(-(-96 * k // BT), T // 128, first + 1)
    ends = [first, direct_end, T // 32, T // 8, T // 2, T]
    first_rows = first * BT if sel or first * BT < N else N
    out, t0, thresholded, tail_done = [], 0, thr0, False
    for p, t1 in enumerate(ends):
        if p == 0 and thr0:
            continue
        if t1 <= t0:
            continue
        t1 = min(t1, T)
        if p == 0:
            out.append(("mode0", t0, t1))
        elif not thresholded:
            out.append(("mode1", t0, t1))
            thresholded = True
        else:
            out.append(("mode2", t0, t1))
        if has_tail and t1 == T and not tail_done:
            tail_done = True
            out.append(("tail", T_tail))
        out.append(("select", int(t1 == T)))
        t0 = t1
    return dict(launches=out, first=first, direct_end=direct_end, ends=ends, has_tail=has_tail, T=T, first_rows=first_rows, cap=cap)


# ------------------------------------------------------------------------------------------------------------------ row constants
def row_constants(x, xn, fmt, D):
    """What the preparation kernel of `fmt` must leave for the rows x [N, D] (float32 values; of a 16-bit bank the widened ones)
    with weighted norms xn [N]: rowp[i] = {xn 2^-e, nx', 2^-e, 0}.

      e        fp32: the row maximum (NaNs skipped, as fmaxf skips them) times 2^-e lies in [2^13, 2^14); resident banks: 0
      image    fp32 only, BIT-EXACT: x * 2^-e (one fp32 multiply by a power of two) rounded once to fp16
      norm     ||x 2^-e||_2 in float64
      nx_lo    the least nx' the proof accepts: norm, plus for a resident fp16 row with nsub fp16-subnormal elements the header's
               additive term sqrt(nsub) 2^-14 / eps_a(hi + lo)
      nx_hi    the most a correct kernel can produce: (norm (1 + D 2^-22) + the term (1 + 1e-6)(1 + U)) (1 + 2^-21)(1 + 2^-22)
               times (1 + U) ** (sum_roundings(D) / 2 + 4) -- the roundings of the sum of squares, halved by the square root, and
               one each for sqrtf, the product with 1 + D 2^-22, the fma of the subnormal term, the product with 1 + 2^-21
      unb      rows that take {0, inf, 1, 0}: fp32 -- an infinite element, or a maximum below 2^-113 (e < -126: 2^-e would leave
               fp32); fp16 -- an inf or NaN element; bf16 -- an inf / NaN element, a nonzero element outside [2^-60, 2^120), or
               a weighted norm that is not finite
      nanrow   fp32 only: a NaN element and no infinite one.  The kernel's maximum skips the NaN, so the row is scaled like any
               other and its NaN reaches the image and nx'.  Its exact score is -inf whatever the query, so keeping it for every
               query and dropping it for every query are both right; what must not happen is a FINITE nx'."""
    assert fmt in FMTS
    x = np.asarray(x, dtype=np.float32)
    xn = np.asarray(xn, dtype=np.float32)
    N = x.shape[0]
    assert x.shape == (N, D) and xn.shape == (N,)
    a = np.abs(x.astype(np.float64))
    isnan = np.isnan(a)
    mx = np.where(isnan, 0.0, a).max(axis=1)
    e = np.zeros(N, dtype=np.int64)
    nanrow = np.zeros(N, dtype=bool)
    with np.errstate(invalid="ignore"):
        if fmt == "fp32":
            ok = (mx > 0) & (mx < INF)
            e[ok] = np.frexp(mx[ok])[1] - 14
            unb = ~(mx < INF) | (e < -126)
            nanrow = isnan.any(axis=1) & ~unb
        elif fmt == "fp16":
            unb = ~(a < INF).all(axis=1)
        else:
            unb = bfr.unboundable(x) | ~(xn.astype(np.float64) < INF)
    e[unb] = 0
    scale = np.ldexp(np.float32(1.0), -e).astype(np.float32)
    with np.errstate(all="ignore"):
        xs32 = x * scale[:, None]                                   # fp32, exact up to underflow: the kernel's own multiply
        image = None
        if fmt == "fp32":
            image = xs32.astype(np.float16)
            image[unb] = 0
        xn_s = xn * scale
        xn_s[unb] = 0
        xs = np.where(unb[:, None], 0.0, x.astype(np.float64) * np.ldexp(1.0, -e)[:, None])
        norm = np.sqrt((xs * xs).sum(axis=1))
    term = np.zeros(N)
    if fmt == "fp16":
        term = np.sqrt(lpr.count_subnormals(x.astype(np.float16)).astype(np.float64)) * 2.0 ** -14 / eps_a("fp16", D, True)
        term[unb] = 0
    nx_lo = norm + term
    nx_hi = ((norm * (1 + D * 2.0 ** -22) + term * (1 + 1e-6) * (1 + U)) * (1 + 2.0 ** -21) * (1 + 2.0 ** -22)
             * (1 + U) ** (sum_roundings(D) / 2 + 4))
    nx_lo[unb], nx_hi[unb] = INF, INF
    return dict(fmt=fmt, N=N, D=D, e=e, scale=scale, xn_s=xn_s, image=image, norm=norm, nx_lo=nx_lo, nx_hi=nx_hi, unb=unb, nanrow=nanrow)


def model_rowp(ref, rows_padded):
    """A rowp array that meets the statement (nx' = the float just above norm (1 + D 2^-22) + term): what the checkers accept, and
    the material for the planted defects of the CPU test."""
    N, D = ref["N"], ref["D"]
    rp = np.zeros((rows_padded, 4), dtype=np.float32)
    rp[N:, 1] = np.nan
    with np.errstate(all="ignore"):
        want = ref["norm"] * (1 + D * 2.0 ** -22) + (ref["nx_lo"] - ref["norm"])
        nx = want.astype(np.float32)
        nx = np.where(nx.astype(np.float64) < want, np.nextafter(nx, np.float32(INF)), nx)
    rp[:N, 0], rp[:N, 1], rp[:N, 2] = ref["xn_s"], nx, ref["scale"]
    rp[:N][ref["unb"]] = (0.0, INF, 1.0, 0.0)
    rp[:N, 1][ref["nanrow"]] = np.nan
    return rp


def check_rowp(rowp, ref):
    """rowp [rows_padded, 4] float32 as the device left it against row_constants' statement."""
    N = ref["N"]
    rowp = np.asarray(rowp, dtype=np.float32)
    b = f32bits(rowp)
    pad = rowp[N:]
    if len(pad) and not ((b[N:, [0, 2, 3]] == 0).all() and np.isnan(pad[:, 1]).all()):
        bad = N + int(np.argmax(~((b[N:, [0, 2, 3]] == 0).all(axis=1) & np.isnan(pad[:, 1]))))
        return f"padding row {bad} is not the sentinel {{0, NaN, 0, 0}}: {rowp[bad]}"
    want_unb = f32bits(np.array([0.0, INF, 1.0, 0.0], dtype=np.float32))
    for i in np.flatnonzero(ref["unb"]):
        if not (b[i] == want_unb).all():
            return f"unboundable row {i} must hold {{0, inf, 1, 0}}, holds {rowp[i]}"
    rows = np.flatnonzero(~ref["unb"])
    z_ok = b[rows, 2] == f32bits(ref["scale"][rows])
    if not z_ok.all():
        i = rows[np.argmin(z_ok)]
        return f"row {i}: 2^-e is {rowp[i, 2]}, expected {ref['scale'][i]}"
    if (b[rows, 3] != 0).any():
        return f"row {rows[np.argmax(b[rows, 3] != 0)]}: the fourth component is not +0"
    xs = ref["xn_s"][rows]
    x_ok = (b[rows, 0] == f32bits(xs)) | (np.isnan(xs) & np.isnan(rowp[rows, 0]))
    if not x_ok.all():
        i = rows[np.argmin(x_ok)]
        return f"row {i}: xn 2^-e is {rowp[i, 0]!r}, expected {ref['xn_s'][i]!r}"
    nan = ref["nanrow"][rows]
    nx = rowp[rows, 1].astype(np.float64)
    if np.isfinite(nx[nan]).any():
        return f"row {rows[nan][np.argmax(np.isfinite(nx[nan]))]} has a NaN element and a finite nx'"
    with np.errstate(invalid="ignore"):
        low = ~nan & ~(nx >= ref["nx_lo"][rows])
        high = ~nan & ~(nx <= ref["nx_hi"][rows])
    if low.any():
        i = rows[np.argmax(low)]
        return f"row {i}: nx' = {rowp[i, 1]!r} is below the row's norm (+ subnormal term) {ref['nx_lo'][i]!r}: not an upper bound"
    if high.any():
        i = rows[np.argmax(high)]
        return f"row {i}: nx' = {rowp[i, 1]!r} exceeds what the roundings allow, {ref['nx_hi'][i]!r}"
    return None


def same16(got, want):
    """Bit equality of two uint16 pattern arrays; -> None or the first difference."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    d = np.argwhere(got != want)
    return None if len(d) == 0 else f"{len(d)} elements differ, first at {tuple(d[0])}: {int(got[tuple(d[0])]):#06x} != {int(want[tuple(d[0])]):#06x}"


def check_image(img_bits, ref):
    """The fp16 image [rows_padded, D] (uint16 patterns) of an fp32 bank: bit-equal to the statement (any NaN equals any NaN),
    zero in the padding rows."""
    N = ref["N"]
    img_bits = np.asarray(img_bits, dtype=np.uint16)
    if (img_bits[N:] != 0).any():
        return f"padding rows of the image are not zero (row {N + int(np.argwhere(img_bits[N:] != 0)[0][0])})"
    want = ref["image"].view(np.uint16)
    nan = np.isnan(ref["image"])
    got = np.where(nan & np.isnan(img_bits[:N].view(np.float16)), want, img_bits[:N])
    return same16(got, want)


# -------------------------------------------------------------------------------------------------------------- query constants
def query_constants(tw, qn, fmt, D, eps_a32):
    """What query16_kernel must leave for the weighted queries tw [Q, D] with norms qn [Q]: the images qh, ql (16-bit patterns, the
    operand format of `fmt`: fp16 for 'fp32' and 'fp16', bf16 for 'bf16') and qbase = {qn 2^-f, y, 2^-f, qn}, exact but for y:
      y_lo = eps_a ||q'||_2 in float64 (eps_a the float handed over), the least the proof accepts;
      y_hi = y_lo (1 + D 2^-22) (1 + U) ** (sum_roundings(D) / 2 + 3): the sum of squares, sqrtf, the two products.
    flagged: the queries init_state_kernel must hand to the exact route (scale clamped / outside the bf16 window)."""
    tw = np.asarray(tw, dtype=np.float32)
    qn = np.asarray(qn, dtype=np.float32)
    Q = tw.shape[0]
    split = bfr.scale_query if fmt == "bf16" else lpr.scale_query
    ofmt = "bf16" if fmt == "bf16" else "fp16"
    qh = np.zeros((Q, D), dtype=np.uint16)
    ql = np.zeros((Q, D), dtype=np.uint16)
    s = np.zeros(Q, dtype=np.float32)
    norm = np.zeros(Q)
    for q in range(Q):
        qp, h, l, sq = split(tw[q])
        qh[q], ql[q], s[q] = bits16(h, ofmt), bits16(l, ofmt), sq
        norm[q] = math.sqrt(float((qp.astype(np.float64) ** 2).sum()))
    with np.errstate(all="ignore"):
        qn_s = qn * s
    y_lo = float(np.float32(eps_a32)) * norm
    y_hi = y_lo * (1 + D * 2.0 ** -22) * (1 + U) ** (sum_roundings(D) / 2 + 3)
    flagged = ~((s > 2.0 ** -100) & (s < 2.0 ** 30)) if fmt == "bf16" else s >= 2.0 ** 126
    return dict(fmt=fmt, Q=Q, D=D, qh=qh, ql=ql, s=s, qn_s=qn_s, qn=qn, norm=norm, y_lo=y_lo, y_hi=y_hi, flagged=flagged)


def model_qbase(ref):
    qb = np.zeros((ref["Q"], 4), dtype=np.float32)
    want = ref["y_lo"] * (1 + ref["D"] * 2.0 ** -22)
    y = want.astype(np.float32)
    y = np.where(y.astype(np.float64) < want, np.nextafter(y, np.float32(INF)), y)
    qb[:, 0], qb[:, 1], qb[:, 2], qb[:, 3] = ref["qn_s"], y, ref["s"], ref["qn"]
    return qb


def check_query(qh, ql, qbase, ref, lo=None):
    """qh, ql [Qp, D] uint16 patterns, qbase [Q, 4] float32 as the device left them.  lo (hi + lo searches): ql is held to the
    statement as ever; the argument only words the message."""
    Q = ref["Q"]
    for name, got, want in (("qh", qh, ref["qh"]), ("ql", ql, ref["ql"])):
        got = np.asarray(got, dtype=np.uint16)
        if (got[Q:] != 0).any():
            return f"{name}: padding rows are not zero"
        r = same16(got[:Q], want)
        if r:
            return f"{name}: {r}" + (" (the second pass of a hi + lo search multiplies this image)" if lo and name == "ql" else "")
    qbase = np.asarray(qbase, dtype=np.float32)
    b = f32bits(qbase)
    for c, name, want in ((0, "qn 2^-f", ref["qn_s"]), (2, "2^-f", ref["s"]), (3, "qn", ref["qn"])):
        ok = b[:, c] == f32bits(want)
        if not ok.all():
            q = int(np.argmin(ok))
            return f"qbase[{q}].{'xyzw'[c]} ({name}) is {qbase[q, c]!r}, expected {want[q]!r}"
    y = qbase[:, 1].astype(np.float64)
    if not (y >= ref["y_lo"]).all():
        q = int(np.argmin(y >= ref["y_lo"]))
        return f"qbase[{q}].y = {qbase[q, 1]!r} is below eps_a ||q'|| = {ref['y_lo'][q]!r}: the half-width is not a bound"
    if not (y <= ref["y_hi"]).all():
        q = int(np.argmin(y <= ref["y_hi"]))
        return f"qbase[{q}].y = {qbase[q, 1]!r} exceeds eps_a ||q'|| (1 + D 2^-22) and its roundings, {ref['y_hi'][q]!r}"
    return None


def check_flags(overflow, redo, ref):
    overflow, redo = np.asarray(overflow), np.asarray(redo)
    if not np.array_equal(overflow != 0, ref["flagged"]):
        q = int(np.argmax((overflow != 0) != ref["flagged"]))
        return f"overflow[{q}] = {overflow[q]}, expected {int(ref['flagged'][q])} (2^-f = {ref['s'][q]!r})"
    if not (redo[ref["flagged"]] == 1).all():
        return "a flagged query came back with redo = 0"
    return None


# --------------------------------------------------------------------------------------------------------- inputs on an integer grid
def exact_grid_case(fmt, lo, Q, N, D, seed):
    """Inputs whose dot^ is defined TO THE BIT.  Row i is m_i 2^g_i with integers m in -3 .. 3 (every row has a nonzero one); query
    q is q' 2^f_q with q' = H + L on a grid of the operand format:
      fp16 operands   H = 8 h, 1025 <= |h| <= 2047 (11-bit significands inside (2^13, 2^14), where query16_kernel puts the
                      largest element: here all of them; not 2^13 itself, below which the grid is finer), L in +-{1, 2, 3} -- below half a unit of H, so qh = H, ql = L;
      bf16 operands   H = h 2^-28, 129 <= |h| <= 255 (8-bit significands inside (2^-21, 2^-20)), L = l 2^-32, l in +-{1 .. 7}.
    Bit budget: in units of 1 (fp16) / 2^-32 (bf16) and of the row's power of two, |q'_d| <= 8 * 2047 + 3 < 2^14 / 16 * 255 + 7 <
    2^12, |m_d| <= 3, and every product, whichever of H, L or H + L it is taken of, is an integer with
        sum_d |H_d m_d| + |L_d m_d| <= 3 D (8 * 2047 + 3) = 49 137 D   (fp16)        3 D (16 * 255 + 7) = 12 261 D   (bf16),
    below 2^24 for D <= 341 and D <= 1368: every partial sum, in any order and however the passes interleave, is an integer of
    magnitude below 2^24 times a power of two -- an fp32 number.  No rounding or truncation can occur, so dot^ is the integer dot
    product.  The function asserts that budget for the arrays it returns.
    -> dict(tw, x (float32 values), dot (float32 [Q, N]: the exact dot^ under `lo`), dot_other (the other pass count's), H, L)."""
    bf = fmt == "bf16"
    rng = np.random.default_rng(seed)
    m = rng.integers(-3, 4, size=(N, D))
    m[np.arange(N), rng.integers(0, D, size=N)] = 3 - 2 * (np.arange(N) % 3 == 0)       # a known nonzero entry: 3 or 1
    g = rng.integers(*{"fp32": (-8, 9), "fp16": (-4, 5), "bf16": (-12, 13)}[fmt], size=N)
    x = np.ldexp(m.astype(np.float32), g[:, None]).astype(np.float32)
    if bf:
        h = rng.integers(129, 256, size=(Q, D)) * rng.choice([-1, 1], size=(Q, D))
        l = rng.integers(1, 8, size=(Q, D)) * rng.choice([-1, 1], size=(Q, D))
        Hi, Li, qexp = 16 * h, l, -32
    else:
        h = rng.integers(1025, 2048, size=(Q, D)) * rng.choice([-1, 1], size=(Q, D))
        l = rng.integers(1, 4, size=(Q, D)) * rng.choice([-1, 1], size=(Q, D))
        Hi, Li, qexp = 8 * h, l, 0
    f = rng.integers(-5, 6, size=Q)
    tw = np.ldexp((Hi + Li).astype(np.float32), (qexp + f)[:, None]).astype(np.float32)
    # the row's unit in the operand stage 1 multiplies: the image of an fp32 row is m 2^12 (largest |m| 2 or 3) or m 2^13 (1)
    rexp = np.where(np.abs(m).max(axis=1) == 1, 13, 12) if fmt == "fp32" else g
    # ---- the exactness condition, in integers
    worst = int((np.abs(Hi).astype(np.int64) + np.abs(Li)).max(axis=0).sum()) * int(np.abs(m).max())   # sum_d max_q (|H_d| + |L_d|) * max |m|
    assert worst < 2 ** 24, (fmt, D, worst)
    assert int(np.abs(Hi + Li).max()) < 2 ** 24                           # q' itself is an fp32 number
    assert (2 * np.abs(Li) < (16 if bf else 8)).all()                     # L below half a unit of H: the split recovers H and L
    dots = []
    for part in ((Hi + Li), Hi):
        d = part.astype(np.float64) @ m.T.astype(np.float64)               # integers below 2^24: exact
        assert float(np.abs(d).max()) < 2 ** 24 and (d == np.rint(d)).all()
        dots.append(np.ldexp(d, (rexp + qexp)[None, :]).astype(np.float32))
        assert (dots[-1].astype(np.float64) == np.ldexp(d, (rexp + qexp)[None, :])).all()
    both, hi_only = dots
    assert (both != hi_only).any(axis=1).all()                            # the two pass counts give different exact answers
    return dict(fmt=fmt, tw=tw, x=x, dot=both if lo else hi_only, dot_other=hi_only if lo else both,
                H=np.ldexp(Hi.astype(np.float32), qexp), L=np.ldexp(Li.astype(np.float32), qexp), rexp=rexp, f=f)


# ----------------------------------------------------------------------------------------------------------------- scores, sandwich
def den32(qn, xn, eps=EPS):
    """fmaf(qn, xn, eps) [Q, N] as fp32 (the product of two floats is exact in float64)."""
    with np.errstate(all="ignore"):
        return (np.asarray(qn, np.float32).astype(np.float64)[:, None] * np.asarray(xn, np.float32).astype(np.float64)[None, :]
                + float(np.float32(eps))).astype(np.float32)


def scores64(tw, x, qn, xn, eps=EPS):
    """The exact score of every pair in float64: sum_d tw_d x_d over the contract's denominator."""
    with np.errstate(all="ignore"):
        return (np.asarray(tw, np.float32).astype(np.float64) @ np.asarray(x, np.float32).astype(np.float64).T) / den32(qn, xn, eps).astype(np.float64)


def chain_all(tw, x, threads=None):
    """prefilter_lp_reference.fma_chain for every (query, row) pair at once [Q, N] (float64 step, rounded to fp32 each time); torch
    on the CPU only because its element-wise kernels use every core."""
    t = torch.from_numpy(np.ascontiguousarray(tw, dtype=np.float32)).double()
    xx = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).double().t().contiguous()      # [D, N]
    acc = torch.zeros(t.shape[0], xx.shape[1], dtype=torch.float32)
    for d in range(t.shape[1]):
        acc = torch.addcmul(acc.double(), t[:, d:d + 1], xx[d:d + 1]).float()
    return acc.numpy()


def half_width(qref, rref, den, upper=True):
    """hw [Q, N]: eps_a ||q'|| nx' expressed as a score, (y / 2^-f) (nx' / 2^-e) / den, from the largest (upper) or the least
    constants the statements allow."""
    y, nx = (qref["y_hi"], rref["nx_hi"]) if upper else (qref["y_lo"], rref["nx_lo"])
    with np.errstate(all="ignore"):
        return (y / qref["s"].astype(np.float64))[:, None] * (nx / rref["scale"].astype(np.float64))[None, :] / np.asarray(den, np.float64)


def sandwich(tau, score, hw, contract=None):
    """For thresholds tau [Q] that the kernels KNEW (a caller's floor, or the tau the search published): which rows a query's list
    must hold and which it must not.
      must-be-in    score >= tau, the float64 exact score: the property the proof needs (the real dot product lies inside the
                    interval around dot^ as the fp32 chain does: the chain's own roundings are a term of eps_a).
      must-be-out   score < tau - 2 hw - slack.  A listed pair passed `dot^ + c nx' >= a xn' + b se` (prefilter_kernel) or `U >= tau`
                    (select_kernel's compaction).  The first is evaluated with a, b lowered and c raised by 2^-19 relative and an fp32
                    chain whose error the kernel comment bounds by 2^-19 (|a xn'| + |b se| + |c nx'|); in score units |a xn' + b se|
                    is |tau| and c nx' is hw, so passing implies dot^ as a score >= tau - hw - 2 * 2^-19 (|tau| + hw), and dot^ as a
                    score is at most score + hw: score >= tau - 2 hw - 2^-18 (|tau| + hw).  The second widens U by 2^-21 relative
                    after four fp32 operations (2^-22 together) on a value next to tau: 2^-20 (|tau| + hw) covers it.  Both fit
                    slack = 2^-17 (|tau| + hw), twice their sum's leading term: derived from the factors, not from any output.
    contract (the oracle's fp32 scores [Q, N]): a row whose CONTRACT score is >= tau must be in as well -- that is the proof's own
    wording, and a floor that is the contract score of some row (the MODE 2 case's) is reached by that row whichever way its
    float64 score rounds.
    Rows in between are don't-care; a pair whose score or half-width is NaN / inf is never must-be-out.
    -> (must_in, must_out) boolean [Q, N]."""
    tau = np.asarray(tau, np.float64)[:, None]
    with np.errstate(all="ignore"):
        slack = 2.0 ** -17 * (np.abs(tau) + hw)
        must_in = score >= tau
        if contract is not None:
            must_in = must_in | (np.asarray(contract, np.float64) >= tau)
        must_out = score < tau - 2 * hw - slack
    assert not (must_in & must_out).any()
    return must_in, must_out


def check_sandwich(lists, must_in, must_out, allowed=None):
    """lists: per query the row numbers of its final list.  No duplicates, nothing outside `allowed` (a selection), every
    must-be-in row present, no must-be-out row present."""
    N = must_in.shape[1]
    for q, rows in enumerate(lists):
        rows = np.asarray(rows, dtype=np.int64)
        if len(rows) and (rows.min() < 0 or rows.max() >= N):
            return f"query {q}: a listed row lies outside [0, {N})"
        if len(np.unique(rows)) != len(rows):
            return f"query {q}: a row is listed twice"
        have = np.zeros(N, dtype=bool)
        have[rows] = True
        if allowed is not None and (have & ~allowed).any():
            return f"query {q}: deselected row {int(np.argmax(have & ~allowed))} is listed"
        miss = must_in[q] & ~have
        if miss.any():
            return f"query {q}: row {int(np.argmax(miss))} scores at or above the threshold and is not in the list"
        extra = must_out[q] & have
        if extra.any():
            return f"query {q}: row {int(np.argmax(extra))} lies more than the interval below the threshold and is in the list"
    return None


def check_take_all(cnt, cand_i, cand_d, dot, nslots, slot_rows=None):
    """A take-all slice left as it was stored: cnt[q] >= nslots, slot r of every query holds row r (or slot_rows[r] under a
    selection) and -- where `dot` gives one (not NaN) -- exactly that dot^."""
    Q = dot.shape[0]
    want = np.arange(nslots) if slot_rows is None else np.asarray(slot_rows)
    if (np.asarray(cnt) < nslots).any():
        return f"cnt[{int(np.argmax(np.asarray(cnt) < nslots))}] is below the {nslots} slots of the take-all slice"
    ci = np.asarray(cand_i)[:Q, :nslots]
    if not (ci == want[None, :]).all():
        q, r = np.argwhere(ci != want[None, :])[0]
        return f"cand_i[{q}][{r}] = {ci[q, r]}, expected row {want[r]}"
    return check_dots(np.asarray(cand_d)[:Q, :nslots], dot[:, want])


def check_dots(got, want):
    """dot^ bit for bit (a NaN in `want` = no statement for that pair)."""
    g, w = f32bits(got), f32bits(want)
    bad = (g != w) & ~np.isnan(want)
    if bad.any():
        q, r = np.argwhere(bad)[0]
        return f"{int(bad.sum())} of {bad.size} dot^ differ, first at query {q}, slot {r}: {got[q, r]!r} != {want[q, r]!r}"
    return None


def check_tail_appends(cnt, cand_i, cand_d, dot, first_rows, N):
    """Behind a take-all slice of first_rows slots: rows first_rows .. N-1, each exactly once, in any order, with their dot^."""
    for q in range(dot.shape[0]):
        if cnt[q] != N:
            return f"cnt[{q}] = {cnt[q]}, expected every one of the {N} rows"
        rows = np.asarray(cand_i[q, first_rows:N], dtype=np.int64)
        if not np.array_equal(np.sort(rows), np.arange(first_rows, N)):
            return f"query {q}: the appended rows are not rows {first_rows} .. {N - 1} once each (a padding row or a duplicate?)"
        r = check_dots(np.asarray(cand_d[q, first_rows:N])[None, :], dot[q, rows][None, :])
        if r:
            return f"query {q} (appended rows): {r}"
    return None


def check_pair_bound(dot_hat, chain_scaled, y, nx):
    """|dot^ - chain 2^-(e+f)| <= y nx' for every pair, in float64 with the DEVICE's y [Q] and nx' [N]: the project's own
    inequality, no tolerance.  -> (reason or None, the largest error / bound over the pairs with a finite bound)."""
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(dot_hat, np.float64) - chain_scaled)
        bound = np.asarray(y, np.float64)[:, None] * np.asarray(nx, np.float64)[None, :]
        fin = np.isfinite(bound) & (bound > 0)
        bad = ~(err <= bound) & ~np.isinf(bound) & ~np.isnan(chain_scaled)
        ratio = float((err[fin] / bound[fin]).max()) if fin.any() else 0.0
    if bad.any():
        q, r = np.argwhere(bad)[0]
        return f"{int(bad.sum())} pairs outside the bound, first (query {q}, row {r}): |{dot_hat[q, r]!r} - {chain_scaled[q, r]!r}| > {bound[q, r]!r}", ratio
    return None, ratio


def chain_scaled(chain, qref, rref):
    """chain(tw, x) 2^-(e+f) in float64 (powers of two: exact)."""
    return chain.astype(np.float64) * qref["s"].astype(np.float64)[:, None] * rref["scale"].astype(np.float64)[None, :]


# ------------------------------------------------------------------------------------------------------------------------- inputs
def store(x, fmt):
    """float64 / float32 rows -> the float32 values the bank of `fmt` holds."""
    x = np.asarray(x, dtype=np.float32)
    if fmt == "fp16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    return bfr.bf16(x) if fmt == "bf16" else x


@functools.lru_cache(maxsize=None)
def gaussian_case(fmt, Q, N, D, seed, subnormal_rows=0):
    """Gaussian rows of mixed scale and a weighted query set: (q, w, x as float32 values of the stored format)."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((Q, D), dtype=np.float32)
    decades = 1.3 if fmt == "fp16" else 3.0                       # fp16 rows stay clear of the format's ends
    x = rng.standard_normal((N, D)) * 10.0 ** rng.uniform(-decades, decades, size=(N, 1))
    for j in range(subnormal_rows):                               # rows of fp16 subnormals only, and one with a single subnormal
        r = 37 + 211 * j
        x[r] = rng.standard_normal(D) * (2.0 ** -17 if j % 2 == 0 else 1.0)
        if j % 2:
            x[r, j] = 2.0 ** -16
    w = (1.0 / (rng.random(D, dtype=np.float32) + 0.05) ** 2).astype(np.float32)
    w /= w.sum()
    return q, w, store(x, fmt)


@functools.lru_cache(maxsize=None)
def pair_case(fmt, lo, Q, N, D, seed, subnormal_rows=0):
    """gaussian_case with everything the per-pair checks need, computed once: the oracle's tw, qn, xn, both statements, the
    contract's denominators, the float64 scores and the half-widths (from the largest constants the statements allow)."""
    from oracle import similarity_oracle as so
    q, w, x = gaussian_case(fmt, Q, N, D, seed, subnormal_rows)
    tw, qn = so.prep_queries_np(q, w)
    xn = so.wnorms_np(x, w)
    qref = query_constants(tw, qn, fmt, D, eps_a_f32(fmt, D, lo))
    rref = row_constants(x, xn, fmt, D)
    den = den32(qn, xn)
    return dict(fmt=fmt, lo=lo, q=q, w=w, x=x, tw=tw, qn=qn, xn=xn, qref=qref, rref=rref, den=den, score=scores64(tw, x, qn, xn),
                hw=half_width(qref, rref, den), contract=so.cosine_scores_np(q, x, w))


def floor_of_first_rows(c, rows, k):
    """thr0 of the MODE 2 case: the oracle's k-th best score of each query over the first `rows` rows (fp32, the contract's)."""
    from oracle import similarity_oracle as so
    return np.ascontiguousarray(so.cosine_topk_np(c["q"], c["x"][:rows], k, c["w"])[0][:, k - 1])


def tau_window(c, seen, k):
    """Where a threshold published after the rows `seen` (a boolean mask) may lie: [kth - 2 hw_max - slack, kth] with kth the k-th
    best float64 score over them -- a lower bound of it (the proof needs that) and not a vacuous one (the k best rows are in the
    list, each with L >= score - 2 hw - slack)."""
    kth = kth_best(np.where(seen[None, :], c["score"], -INF), k)
    hw_max = np.where(seen[None, :] & np.isfinite(c["hw"]), c["hw"], 0.0).max(axis=1)
    return kth - 2 * hw_max - 2.0 ** -17 * (np.abs(kth) + hw_max), kth


def sandwich_window(c, tau_lo, tau_hi, allowed=None):
    """The sandwich when only a window of tau is known (the CPU file's view of a threshold the device will publish): must-be-in at
    the window's top, must-be-out at its bottom.  -> (must_in, must_out, don't-care share per query over the allowed rows)."""
    must_in, _ = sandwich(tau_hi, c["score"], c["hw"], c["contract"])
    _, must_out = sandwich(tau_lo, c["score"], c["hw"], c["contract"])
    ok = np.ones(c["score"].shape[1], dtype=bool) if allowed is None else allowed
    care = (~must_in & ~must_out)[:, ok]
    return must_in & ok, must_out & ok, care.mean(axis=1)


# The shapes of the GPU file (k = 5 throughout: cap = 4096, first = 8 tiles) and what the schedule makes of each -- pinned by the
# CPU file against `schedule`.
K = 5
SQ, SD = 300, 128                    # the sandwich cases: queries, features


def sandwich_seed(fmt):
    return {"fp32": 11, "fp16": 12, "bf16": 13}[fmt]


TAKE_ALL_N = {"fp32": 2048, "fp16": 2048 + 44, "bf16": 2048 + 44}
PHASES = {
    # (N, thr0, resident): launches
    (2048, False, False): [("mode0", 0, 8), ("select", 1), ("mode1", 8, 8), ("select", 1)],
    (2092, False, True): [("mode0", 0, 8), ("tail", 8), ("select", 1), ("mode1", 8, 8), ("select", 1)],
    (2048, True, False): [("mode2", 0, 8), ("select", 1)],
    (2048, True, True): [("mode2", 0, 8), ("select", 1)],
    (2304, False, False): [("mode0", 0, 8), ("select", 0), ("mode1", 8, 9), ("select", 1)],
    (2304, False, True): [("mode0", 0, 8), ("select", 0), ("mode1", 8, 9), ("select", 1)],
    (2560, False, False): [("mode0", 0, 8), ("select", 0), ("mode1", 8, 9), ("select", 0), ("mode2", 9, 10), ("select", 1)],
    (2560, False, True): [("mode0", 0, 8), ("select", 0), ("mode1", 8, 9), ("select", 0), ("mode2", 9, 10), ("select", 1)],
}
# under a selection of a resident bank of 2560 rows (10 tiles): one dead tile -> 9 live; two dead -> 8 live, the take-all is final
PHASES_SEL = {
    9: [("mode0", 0, 8), ("select", 0), ("mode1", 8, 9), ("select", 1)],
    8: [("mode0", 0, 8), ("select", 1), ("mode1", 8, 8), ("select", 1)],
}


def selection(N, dead_tiles, seed):
    """A random 50 % selection of N rows with whole tiles dead."""
    rng = np.random.default_rng(seed)
    flags = rng.random(N) < 0.5
    for t in dead_tiles:
        flags[t * BT:(t + 1) * BT] = False
    return flags


def kth_best(score, k):
    """k-th largest of each row of score [Q, n] (NaN as -inf)."""
    s = np.where(np.isnan(score), -INF, score)
    return -np.partition(-s, k - 1, axis=1)[:, k - 1]
