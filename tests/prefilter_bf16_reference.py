"""numpy restatement of stage 1 of the two-stage many-query search over a RESIDENT bf16 bank (csrc/topk_prefilter.hip, file
header, "Resident bf16 bank"): the weighted query is scaled by a power of two so that its largest component lies in
[2^-21, 2^-20) and split into bf16 hi (+ lo), the bank rows are the stored bf16 values themselves, products are exact and
summed in float64.  What the matrix core does with tiny numbers is not known, so the worst is modelled too: bf16-subnormal
operands (|v| < 2^-126) flushed to zero, on either side, and every product below 2^-126 flushed to zero.

bf16 comes from torch on the CPU (``tensor.to(torch.bfloat16)``: round to nearest even, overflow to inf, subnormals kept); a bf16
value is carried here as the float32 it widens to."""
import numpy as np
import torch

TINY = 2.0 ** -126                     # smallest normal magnitude of bf16 and of fp32
QMAX_EXP = -20                         # the largest |q'| of a scaled query lies in [2^(QMAX_EXP - 1), 2^QMAX_EXP)
ROW_LO, ROW_HI = 2.0 ** -60, 2.0 ** 120   # a row is boundable iff its nonzero elements lie in [ROW_LO, ROW_HI) (and xn is finite)
SCALE_LO, SCALE_HI = 2.0 ** -100, 2.0 ** 30   # a query is inside the bound iff SCALE_LO < 2^-f < SCALE_HI


def bf16(x):
    """fp32 array -> the nearest bf16 values (ties to even), as fp32."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    return t.to(torch.bfloat16).to(torch.float32).numpy()


def scale_query(tw):
    """query16_kernel<BF>: tw (fp32 [D]) -> (q' fp32, qh, ql (bf16 as fp32), 2^-f)."""
    tw = np.asarray(tw, dtype=np.float32)
    mx = float(np.abs(tw).max())
    e = 0
    if 0.0 < mx < np.inf:
        e = int(np.frexp(mx)[1]) - QMAX_EXP
    e = min(max(e, -126), 100)
    s = np.float32(2.0 ** -e)
    qp = (tw * s).astype(np.float32)                 # a power of two: exact unless the result is an fp32 subnormal
    qh = bf16(qp)
    ql = bf16((qp - qh).astype(np.float32))          # the difference is exact in fp32
    return qp, qh, ql, float(s)


def query_in_window(s):
    return SCALE_LO < s < SCALE_HI


def flushed(v):
    """bf16 subnormals -> 0 (what a flushing matrix core multiplies)."""
    v = np.array(v, dtype=np.float32, copy=True)
    v[np.abs(v.astype(np.float64)) < TINY] = 0
    return v


def unboundable(x):
    """bankbf16_rowp_kernel's rule for the rows of x [N, D] (bf16 as fp32), without the weighted norm's part of it: True where a
    row has an inf / NaN element or a nonzero element outside [ROW_LO, ROW_HI)."""
    a = np.abs(np.asarray(x, dtype=np.float32).astype(np.float64))
    with np.errstate(invalid="ignore"):
        return (~(a < ROW_HI) | ((a > 0) & (a < ROW_LO))).any(axis=-1)


def stage1_dots(qh, ql, x, lo, flush_q, flush_x, flush_products):
    """dot^ [N] of one query against the rows x [N, D]: sum_d (qh_d [+ ql_d]) * x_d, exact products, float64 sum."""
    x = (flushed(x) if flush_x else np.asarray(x, dtype=np.float32)).astype(np.float64)
    total = np.zeros(x.shape[0])
    for part in ((qh, ql) if lo else (qh,)):
        a = (flushed(part) if flush_q else part).astype(np.float64)
        p = x * a                                    # 8-bit x 8-bit significands: exact in float64
        if flush_products:
            p = np.where(np.abs(p) < TINY, 0.0, p)
        total += p.sum(axis=1)
    return total
