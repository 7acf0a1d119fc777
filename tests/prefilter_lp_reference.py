"""numpy restatement of stage 1 of the two-stage many-query search over a RESIDENT fp16 bank (csrc/topk_prefilter.hip, file
header): the weighted query is scaled by a power of two and rounded to fp16 (hi only, or hi + lo), the bank rows are the
stored fp16 values themselves, products are exact and summed in float64.  The matrix core may or may not flush fp16
subnormals of either operand to zero: both are modelled."""
import numpy as np

SUB = 2.0 ** -14                       # smallest normal fp16 magnitude


def scale_query(tw):
    """query16_kernel: tw (fp32 [D]) -> (q' fp32, qh fp16, ql fp16, 2^-f): the largest |q'| lies in [2^13, 2^14)."""
    tw = np.asarray(tw, dtype=np.float32)
    mx = float(np.abs(tw).max())
    e = 0
    if 0.0 < mx < np.inf:
        e = int(np.frexp(mx)[1]) - 14
    e = max(e, -126)
    s = np.float32(2.0 ** -e)
    qp = (tw * s).astype(np.float32)                 # a power of two: exact
    qh = qp.astype(np.float16)
    ql = (qp - qh.astype(np.float32)).astype(np.float16)
    return qp, qh, ql, float(s)


def flushed(h):
    """fp16 subnormals -> 0 (what a flushing matrix core multiplies)."""
    h = np.array(h, dtype=np.float16, copy=True)
    h[np.abs(h.astype(np.float64)) < SUB] = 0
    return h


def count_subnormals(x16):
    """nsub per row: elements with 0 < |x| < 2^-14."""
    a = np.abs(np.asarray(x16, dtype=np.float16).astype(np.float64))
    return ((a > 0) & (a < SUB)).sum(axis=-1)


def stage1_dots(qh, ql, x16, lo, flush_q, flush_x):
    """dot^ [N] of one query against the rows x16 [N, D]: sum_d (qh_d [+ ql_d]) * x_d, exact products, float64 sum."""
    x = (flushed(x16) if flush_x else np.asarray(x16, dtype=np.float16)).astype(np.float64)
    a = (flushed(qh) if flush_q else qh).astype(np.float64)
    if lo:
        a = a + (flushed(ql) if flush_q else ql).astype(np.float64)
    return x @ a


def fma_chain(tw, x32):
    """The contract's chain acc = fmaf(tw[d], x[d], acc) over d = 0 .. D-1, for every row of x32 [N, D] (fp32).  Every step is
    computed in float64 (the product of two fp32 numbers is exact there) and rounded to fp32: within 2^-53 relative of the
    single rounding of fmaf, which is all a test of an error BOUND needs."""
    tw = np.asarray(tw, dtype=np.float32).astype(np.float64)
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    acc = np.zeros(x.shape[0], dtype=np.float32)
    for d in range(x.shape[1]):
        acc = (tw[d] * x[:, d] + acc.astype(np.float64)).astype(np.float32)
    return acc
