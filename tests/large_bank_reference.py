"""A reference for bank searches that scales to banks the CPU oracles cannot score whole (millions of rows x many queries).
Used by tests/test_large_bank_gpu.py; proved on small banks, without a GPU, by tests/test_large_bank_reference_cpu.py.

A row's (an image's) score depends on that row (image) only, so two things are enough:

  slices            score outputs are compared with the existing oracles on chosen row / image ranges copied to the host
                    (``slices`` picks them: both ends, a window around every line, a strided sample);

  screen + oracle   for top-k lists (``screen_topk``):
                    (a) every item's score in fp64 by plain chunked torch on whatever device holds the bank (``cosine_fp64``,
                        ``distance_fp64``, ``combine_fp64``) -- code that has no part in the kernels under test;
                    (b) per query, the items whose fp64 score is within MARGIN of the k-th best fp64 score survive, and so does
                        every planted item;
                    (c) the exact oracle runs on the survivors on the host; the survivors are kept in ascending global order,
                        so the oracle's tie rule (lower index first) is the global one and local indices map straight back.
                    The result is the expected list bit for bit.

MARGIN = 1e-5.  The oracle's score is within 5e-7 of the plain formula (tests/test_oracle_golden.py), so an item the exact search
ranks among the k best has an fp64 score no lower than the k-th best fp64 score minus 2 x 5e-7; 1e-5 is twenty times the
oracle's bound.  It is a condition from the project's contract, not a measurement.  For a distance (smaller is better) the k
smallest are kept and the margin is relative to the k-th distance.  NaN scores rank as -inf (a NaN distance as +inf), as in
the oracles.  The screen asserts that the survivors number at least k (where that many finite scores exist) and at most
2 k + the planted items: a reference that let half the bank through would prove nothing about its own screen.
"""
import numpy as np
import torch

MARGIN = 1e-5
COMBINES = ("min", "mean", "max")


def slices(n, lines=(), width=2048, sample=4096):
    """Ascending unique indices (int64 numpy) into n items: the first and the last ``width``, ``width`` around every line
    (the item that holds the line included) and a strided sample of ``sample``."""
    parts = [np.arange(0, min(width, n)), np.arange(max(0, n - width), n)]
    for line in lines:
        parts.append(np.arange(max(0, line - width // 2), min(n, line + width // 2)))
    parts.append(np.arange(min(sample, n)) * max(1, n // max(1, min(sample, n))))
    return np.unique(np.concatenate(parts)).astype(np.int64)


def rows_of_images(images, P):
    """Image indices -> the indices of their P rows each, image by image."""
    return (np.asarray(images, np.int64)[:, None] * P + np.arange(P)[None, :]).reshape(-1)


def gather_host(bank, idx):
    """bank[idx] as contiguous fp32 numpy (a 16-bit bank widened exactly)."""
    sel = bank.index_select(0, torch.as_tensor(np.asarray(idx, np.int64), device=bank.device))
    return np.ascontiguousarray(sel.float().cpu().numpy())


def cosine_fp64(queries, rows, weights=None, eps=1e-6, chunk=50000):
    """[Q, R] fp64 weighted-cosine scores of rows [R, D] (any float dtype, any device), the plain formula
    sum(w t x) / (sqrt(sum w t^2) sqrt(sum w x^2) + eps); NaN -> -inf.  ``weights``: None, [D], or [Q, D] (one row per query)."""
    dev = rows.device
    q = queries.to(dev, torch.float64)
    Q, D = q.shape
    w = torch.ones(D, dtype=torch.float64, device=dev) if weights is None else weights.to(dev, torch.float64)
    wq = w.expand(Q, D)
    tw = wq * q
    qn = (tw * q).sum(1).sqrt()
    out = torch.empty(Q, rows.shape[0], dtype=torch.float64, device=dev)
    for lo in range(0, rows.shape[0], chunk):
        x = rows[lo:lo + chunk].double()
        dot = tw @ x.T
        xn = ((x * x) @ wq.T).T.sqrt()                             # [Q, c]: the row norm under every query's weights
        out[:, lo:lo + chunk] = dot / (qn[:, None] * xn + eps)
    return torch.where(torch.isnan(out), torch.full_like(out, -np.inf), out)


def distance_fp64(c, queries, rows, metric, chunk=16384):
    """[Q, R] fp64 weighted MSE / MAE: mean over d of c[d] * v[d] (c [D], or [Q, D]); NaN stays NaN (the combine ranks it)."""
    dev = rows.device
    q = queries.to(dev, torch.float64)
    c = c.to(dev, torch.float64).expand(q.shape)
    out = torch.empty(q.shape[0], rows.shape[0], dtype=torch.float64, device=dev)
    for lo in range(0, rows.shape[0], chunk):
        x = rows[lo:lo + chunk].double()
        for qi in range(q.shape[0]):
            d = x - q[qi]
            v = d.abs() if metric == "MAE" else d * d
            out[qi, lo:lo + chunk] = (v * c[qi]).mean(1)
    return out


def combine_fp64(tok, P, combine, top_t=None, distance=False):
    """[Q, N * P] fp64 token scores (distances) -> [Q, N] combined, by the documented rules: a -inf score (+inf distance; NaN
    counts as that) makes min and mean -inf (max and mean +inf); top_t: only the top_t best tokens count."""
    Q = tok.shape[0]
    bad = np.inf if distance else -np.inf
    s = torch.where(torch.isnan(tok), torch.full_like(tok, bad), tok).view(Q, -1, P)
    if top_t is not None:
        s = s.sort(dim=2, descending=not distance).values[:, :, :top_t]
        if combine == ("max" if not distance else "min"):
            return s[:, :, 0].contiguous()
        if combine == ("min" if not distance else "max"):
            return s[:, :, top_t - 1].contiguous()
    elif combine != "mean":
        return s.min(dim=2).values if combine == "min" else s.max(dim=2).values
    out = s.sum(dim=2) / s.shape[2]
    return torch.where(torch.isnan(out), torch.full_like(out, bad), out)


def screen_topk(score64, k, planted, oracle, smallest=False, idx_offset=0):
    """score64 [Q, M] fp64 (torch, any device); planted: indices always kept; oracle(qi, idx) -> (s [k] f32, i [k] i64 local to
    the ascending int64 numpy array ``idx``, -1 for a missing entry) is the exact search of query qi over the items ``idx``.
    -> (scores [Q, k] f32, indices [Q, k] i64 global + idx_offset, the largest survivor count)."""
    Q, M = score64.shape
    assert k <= M
    key = -score64 if smallest else score64
    key = torch.where(torch.isnan(key), torch.full_like(key, -np.inf), key)
    kth = key.topk(k, dim=1).values[:, k - 1]
    cut = kth - MARGIN * (kth.abs() if smallest else 1.0)
    planted = np.unique(np.asarray(planted, np.int64))
    out_s, out_i, most = [], [], 0
    for qi in range(Q):
        ranked = key[qi] > -np.inf                                   # what ranks as -inf is never returned by any search
        keep = torch.nonzero((key[qi] >= cut[qi]) & ranked).squeeze(1).cpu().numpy()
        assert len(keep) >= min(k, int(ranked.sum())), (qi, len(keep), k)
        idx = np.union1d(keep, planted).astype(np.int64)
        assert len(idx) <= 2 * k + len(planted), f"query {qi}: {len(idx)} survivors of the screen for k = {k}, {len(planted)} planted"
        most = max(most, len(idx))
        s, i = oracle(qi, idx)
        s, i = np.asarray(s, np.float32).reshape(k), np.asarray(i, np.int64).reshape(k)
        out_s.append(s)
        out_i.append(np.where(i >= 0, idx[np.clip(i, 0, len(idx) - 1)] + idx_offset, -1))
    return np.stack(out_s), np.stack(out_i), most
