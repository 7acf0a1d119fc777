"""Plain statements (numpy, float64 and integers) of what STAGE 2 of the two-stage many-query search must do with the candidate
lists stage 1 left: the final select_kernel's choice (needed path, quota path, `bound`), the re-score (scores, order, index offset,
tails) and the certificate (`redo`), candidate by candidate, for tests/test_prefilter_stage2_{cpu,gpu}.py.  The file under test is
csrc/topk_prefilter.hip.  tests/prefilter_stage1_reference.py covers everything up to the last append and is reused, not copied.

All checkers work on ONE query (the GPU file loops over all of them) and on the arrays the call left in the caller's workspace:
there is no model of dot^ here, the device's own cand_d is the input.  They return None or a reason string (check_final_select:
also the number of memberships BAND leaves undecided)."""
import functools

import numpy as np

from tests import prefilter_stage1_reference as sr
from tests.prefilter_stage1_reference import EPS, FMTS, INF, RESCORE_MAX, chain_all    # noqa: F401  (FMTS: re-exported)

# BAND: the relative slack inside which the side of a candidate's U (or L) against a threshold is a don't-care.  select_kernel's
#     err = qb.y * rp.y;  hi = (cd + err) * sc;  U = hi / den;  U *= 1 +- 2^-21
# holds these fp32 roundings: the product err (1, relative to err), the sum (1), the product with sc = 2^(e+f) (a power of two:
# none), the division (the compiler's: correctly rounded or within 2.5 ulp -- 3) and the widening product (1): 6 roundings of
# 2^-24 each.  Contraction (the file is built with it on) can only fuse the first product into the sum, which removes one.  den
# is an explicit fmaf and 1 + 2^-21 a constant: the same bits here and there.  `intervals` rounds to fp32 after every operation,
# so it differs from the device by at most those 6 roundings: BAND = 8 * 2^-24 = 2^-21, applied to |value| + the candidate's
# half-width (the first two roundings are relative to err and to |cd| + err, which exceed |hi| when cd and err cancel).
BAND = 2.0 ** -21
Q, D, K = 40, 128, 5                                   # the GPU file's shapes: one query tile, above the Q >= 17 floor
N_OF = {"fp32": 2560, "fp16": 2560 + 37, "bf16": 2560 + 37}
N_K192 = {"fp32": 4608, "fp16": 4608 + 37, "bf16": 4608 + 37}
OFFSET = 2 ** 33 + 7


def r32(a):
    """Round float64 values to fp32 (one rounding), back as float64."""
    with np.errstate(all="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def counting(rows, rowp, sel):
    """Which candidates of a list count: under a selection all but those whose row holds the sentinel (rowp[., 2] == 0)."""
    rows = np.asarray(rows, dtype=np.int64)
    return np.asarray(rowp, np.float32)[rows, 2] != 0 if sel else np.ones(len(rows), dtype=bool)


def intervals(cand_d, rows, qbase_q, rowp, xn, eps=EPS, sel=False):
    """float64 (U, L) of one query's candidates as select_kernel defines them: ((dot^ +- y nx') 2^(e+f)) / fmaf(qn, xn, eps), widened
    by 2^-21 away from the score, NaN -> +inf / -inf, every operation rounded to fp32 (see BAND for what that leaves open).  sel:
    a candidate whose row holds the sentinel does not count: U = L = -inf (a row that counts never has U = -inf), xn not read."""
    rows = np.asarray(rows, dtype=np.int64)
    cd = np.asarray(cand_d, dtype=np.float32).astype(np.float64)
    rp = np.asarray(rowp, dtype=np.float32)[rows].astype(np.float64)
    qb = np.asarray(qbase_q, dtype=np.float32).astype(np.float64)
    xn = np.asarray(xn, dtype=np.float32)
    dead = ~counting(rows, rowp, sel)
    xr = xn[np.minimum(rows, len(xn) - 1)].astype(np.float64)
    w = 2.0 ** -21
    with np.errstate(all="ignore"):
        den = r32(qb[3] * xr + float(np.float32(eps)))
        sc = r32(r32(1.0 / qb[2]) * r32(1.0 / rp[:, 2]))
        err = r32(qb[1] * rp[:, 1])
        U = r32(r32(r32(cd + err) * sc) / den)
        L = r32(r32(r32(cd - err) * sc) / den)
        U = r32(np.where(U >= 0, U * (1 + w), U * (1 - w)))
        L = r32(np.where(L >= 0, L * (1 - w), L * (1 + w)))
    U = np.where(np.isnan(U), INF, U)
    L = np.where(np.isnan(L), -INF, L)
    U[dead], L[dead] = -INF, -INF
    return U, L


def tie_classes(cand_d, rows, rowp, xn):
    """Class number per candidate: equal (cand_d bits, rowp row bits, xn bits) -> equal device U."""
    rows = np.asarray(rows, dtype=np.int64)
    xn = np.asarray(xn, dtype=np.float32)
    key = np.concatenate([sr.f32bits(cand_d)[:, None], sr.f32bits(np.asarray(rowp, np.float32)[rows]),
                          sr.f32bits(xn[np.minimum(rows, len(xn) - 1)])[:, None]], axis=1)
    if len(rows) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.unique(key, axis=0, return_inverse=True)[1].reshape(-1)


def sides(U, L, thr, band, mult=1):
    """(above, below) of each candidate's U against thr, decided only outside band * mult * (max(|U|, |thr|) + half-width)."""
    with np.errstate(all="ignore"):
        s = band * mult * (np.maximum(np.abs(U), abs(thr)) + (U - L) / 2)
        s = np.where(np.isfinite(s), s, 0.0)
        return U > thr + s, U < thr - s


def kth_largest(v, k):
    return -INF if len(v) < k else float(-np.partition(-np.asarray(v, np.float64), k - 1)[k - 1])


def check_final_select(rows, U, L, k, nsel, sel_i, bound, live, ties=None, band=BAND):
    """One query's final selection against its list.  rows: the listed rows; U, L: `intervals` of them; live: which of them count
    (`counting`); ties: `tie_classes` (None: none); band = 0: U and L are the device's own to the bit (synthetic arrays).
    -> (reason or None, memberships left undecided by the band).

      * no row twice in sel_i[:nsel], every selected row a listed one that counts, nsel <= 256;
      * bound == -inf: every live candidate selected (live <= 256), or the needed path: a k-th largest L exists, selected <=> U >= L_k;
      * bound > -inf: nsel == 256 < live, every selected U >= bound, every unselected U <= bound, and the candidates with U >= L_k
        do not fit 256 (or no k-th largest finite L exists): the quota path is taken only then.
    L_k is the k-th largest of the reference's own L, itself within the band of the device's, so U against L_k is decided outside
    twice the band.  A tie class is one value: it counts once among the undecided, and not at all when the selection splits it
    (its U is then the bound itself)."""
    rows = np.asarray(rows, dtype=np.int64)
    n = len(rows)
    live = np.asarray(live, dtype=bool)
    nlive = int(live.sum())
    bound = float(bound)
    if not 0 <= nsel <= RESCORE_MAX:
        return f"nsel = {nsel} outside 0 .. {RESCORE_MAX}", 0
    sel = np.asarray(sel_i, dtype=np.int64)[:nsel]
    if len(np.unique(sel)) != nsel:
        return "a row is selected twice", 0
    if len(np.unique(rows)) != n:
        return "a row is listed twice", 0
    order = np.argsort(rows)
    at = np.minimum(np.searchsorted(rows[order], sel), max(n - 1, 0))
    if nsel and (n == 0 or not (rows[order][at] == sel).all()):
        return "a selected row is not in the list", 0
    chosen = np.zeros(n, dtype=bool)
    chosen[order[at]] = nsel > 0
    if (chosen & ~live).any():
        return f"row {int(rows[np.argmax(chosen & ~live)])} does not count (sentinel) and is selected", 0
    ties = np.arange(n) if ties is None else np.asarray(ties)
    Lk = kth_largest(L[live], k)
    above_k, below_k = sides(U, L, Lk, band, 2)
    need_k = ~below_k if band else U >= Lk                       # could be needed / is needed (exact mode)

    def undecided(mask):
        """Distinct tie classes among the undecided candidates, less those the selection splits."""
        cls = set(ties[mask & live].tolist())
        split = set(ties[chosen & live].tolist()) & set(ties[~chosen & live].tolist())
        return len(cls - split)

    if bound == -INF:
        if nsel == nlive:
            return (None, 0) if nlive <= RESCORE_MAX else ("more than 256 selected", 0)
        if Lk == -INF:
            return "bound = -inf with candidates left out and no k-th largest finite lower bound", 0
        out = live & ~chosen & (above_k if band else U >= Lk)
        if out.any():
            return f"row {int(rows[np.argmax(out)])} has U >= L_k, is left out, and bound = -inf", 0
        extra = chosen & below_k
        if extra.any():
            return f"row {int(rows[np.argmax(extra)])} has U < L_k and is selected on the needed path", 0
        return None, undecided(~above_k & ~below_k) if band else 0
    if nsel != RESCORE_MAX or nlive <= RESCORE_MAX:
        return f"bound = {bound!r} is finite with nsel = {nsel}, live = {nlive}: the quota path needs nsel = 256 < live", 0
    above, below = sides(U, L, bound, band)
    if (chosen & below).any():
        return f"selected row {int(rows[np.argmax(chosen & below)])} has U < bound = {bound!r}", 0
    if (live & ~chosen & above).any():
        i = int(np.argmax(live & ~chosen & above))
        return f"row {int(rows[i])} has U = {U[i]!r} > bound = {bound!r} and is left out", 0
    care = undecided(~above & ~below) if band else 0
    if Lk > -INF:
        could = int((live & need_k).sum())
        if could <= RESCORE_MAX:
            return f"quota path taken although only {could} candidates have U >= L_k: the needed path fits", 0
        sure = int((live & (above_k if band else need_k)).sum())
        if sure <= RESCORE_MAX:
            care += undecided(~above_k & ~below_k)
    return None, care


# ------------------------------------------------------------------------------------------------------------------- exact scores
def exact_scores(tw, qn, x, xn, eps=EPS):
    """The contract's score of every pair, fp32 [Q, N]: finish_score of the oracle chain -- fp32(chain / fmaf(qn, xn, eps)), NaN ->
    -inf."""
    with np.errstate(all="ignore"):
        s = (chain_all(tw, x).astype(np.float64) / sr.den32(qn, xn, eps).astype(np.float64)).astype(np.float32)
    return np.where(np.isnan(s), np.float32(-INF), s).astype(np.float32)


def topk_of(score_q, k, allowed=None, few=False, idx_offset=0):
    """The oracle's answer for one query from its scores [N] (fp32): (score desc, row asc) over the allowed rows, the first k;
    few: rows scoring -inf are not returned.  Missing entries are (-inf, -1)."""
    rows = np.arange(len(score_q)) if allowed is None else np.flatnonzero(allowed)
    s = np.asarray(score_q, dtype=np.float32)[rows]
    if few:
        rows, s = rows[s > -INF], s[s > -INF]
    order = np.lexsort((rows, -s.astype(np.float64)))[:k]
    out_s = np.full(k, -INF, dtype=np.float32)
    out_i = np.full(k, -1, dtype=np.int64)
    out_s[:len(order)] = s[order]
    out_i[:len(order)] = rows[order] + idx_offset
    return out_s, out_i


def same_answer(out_s, out_i, want_s, want_i):
    return np.array_equal(sr.f32bits(out_s), sr.f32bits(want_s)) and np.array_equal(np.asarray(out_i, np.int64), np.asarray(want_i, np.int64))


def check_rescore(sel_rows, tw_q, qn_q, x, xn, k, idx_offset, out_s, out_i, few, eps=EPS, scores=None):
    """One query's output against the exact scores of EXACTLY its selected rows: bit for bit the oracle chain's (scores: that
    query's row of `exact_scores`, else computed here), ordered (score desc, row asc), the first k, out_i = idx_offset + row; with
    fewer than k rows the (-inf, -1) tail -- from n, or under `few` from the number of rows that score above -inf, which alone
    are returned.  (`few` changes nothing when n >= k: the kernel's rule.)"""
    sel_rows = np.asarray(sel_rows, dtype=np.int64)
    if scores is None:
        xs = np.asarray(x, np.float32)[sel_rows]
        s = exact_scores(np.asarray(tw_q, np.float32)[None, :], np.asarray([qn_q], np.float32), xs, np.asarray(xn, np.float32)[sel_rows], eps)[0]
    else:
        s = np.asarray(scores, dtype=np.float32)[sel_rows]
    full = np.full(int(sel_rows.max()) + 1 if len(sel_rows) else 1, -INF, dtype=np.float32)
    allowed = np.zeros(len(full), dtype=bool)
    full[sel_rows], allowed[sel_rows] = s, True
    want_s, want_i = topk_of(full, k, allowed, few and len(sel_rows) < k, idx_offset)
    out_s, out_i = np.asarray(out_s, np.float32), np.asarray(out_i, np.int64)
    bad = (sr.f32bits(out_s) != sr.f32bits(want_s)) | (out_i != want_i)
    if bad.any():
        j = int(np.argmax(bad))
        return f"rank {j}: ({out_s[j]!r}, {int(out_i[j])}) != ({want_s[j]!r}, {int(want_i[j])}) from the {len(sel_rows)} selected rows"
    return None


def check_certificate(out_s, bound, overflow, nsel, k, few, redo):
    """redo against the statement, from the read-back bound and out_s themselves (fp32 compared as fp32: exact)."""
    b = np.float32(bound)
    if nsel >= k:
        want = int(bool(overflow) or not (np.float32(out_s[k - 1]) > b))
        why = f"overflow = {int(overflow)}, out_s[k-1] = {out_s[k - 1]!r}, bound = {b!r}"
    elif not few:
        want, why = 1, f"only {nsel} candidates for k = {k}"
    else:
        want = int(bool(overflow) or bool(b > np.float32(-INF)))
        why = f"few: overflow = {int(overflow)}, bound = {b!r}"
    return None if int(redo) == want else f"redo = {int(redo)}, expected {want} ({why})"


def check_soundness(rows, live, sel_rows, score_q, k, nsel, bound, redo, out_s, out_i, want_s, want_i):
    """One query: with redo == 0 the answer IS the oracle's (want_s, want_i: `topk_of` over the whole bank or the selection), bit
    for bit; and whatever redo says, every listed candidate that counts and was not selected scores (exactly) <= bound when the
    bound is finite, and < out_s[k-1] when bound == -inf and k rows were re-scored."""
    if int(redo) == 0 and not same_answer(out_s, out_i, want_s, want_i):
        return "redo = 0 and the answer is not the oracle's"
    rows = np.asarray(rows, dtype=np.int64)
    left = rows[np.asarray(live, bool) & ~np.isin(rows, np.asarray(sel_rows, np.int64))]
    s = np.asarray(score_q, np.float32)[left]
    if bound > -INF:
        bad = ~(s <= np.float32(bound))
        what = f"bound = {bound!r}"
    elif nsel >= k:
        bad = ~(s < np.float32(out_s[k - 1]))
        what = f"the k-th returned score {out_s[k - 1]!r}"
    else:
        return None
    return f"row {int(left[np.argmax(bad)])} was left out and scores {s[np.argmax(bad)]!r}, not below {what}" if bad.any() else None


# ------------------------------------------------------------------------------------------------------------------ case builders
def hw_of(tw, x, den, eps_a):
    """The half-width of every pair in score units, float64 [Q, N]: eps_a ||q'|| ||x'|| 2^(e+f) / den = eps_a ||tw|| ||x|| / den (the
    powers of two cancel); inf / NaN where a row's norm is."""
    with np.errstate(all="ignore"):
        nq = np.sqrt((np.asarray(tw, np.float64) ** 2).sum(axis=1))
        nx = np.sqrt((np.asarray(x, np.float64) ** 2).sum(axis=1))
        return eps_a * nq[:, None] * nx[None, :] / np.asarray(den, np.float64)


def background(fmt, N, seed, n_q=Q, d=D):
    """Gaussian queries and rows of unit norm times a scale in [0.5, 4): (q float32 [Q, D], x float32 values of the stored format)."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n_q, d), dtype=np.float32)
    g = rng.standard_normal((N, d))
    x = g / np.linalg.norm(g, axis=1, keepdims=True) * rng.uniform(0.5, 4.0, size=(N, 1))
    return rng, q, sr.store(x, fmt)


def score_rows(t, qn_q, x):
    """(float64 exact scores of query t against stored rows x, their fp32 denominators)."""
    from oracle import similarity_oracle as so
    den = sr.den32(np.asarray([qn_q], np.float32), so.wnorms_np(x))[0].astype(np.float64)
    return (x.astype(np.float64) @ t.astype(np.float64)) / den, den


def plant(rng, t, qn_q, fmt, count, s_lo, s_hi):
    """`count` stored rows of `fmt` whose exact float64 score for query t lies in [s_lo, s_hi]: x = c u + sqrt(1 - c^2) v, u = t /
    ||t||, v a random unit vector orthogonal to u, c drawn from the window; storing moves the score, so rows are drawn until
    enough land inside."""
    d = len(t)
    u = t.astype(np.float64) / np.linalg.norm(t.astype(np.float64))
    got = []
    for _ in range(200):
        m = max(8 * count, 4096)
        c = rng.uniform(s_lo, s_hi, size=m)
        g = rng.standard_normal((m, d))
        g -= (g @ u)[:, None] * u[None, :]
        v = g / np.linalg.norm(g, axis=1, keepdims=True)
        x = sr.store(c[:, None] * u[None, :] + np.sqrt(1 - c * c)[:, None] * v, fmt)
        s, _ = score_rows(t, qn_q, x)
        ok = (s >= s_lo) & (s <= s_hi)
        if fmt == "fp16":                       # an fp16-subnormal element adds its own term to the row's nx': another half-width
            ok &= sr.lpr.count_subnormals(x.astype(np.float16)) == 0
        got.extend(x[ok][:count - len(got)])
        if len(got) == count:
            return np.array(got, dtype=np.float32)
    raise AssertionError(f"could not plant {count} rows in [{s_lo}, {s_hi}]")


# windows of the planted rows below the k-th planted score s_k, in half-widths hw (of the planted query at unit rows): (count, from, to).
# The certified window of the issue is [-1.8, -1.2], the refused one [-0.6, -0.2]; inside them the rows stand so that the candidate
# whose U becomes the bound (rank 256 by U: k + 250 above it) stands alone, BAND away from its neighbours under any format.
WINDOWS = {
    "needed": [],
    "quota-certified": [(250, -1.5, -1.2), (1, -1.63, -1.61), (49, -1.8, -1.7)],
    "quota-refused": [(250, -0.4, -0.2), (1, -0.51, -0.49), (49, -0.6, -0.55)],
    "ties": [(100, -1.35, -1.2), (-400, -1.69, -1.67)],                         # negative count: that many copies of ONE row
}
PATH = {"needed": "needed", "quota-certified": "quota-certified", "quota-refused": "quota-refused", "ties": "quota-certified"}
PLANTED_Q = 3                                            # the planted query (any but the first: nothing special about it)


@functools.lru_cache(maxsize=None)
def planted_case(name, fmt, lo, k=K):
    """The needed / quota / ties cases of the issue's table: a background bank, and for query PLANTED_Q k rows at c = 0.8 + j 1e-4
    and the rows of WINDOWS[name] under the least of them, s_k, at random positions (every tile, the tail tile included).
    -> dict(q, tw, qn, x, xn, planted={query: path}, top (rows of the k), groups ([(rows, from, to)] in hw), s_k, hw)."""
    from oracle import similarity_oracle as so
    N = N_OF[fmt]
    rng, q, x = background(fmt, N, 100 + 7 * FMTS.index(fmt) + lo + 31 * sorted(WINDOWS).index(name))
    tw, qn = so.prep_queries_np(q, None)
    t, pq = tw[PLANTED_Q], PLANTED_Q
    eps_a = sr.eps_a(fmt, D, lo)
    total = k + sum(abs(c) for c, _, _ in WINDOWS[name])
    where = np.concatenate([[N - 1, 3], 4 + rng.permutation(N - 5)[:total - 2]])   # one in the last (tail) tile, one in the first
    top = np.concatenate([plant(rng, t, qn[pq], fmt, 1, 0.8 + j * 1e-4 - 2e-5, 0.8 + j * 1e-4 + 2e-5) for j in range(k)])
    s_top, den_top = score_rows(t, qn[pq], top)
    s_k = float(s_top.min())
    hw = float(hw_of(t[None, :], top, den_top[None, :], eps_a)[0].max())    # unit rows: the same for all planted rows to 2^-10
    x[where[:k]] = top
    groups, at = [], k
    for count, a, b in WINDOWS[name]:
        rows = plant(rng, t, qn[pq], fmt, 1 if count < 0 else count, s_k + a * hw, s_k + b * hw)
        x[where[at:at + abs(count)]] = rows                               # (one row broadcast: the copies)
        groups.append((where[at:at + abs(count)].copy(), a, b))
        at += abs(count)
    xn = so.wnorms_np(x)
    return dict(name=name, fmt=fmt, lo=lo, k=k, q=q, tw=tw, qn=qn, x=x, xn=xn, planted={pq: PATH[name]}, top=where[:k].copy(), groups=groups,
                s_k=s_k, hw=hw)


@functools.lru_cache(maxsize=None)
def score_tie_case(fmt, k=K):
    """2k bit-identical copies of the planted query's best row, one in each of 2k different tiles, the last (tail) tile included."""
    from oracle import similarity_oracle as so
    N = N_OF[fmt]
    rng, q, x = background(fmt, N, 300 + FMTS.index(fmt))
    tw, qn = so.prep_queries_np(q, None)
    best = plant(rng, tw[PLANTED_Q], qn[PLANTED_Q], fmt, 1, 0.8, 0.81)[0]
    tiles = np.arange(-(-N // 256))[::-1][:2 * k]                        # 2k tiles from the last one down (10 or 11 tiles in all)
    rows = np.minimum(tiles * 256 + rng.integers(0, 256, size=2 * k), N - 1)
    x[rows] = best
    return dict(q=q, tw=tw, qn=qn, x=x, xn=so.wnorms_np(x), planted={PLANTED_Q: "needed"}, copies=np.sort(rows))


@functools.lru_cache(maxsize=None)
def unboundable_case(fmt):
    """Rows with a NaN, an inf, all zeros and (bf16) an element below 2^-60; and for query PLANTED_Q a bank whose every row points
    away from it, so that its k-th best score is negative (the all-zero rows score 0).  The NaN and inf rows that must be selected
    stand in the take-all slice (rows < 2048), where every pair is stored.  Behind it stage 1 tests dot^ itself, and a resident
    bank's NaN or inf element makes that NaN or -inf for some queries: such a row (exact score -inf whatever the query) may be
    listed or not, so the `late` rows only have to be selected WHEN listed (check_final_select: U = +inf) and never returned."""
    from oracle import similarity_oracle as so
    N = N_OF[fmt]
    rng, q, x = background(fmt, N, 400 + FMTS.index(fmt))
    tw, qn = so.prep_queries_np(q, None)
    u = tw[PLANTED_Q].astype(np.float64) / np.linalg.norm(tw[PLANTED_Q].astype(np.float64))
    c = x.astype(np.float64) @ u
    x = sr.store(x - ((c + np.abs(c) + 0.05 * np.linalg.norm(x, axis=1)) [:, None]) * u[None, :], fmt)
    rows = dict(nan=[5, 1500], inf=[300, 1900], zero=[7, 1000], late=[N - 3, N - 2])
    x[rows["nan"] + rows["late"][:1], 9] = np.nan
    x[rows["inf"][0], 2], x[rows["inf"][1], 3], x[rows["late"][1], 3] = np.inf, -np.inf, np.inf
    x[rows["zero"]] = 0
    if fmt == "bf16":
        rows["tiny"] = [11, N - 5]
        x[rows["tiny"], 4] = 2.0 ** -70
    with np.errstate(all="ignore"):
        xn = so.wnorms_np(x)
    return dict(q=q, tw=tw, qn=qn, x=x, xn=xn, planted={PLANTED_Q: "needed"}, rows=rows,
                unb=sorted(rows["nan"] + rows["inf"] + rows.get("tiny", [])))


@functools.lru_cache(maxsize=None)
def plain_case(fmt, N, seed, with_nan_row=None):
    from oracle import similarity_oracle as so
    _, q, x = background(fmt, N, seed)
    if with_nan_row is not None:
        x[with_nan_row, 17] = np.nan
    tw, qn = so.prep_queries_np(q, None)
    with np.errstate(all="ignore"):
        xn = so.wnorms_np(x)
    return dict(q=q, tw=tw, qn=qn, x=x, xn=xn, planted={})


FEW_ROWS = (300, 1100, 1201)                             # the selection of the `few` case: two whole tiles live; 1100 holds a NaN


def floors(c, k=K):
    """thr0 of the floor case: the oracle's k-th best over the first 1024 rows, but 2.0 (above every score), NaN and -inf for
    queries 3, 4, 5."""
    thr = np.sort(exact_scores(c["tw"], c["qn"], c["x"][:1024], c["xn"][:1024]), axis=1)[:, -k].copy()
    thr[3], thr[4], thr[5] = 2.0, np.nan, -INF
    return thr
