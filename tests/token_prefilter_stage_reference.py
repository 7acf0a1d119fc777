"""Plain statements (numpy, float64 and integers) of what the PATCH-TOKEN route of the two-stage many-query search must do IMAGE
BY IMAGE -- the slices the host walks, the fold of the per-row sandwich into images, the exact threshold in force during every
slice, the parameters token_rescore_body publishes, the running list -- and the planted inputs that make the fold's every lane
and bit decide an image, for tests/test_token_prefilter_stage_{cpu,gpu}.py.  The code under test is the second half of
csrc/topk_prefilter.hip ("Patch-token banks").  Built on tests/prefilter_stage1_reference.py (row constants, query constants, half
widths, the sandwich and its slack, unchanged) and tests/token_search_reference.py (the contract's combined scores)."""
import functools

import numpy as np

from tests import prefilter_stage1_reference as sr
from tests import token_prefilter_select_reference as tps
from tests import token_search_reference as tsr

BT, SCAP, TOK_KMAX = sr.BT, sr.SCAP, 256
INF = sr.INF
PS = (1, 2, 4, 8, 16, 32, 64)


# ---------------------------------------------------------------------------------------------------------------- the schedule
def tile_images(t, N, P):
    """The images whose rows lie in bank tile t (P divides 256: an image never straddles a tile)."""
    return np.arange(t * BT // P, min((t + 1) * BT // P, N))


def token_schedule(N, P, k, n_live=None, direct_sel=None, last_live=0, tiles=None):
    """topk_tokens_prefiltered's launches as a pure function of the shape (and of the selection's live-tile list): T whole tiles
    (positions of the live list under a selection, the live tail tile not counted), direct_end, the five ends, and the slices
    [(t0, t1, 'direct' | 'staged', tail: the tail launch rides with it)].  `images` (when `tiles` is given, or without a
    selection): per slice the boolean mask [N] of the images stage 1 looks at in that slice."""
    R = N * P
    sel = n_live is not None
    T_tail = R // BT
    tail_live = R % BT != 0 and (not sel or bool(last_live))
    if sel:
        T = n_live - int(tail_live)
        direct_end = min(direct_sel, T)
    else:
        T = T_tail
        direct_end = min(max(-(-96 * k * P // BT), T // 128, 1), T)
    ends = [direct_end, T // 32, T // 8, T // 2, T]
    slices, t0 = [], 0
    for t1 in ends:
        if t1 <= t0:
            continue
        slices.append((t0, t1, "staged" if slices else "direct", bool(tail_live and t1 == T)))
        t0 = t1
    out = dict(T=T, direct_end=direct_end, ends=ends, slices=slices, tail_live=bool(tail_live))
    if sel and tiles is None:
        return out
    images = []
    for t0, t1, _, tail in slices:
        m = np.zeros(N, dtype=bool)
        for p in list(range(t0, t1)) + ([T] if tail else []):
            t = int(tiles[p]) if sel else (T_tail if p == T else p)
            m[tile_images(t, N, P)] = True
        images.append(m)
    out["images"] = images
    return out


# ---------------------------------------------------------------------------------------------------------------------- the fold
def image_sandwich(must_in_rows, must_out_rows, P, combine):
    """The per-row sandwich [Q, N P] folded into images [Q, N].  min: in iff every row is in, out iff any row is out; max: in iff
    any row is in, out iff every row is out.  A row the bound gives up on is in neither class (sandwich's rule), so it can make no
    image must-be-out under 'max' and decides nothing under 'min'."""
    Q = must_in_rows.shape[0]
    mi = np.asarray(must_in_rows, dtype=bool).reshape(Q, -1, P)
    mo = np.asarray(must_out_rows, dtype=bool).reshape(Q, -1, P)
    if combine == "min":
        must_in, must_out = mi.all(axis=2), mo.any(axis=2)
    else:
        assert combine == "max"
        must_in, must_out = mi.any(axis=2), mo.all(axis=2)
    assert not (must_in & must_out).any()
    return must_in, must_out


# ----------------------------------------------------------------------------------------------------------------- the thresholds
def kth_finite(sc, k):
    """[Q] float32: the k-th best of every row of sc [Q, M] among the entries above -inf; -inf when there are fewer than k."""
    s = np.asarray(sc, dtype=np.float32)
    if s.shape[1] < k:
        return np.full(s.shape[0], -INF, np.float32)
    return (-np.partition(-s, k - 1, axis=1)[:, k - 1]).astype(np.float32)


def slice_taus(scores, thr0, k, slices):
    """float32 [len(slices) + 1, Q]: entry i is the exact tau_q in force DURING slice i -- max(thr0 or -inf, the k-th best contract
    combined score over the images of all earlier slices), -inf while fewer than k images scoring above -inf are decided, a NaN
    thr0 counting as none -- and the last entry the same over all slices: what the search leaves in `tau`.  scores [Q, N]
    (deselected images already -inf), slices: boolean masks [N]."""
    scores = np.asarray(scores, dtype=np.float32)
    Q = scores.shape[0]
    floor = np.full(Q, -INF, np.float32) if thr0 is None else np.asarray(thr0, np.float32).copy()
    floor[np.isnan(floor)] = -INF
    seen = np.zeros(scores.shape[1], dtype=bool)
    out = [floor.copy()]
    for m in slices:
        seen = seen | np.asarray(m, dtype=bool)
        out.append(np.maximum(floor, kth_finite(np.where(seen[None, :], scores, np.float32(-INF)), k)))
    return np.array(out, dtype=np.float32)


def model_qpar(tau, qbase, eps=sr.EPS):
    """token_rescore_body's (and init_state_kernel's) publication restated in fp32, one operation per line: -> float32 [Q, 4]."""
    f = np.float32
    tau, qb = np.asarray(tau, f), np.asarray(qbase, f)
    with np.errstate(all="ignore"):
        t = np.where(tau > f(-3.0e38), tau, f(-3.0e38)).astype(f)
        a = (t * qb[:, 0]).astype(f)
        te = (t * f(eps)).astype(f)
        b = (te * qb[:, 2]).astype(f)
        da = (np.abs(a) * f(2.0 ** -19)).astype(f)
        a = (a - da).astype(f)
        db = (np.abs(b) * f(2.0 ** -19)).astype(f)
        b = (b - db).astype(f)
        a = np.where(a > f(-3.0e38), a, f(-3.0e38)).astype(f)
        c = (qb[:, 1] * f(1.0 + 2.0 ** -19)).astype(f)
    return np.stack([-a, c, -b, np.zeros_like(a)], axis=1).astype(f)


# ------------------------------------------------------------------------------------------------------------------ the running list
def orderable(s):
    u = sr.f32bits(s)
    return u ^ np.where(u >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def image_key(score, image):
    """The 64-bit key of the running list: larger = better score, then lower image."""
    key = (orderable(score).astype(np.uint64) << np.uint64(32)) | (~np.asarray(image).astype(np.uint32)).astype(np.uint64)
    return key.reshape(()) if np.ndim(score) == 0 and np.ndim(image) == 0 else key


def expected_list(scores_q, k):
    """The keys the list of one query must hold at the end: the k largest keys over the images scoring above -inf."""
    s = np.asarray(scores_q, dtype=np.float32)
    keys = image_key(s, np.arange(len(s)))[s > -INF]
    return set(np.sort(keys)[::-1][:k].tolist())


def key_parts(keys):
    """(score bits uint32, image int64) of list keys."""
    keys = np.asarray(keys, dtype=np.uint64)
    o = (keys >> np.uint64(32)).astype(np.uint32)
    return o ^ np.where(o >> 31, np.uint32(0x80000000), np.uint32(0xFFFFFFFF)), ((~keys) & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------ inputs
QSTAR = 3
KINDS = ("ordinary", "min-probe", "max-probe", "all-high", "all-low")


def shape_of(P, staged=False, tail=False):
    """(lead tiles of ordinary images, trailing tiles, tail images, k) of a planted case: single slice -- k large enough that
    ceil(96 k P / 256) reaches every whole tile; staged -- k = 1 and the 2 P + 1 planted tiles inside the last slice [T // 2, T)."""
    tail_images = min(5, BT // P - 1) if tail else 0
    if staged:
        return 2 * P + 14, 5, tail_images, 1                           # T = 4 P + 20, T // 2 = 2 P + 10 <= lead
    lead = max(4, 8 - 2 * P)
    T = lead + 2 * P + 1
    return lead, 0, tail_images, -(-T * BT // (96 * P))


@functools.lru_cache(maxsize=4)
def planted_case(P, combine, fmt, lo, D=128, seed=0, Q=24, staged=False, tail=False, k=None, ties=False, zero_q=None, nan_images=0,
                 unboundable_image=False):
    """A token bank for the designated query q* = QSTAR whose planted images make every token position and every image position
    of a 256-row tile decide an image on its own.  Ordinary rows: Gaussian images (a centre plus token noise).  Planted images are
    assembled from "high" tokens -- tw[q*] plus 5 % noise, rounded to `fmt`: cosine ~ 0.999 with q* -- and "low" tokens, their
    negation.  Tile layout: `lead` ordinary tiles, then for p = 0 .. P-1 one tile of min-probes (all high, token p low) and one of
    max-probes (all low, token p high) -- 256 / P image positions each --, one tile that holds two all-high and two all-low images
    among ordinary ones, `trail` ordinary tiles, and (tail) a partial tile with one image of each planted kind.
    thr0: per query the contract's k-th best combined score over the ordinary images of the lead tiles (a valid floor).
    Asserted here (a condition of the inputs, not a measurement): against the threshold in force while stage 1 looks at them --
    thr0 in a single slice, slice_taus' entry of the last slice when staged -- every min-probe and all-low image is must-be-out
    for q* under 'min', every max-probe must-be-in under 'max', every all-high image must-be-in and every all-low must-be-out under
    both; none is a don't-care.
    ties: query 0's best image gets a bit-identical copy on the other side of the last slice's boundary (an exact tie at the k-th
    place when k = 1: the lower image must win).
    zero_q: that query is all zero (flagged by the route).  nan_images: that many ordinary images get a NaN in one token.
    unboundable_image: ordinary image 1 gets an element the row bound gives up on (fp16: +inf; bf16: outside the window)."""
    from oracle import similarity_oracle as so
    rng = np.random.default_rng(1000 * seed + 10 * P + (combine == "max") + 2 * (fmt == "bf16") + 4 * lo)
    lead, trail, tail_images, k0 = shape_of(P, staged, tail)
    k = k0 if k is None else k
    ipt = BT // P
    T = lead + 2 * P + 1 + trail
    N = T * ipt + tail_images
    q = rng.standard_normal((Q, D), dtype=np.float32)
    if zero_q is not None:
        q[zero_q] = 0
    tw, qn = so.prep_queries_np(q, None)
    centre = rng.standard_normal((N, 1, D))
    x = centre + 0.7 * rng.standard_normal((N, P, D))
    kind = np.zeros(N, dtype=np.int64)
    probe_p = np.full(N, -1, dtype=np.int64)

    def high(n):
        return tw[QSTAR].astype(np.float64) * (1.0 + 0.05 * rng.standard_normal((n, D)))

    def plant(i, what, p=-1):
        h = high(P)
        if what == "min-probe":
            h[p] = -h[p]
        elif what == "max-probe":
            h = -h
            h[p] = -h[p]
        elif what == "all-low":
            h = -h
        x[i] = h
        kind[i], probe_p[i] = KINDS.index(what), p

    for p in range(P):
        for pos in range(ipt):
            plant((lead + 2 * p) * ipt + pos, "min-probe", p)
            plant((lead + 2 * p + 1) * ipt + pos, "max-probe", p)
    special = (lead + 2 * P) * ipt
    for j, what in enumerate(("all-high", "all-low", "all-low", "all-high")):
        plant(special + (j * (ipt - 1)) // 3, what)
    for j, what in enumerate(("min-probe", "max-probe", "all-low", "all-high")[:tail_images]):
        plant(T * ipt + j, what, P - 1 if "probe" in what else -1)
    xw = sr.store(x.reshape(N * P, D), fmt).reshape(N, P, D)
    low = (kind == KINDS.index("all-low")) | (kind == KINDS.index("min-probe")) | (kind == KINDS.index("max-probe"))
    assert low.any()                                                   # (negation is exact in both formats: low = -high to the bit)
    ordinary = np.flatnonzero(kind == 0)
    if nan_images:
        for j, i in enumerate(ordinary[5:5 + 7 * nan_images:7]):
            xw[i, j % P, (3 * j) % D] = np.nan
    if unboundable_image:
        xw[ordinary[1], P // 2, 9] = np.inf if fmt == "fp16" else sr.store(np.array([1e-30]), fmt)[0]
    sched = token_schedule(N, P, k)
    assert (len(sched["slices"]) > 1) == staged, sched
    if ties:
        with np.errstate(all="ignore"):
            g = int(np.argmax(tsr.combined_scores(q[:1], xw, combine)[0]))
        dst = int(ordinary[-1]) if not sched["images"][-1][g] else int(np.flatnonzero(sched["images"][0] & (kind == 0))[2])
        xw[dst] = xw[g]
        tie = (min(g, dst), max(g, dst))
        assert sched["images"][-1][tie[1]] and not sched["images"][-1][tie[0]]
    flat = np.ascontiguousarray(xw.reshape(N * P, D))
    with np.errstate(all="ignore"):
        xn = so.wnorms_np(flat)
        rows = so.cosine_scores_np(q, flat, None)                       # the contract's row scores, NaN kept
        combined = tsr.combine_scores(np.where(np.isnan(rows), np.float32(-INF), rows).astype(np.float32).reshape(Q, N, P), combine)
    qref = sr.query_constants(tw, qn, fmt, D, sr.eps_a_f32(fmt, D, lo))
    rref = sr.row_constants(flat, xn, fmt, D)
    den = sr.den32(qn, xn)
    score = sr.scores64(tw, flat, qn, xn)
    hw = sr.half_width(qref, rref, den)
    rows = np.where(np.isnan(score), np.float32(np.nan), rows)          # (the oracle reports a NaN score as -inf: no statement for it)
    sample = ordinary[ordinary < lead * ipt][:512]
    thr0 = kth_finite(combined[:, sample], k)
    assert (thr0 > -INF).all()
    c = dict(P=P, combine=combine, fmt=fmt, lo=lo, D=D, Q=Q, N=N, k=k, q=q, tw=tw, qn=qn, xw=xw, flat=flat, xn=xn, qref=qref, rref=rref,
             den=den, score=score, hw=hw, rows=rows, combined=combined, thr0=thr0, kind=kind, probe_p=probe_p, sched=sched,
             zero_q=zero_q, tie=tie if ties else None, T=T, ipt=ipt, lead=lead)
    # ---- the condition: every planted image in its class for q*, against the threshold in force in its slice
    taus = slice_taus(combined, thr0, k, sched["images"])
    in_last = sched["images"][-1]
    assert in_last[kind != 0].all()
    tau = taus[len(sched["slices"]) - 1]
    must_in, must_out = image_classes(c, tau)
    kq = lambda name: kind == KINDS.index(name)
    # (at P = 1 a max-probe IS an all-high image and a min-probe an all-low one)
    if combine == "min":
        assert must_out[QSTAR][kq("min-probe") | kq("all-low")].all()
        assert (must_out if P > 1 else must_in)[QSTAR][kq("max-probe")].all()
    else:
        assert must_in[QSTAR][kq("max-probe")].all() and must_out[QSTAR][kq("all-low")].all()
        assert (must_in if P > 1 else must_out)[QSTAR][kq("min-probe")].all()
    assert must_in[QSTAR][kq("all-high")].all()
    return c


def image_classes(c, tau, flags=None):
    """(must_in, must_out) [Q, N] of the case's images at thresholds tau [Q]; under a selection (flags per image) a deselected
    image is in neither class (check_sandwich's `allowed` forbids it outright)."""
    mi, mo = sr.sandwich(tau, c["score"], c["hw"], c["rows"])
    must_in, must_out = image_sandwich(mi, mo, c["P"], c["combine"])
    if flags is not None:
        must_in, must_out = must_in & flags[None, :], must_out & flags[None, :]
    return must_in, must_out


def fold_pass_bits(row_pass, P, combine, wrong=None, skip=None):
    """Candidate images [Q, N] from per-row pass bits [Q, N P].  wrong: 'or' under min / 'and' under max swaps the operation;
    skip = p: token p is left out of the fold (the planted defects of the CPU file; None, None is the right fold)."""
    r = np.asarray(row_pass, dtype=bool).reshape(row_pass.shape[0], -1, P)
    use_and = (combine == "min") != (wrong is not None)
    if skip is not None:
        r = r.copy()
        r[:, :, skip] = use_and
        if P == 1:
            return r[:, :, 0]
    return r.all(axis=2) if use_and else r.any(axis=2)


def lists_of(cand):
    return [np.flatnonzero(row) for row in cand]


def counts(must_in, must_out, listed=None, scope=None):
    """The numbers the GPU file records per case over the (query, image) pairs in `scope` (boolean [Q, N]; None: all): must-in,
    must-out, don't-care (and listed, listed / pairs)."""
    n = must_in.size if scope is None else int(scope.sum())
    out = dict(must_in=int(must_in.sum()), must_out=int(must_out.sum()), dont_care=int(n - must_in.sum() - must_out.sum()), pairs=int(n))
    if listed is not None:
        out.update(listed=int(listed), ratio=round(listed / n, 5))
    return out


# ---- the parameter sets of the GPU file (pinned here so that the CPU file checks the condition for every one of them)
def _single():
    out = []
    for ci, combine in enumerate(("min", "max")):                      # every P under both combines, tails spread over formats
        for n, P in enumerate(PS):
            fmt, lo = (("fp16", False), ("bf16", True), ("fp16", True), ("bf16", False))[(n + ci) % 4]
            out.append((P, combine, fmt, lo, (n + 2 * ci) % 3 != 0))
    return out


SINGLE = _single()                                                     # (P, combine, fmt, lo, tail)
STAGED = [(4, "min", "fp16", False), (4, "max", "bf16", True), (16, "max", "fp16", True), (16, "min", "bf16", False)]
TIES = (4, "max", "fp16", False)
ZERO_Q = 11


def single_case(P, combine, fmt, lo, tail):
    return planted_case(P, combine, fmt, lo, tail=tail)


def staged_case(P, combine, fmt, lo, ties=False):
    return planted_case(P, combine, fmt, lo, staged=True, tail=True, ties=ties, zero_q=ZERO_Q, Q=40 if P == 4 else 17)


def staged_floor(c):
    """The staged cases run with a floor under 'min' and without one under 'max'."""
    return c["thr0"] if c["combine"] == "min" else None


def open_case(P, combine, fmt):
    return planted_case(P, combine, fmt, False, tail=True, nan_images=6, seed=1)


SELECTED = [a for a in SINGLE if a[4]][::2] + [[a for a in SINGLE if a[4]][1]] + [a + ("staged",) for a in STAGED[1:3]]


def selected_case(args):
    P, combine, fmt, lo = args[:4]
    return planted_case(P, combine, fmt, lo, staged=args[-1] == "staged", tail=True, unboundable_image=True)


def selected_floor(c, flags):
    """thr0 under the selection: the contract's k-th best combined score over the selected ordinary images (a valid floor)."""
    thr0 = kth_finite(c["combined"][:, (c["kind"] == 0) & flags], c["k"])
    assert (thr0 > -INF).all()
    return thr0


def selection_of(c, seed=5):
    """A selection of the case's images that kills whole tiles (the first, two neighbours among the probes) and whose live list
    ends in the tail tile; ordinary image 1 -- the one that holds the unboundable row -- is deselected, the planted images of the
    tail stay."""
    rng = np.random.default_rng(seed)
    N, P, ipt = c["N"], c["P"], c["ipt"]
    f = rng.random(N) < 0.6
    for t in (0, c["lead"] + 1, c["lead"] + 2):
        f[t * ipt:(t + 1) * ipt] = False
    f[np.flatnonzero(c["kind"] == 0)[1]] = False
    assert N > c["T"] * ipt
    f[c["T"] * ipt:] = True
    return f


def selected_schedule(c, flags):
    """(tiles, cum, last_live, direct_end, schedule) of the case under the selection, from the restatement of the preparation."""
    N, P, k = c["N"], c["P"], c["k"]
    R = N * P
    _, tiles, cum, last_live = tps.prepare(np.zeros((-(-R // BT) * BT, 4), np.float32), flags, P)
    de = tps.direct_end(cum, len(tiles), k)
    return tiles, cum, last_live, de, token_schedule(N, P, k, len(tiles), de, last_live, tiles)


# ---- the preparation's shapes (part f): (P, tiles_all); N is no multiple of 32 and N P no multiple of 256
PREPARE_SHAPES = [(1, 2500), (2, 1025), (4, 1024), (8, 1023), (16, 65), (32, 64), (64, 63), (16, 1025), (64, 2500)]
PREPARE_SELECTIONS = ("half", "sparse", "last", "seam", "all")


def prepare_shape(P, tiles_all):
    """N images with (N P + 255) // 256 == tiles_all, N % 32 != 0 and N P % 256 != 0."""
    ipt = BT // P
    N = (tiles_all - 1) * ipt + ipt // 2                               # (ipt >= 4: the last tile is half full)
    while N % 32 == 0 or (N * P) % BT == 0:
        N += 1
    assert -(-N * P // BT) == tiles_all, (P, tiles_all, N)
    return N


def prepare_selection(kind, N, P, tiles_all, seed=0):
    rng = np.random.default_rng(seed + 17 * P + tiles_all)
    if kind == "half":
        return rng.random(N) < 0.5
    if kind == "sparse":
        return rng.random(N) < 0.01
    f = np.zeros(N, dtype=bool)
    if kind == "last":
        f[N - 1] = True
    elif kind == "seam":                                               # the images of tiles 1023 and 1024 (the last two of a smaller bank)
        a = min(1023, tiles_all - 2)
        f[a * BT // P:min((a + 2) * BT // P, N)] = True
    else:
        assert kind == "all"
        f[:] = True
    return f


def prepare_rowp(N, P, seed=0):
    """Random row constants [rows padded, 4] with some {0, inf, 1, 0} rows and the padding sentinel behind row N P."""
    rng = np.random.default_rng(seed + P)
    R = N * P
    rows = -(-R // BT) * BT
    rp = rng.standard_normal((rows, 4), dtype=np.float32)
    rp[rng.integers(0, R, size=max(R // 50, 1))] = (0.0, INF, 1.0, 0.0)
    rp[R:] = tps.SENTINEL
    return rp


def prepare_loop(rowp, flags, P):
    """tps.prepare said again: every row looks its image up, and a plain loop walks the tiles."""
    N = len(flags)
    R = N * P
    out = np.array(rowp, dtype=np.float32, copy=True)
    keep = np.zeros(rowp.shape[0], dtype=bool)
    keep[:R] = np.asarray(flags, dtype=bool)[np.arange(R) // P]
    out[~keep] = tps.SENTINEL
    tiles, cum, running = [], [], 0
    tiles_all = rowp.shape[0] // BT
    for t in range(tiles_all):
        n = int(np.count_nonzero(flags[t * BT // P:min((t + 1) * BT // P, N)]))
        running += n
        if n:
            tiles.append(t)
            cum.append(running)
    return out, np.array(tiles, np.int32), np.array(cum, np.int32), int(bool(tiles) and tiles[-1] == tiles_all - 1)
