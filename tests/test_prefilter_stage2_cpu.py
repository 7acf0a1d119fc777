"""CPU: tests/prefilter_stage2_reference.py held to account.  The case builders put every planted row where its case needs it,
by margins recomputed here from float64 exact scores and the library's own eps_a; every checker rejects the defect it exists for,
on synthetic arrays; BAND is as tight as its derivation says."""
import numpy as np
import pytest
import torch

from oracle import similarity_oracle as so
from sky_embeddings_amd import ops
from tests import prefilter_stage1_reference as sr
from tests import prefilter_stage2_reference as s2
from tests.prefilter_stage2_reference import BAND, INF, K

PLANTED = [(name, fmt, lo) for name in s2.WINDOWS for fmt in s2.FMTS for lo in (False, True)]
PLANTED_IDS = [f"{n}-{f}-{'hi+lo' if l else 'hi'}" for n, f, l in PLANTED]
MARGIN = 0.2                                             # half-widths: the issue's condition on both sides of every window


def lib_eps_a(fmt, lo):
    if fmt == "fp32":
        return ops.topk_prefilter_eps_a(s2.D, lo, False)
    return ops.topk_prefilter_eps_a_resident(s2.D, {"fp16": torch.float16, "bf16": torch.bfloat16}[fmt], lo)


def nextf(v, up=True):
    return float(np.nextafter(np.float32(v), np.float32(INF if up else -INF)))


# ---------------------------------------------------------------------------------------------------------------------------- pins
def test_exact_scores_and_topk_are_the_oracles():
    c = s2.unboundable_case("bf16")
    with np.errstate(all="ignore"):
        want = so.cosine_scores_np(c["q"], c["x"], None)
    want = np.where(np.isnan(want), np.float32(-INF), want)
    got = s2.exact_scores(c["tw"], c["qn"], c["x"], c["xn"])
    assert np.array_equal(sr.f32bits(got), sr.f32bits(want))
    assert np.isneginf(got[:, c["rows"]["nan"] + c["rows"]["inf"]]).all() and (got[:, c["rows"]["zero"]] == 0).all()
    assert np.sort(got[s2.PLANTED_Q])[-K] < 0                                     # the query whose k-th best is negative
    p = s2.plain_case("fp16", 2597, 500)
    ref_s, ref_i = so.cosine_topk_np(p["q"], p["x"], K, None)
    sc = s2.exact_scores(p["tw"], p["qn"], p["x"], p["xn"])
    for q in range(s2.Q):
        assert s2.same_answer(*s2.topk_of(sc[q], K, idx_offset=s2.OFFSET), ref_s[q], ref_i[q] + s2.OFFSET)
    # fewer rows than k, and the few rule: rows scoring -inf are returned without it (last, by row) and dropped with it
    few = np.zeros(2597, dtype=bool)
    few[[4, 9, 2000]] = True
    sq = sc[0].copy()
    sq[9] = -INF
    assert s2.topk_of(sq, K, few)[1].tolist() == sorted([4, 2000], key=lambda r: -sq[r]) + [9, -1, -1]
    assert s2.topk_of(sq, K, few, few=True)[1].tolist() == sorted([4, 2000], key=lambda r: -sq[r]) + [-1, -1, -1]


# ------------------------------------------------------------------------------------------------------------------ builder margins
@pytest.mark.parametrize("name,fmt,lo", PLANTED, ids=PLANTED_IDS)
def test_builder_margins(name, fmt, lo):
    """Scored by the reference alone (dot^ := the exact dot product, U = s + hw, L = s - hw with the library's eps_a): the planted
    query takes its path with 0.2 half-widths to spare on both sides of every window, and no candidate but the one whose U is the
    threshold (and its tie class) lies within BAND of a threshold."""
    c = s2.planted_case(name, fmt, lo)
    pq = s2.PLANTED_Q
    eps_a = lib_eps_a(fmt, lo)
    assert eps_a == sr.eps_a(fmt, s2.D, lo)
    den = sr.den32(c["qn"], c["xn"]).astype(np.float64)
    s = sr.scores64(c["tw"], c["x"], c["qn"], c["xn"])[pq]
    hw = s2.hw_of(c["tw"][pq:pq + 1], c["x"], den[pq:pq + 1], eps_a)[0]
    top, planted = c["top"], np.concatenate([c["top"]] + [g[0] for g in c["groups"]])
    rest = np.setdiff1d(np.arange(len(s)), planted)
    assert len(np.unique(planted)) == len(planted) and planted.max() == len(s) - 1          # the tail tile holds one
    if fmt == "fp16":                                        # no subnormal term in any planted row's nx': hw above is the device's
        assert (sr.lpr.count_subnormals(c["x"][planted].astype(np.float16)) == 0).all()
    s_k = s[top].min()
    assert abs(s_k - c["s_k"]) < 1e-12 and np.allclose(hw[planted], c["hw"], rtol=2e-3)
    assert (np.abs(np.sort(s[top]) - (0.8 + 1e-4 * np.arange(K))) <= 2.5e-5).all()
    assert s[rest].max() <= 0.5                                                              # everything else: c <= 0.5
    for rows, a, b in c["groups"]:
        h = hw[rows]
        assert (s[rows] >= s_k + a * h - 1e-9).all() and (s[rows] <= s_k + b * h + 1e-9).all()
    U, L = s + hw, s - hw
    L_k = np.sort(L)[-K]
    assert L_k == L[top].min()
    m = hw[planted].max() * MARGIN
    if name == "needed":
        assert (U[rest] < L_k - m).all()
        return
    window = np.concatenate([g[0] for g in c["groups"]])
    lo_w, hi_w = (-0.6, -0.2) if name == "quota-refused" else (-1.8, -1.2)
    assert len(window) == (500 if name == "ties" else 300)
    assert (s[window] >= s_k + lo_w * hw[window] - 1e-9).all() and (s[window] <= s_k + hi_w * hw[window] + 1e-9).all()
    assert (U[window] >= L_k + m).all()                      # all of them needed: the needed path cannot fit (k + 300 > 256)
    assert (s[window] <= s_k - m).all()                      # none of them among the k best
    assert (U[rest] < L_k - m).all()
    order = np.argsort(-U, kind="stable")
    uk = U[order[255]]
    if name == "quota-refused":
        assert uk >= s_k + m                                 # bound - s_k >= 0.2 hw: refused
    else:
        assert uk <= s_k - m                                 # s_k - bound >= 0.2 hw: certified
    # nobody but the threshold's own tie class within BAND of it
    cand = np.concatenate([planted, rest[U[rest] >= L_k - 2 * hw[rest]]])
    for thr, mult in ((uk, 1), (L_k, 2)):
        above, below = s2.sides(U[cand], L[cand], thr, BAND, mult)
        inside = cand[~above & ~below]
        own = U[inside] == thr if mult == 1 else L[inside] == thr
        if mult == 2:
            assert len(inside) == 0, inside
        else:
            assert own.all() and len(inside) == (400 if name == "ties" else 1), (len(inside), int(own.sum()))
    if name == "ties":
        copies = c["groups"][1][0]
        assert len(copies) == 400 and (c["x"][copies] == c["x"][copies[0]]).all() and (U[copies] == uk).all()
        assert (U > uk).sum() == 105                         # the k and the 100 distinct rows: 151 copies fill the quota


def test_other_builders():
    for fmt in s2.FMTS:
        c = s2.score_tie_case(fmt)
        sc = s2.exact_scores(c["tw"], c["qn"], c["x"], c["xn"])[s2.PLANTED_Q]
        assert len(np.unique(c["copies"] // 256)) == 2 * K and c["copies"].max() // 256 == (s2.N_OF[fmt] - 1) // 256
        assert s2.topk_of(sc, K)[1].tolist() == c["copies"][:K].tolist() and (sc[c["copies"]] == sc.max()).all()
        u = s2.unboundable_case(fmt)
        ref = sr.row_constants(u["x"], u["xn"], fmt, s2.D)
        every = set(u["unb"]) | set(u["rows"]["late"])
        want = every - (set(u["rows"]["nan"] + u["rows"]["late"][:1]) if fmt == "fp32" else set())   # (an fp32 NaN row is a `nanrow`: NaN nx')
        assert set(np.flatnonzero(ref["unb"]).tolist()) == want and set(np.flatnonzero(ref["nanrow"]).tolist()) == every - want
        assert max(u["rows"]["nan"] + u["rows"]["inf"]) < 2048 <= min(u["rows"]["late"])     # must-select rows: in the take-all slice
        assert np.sort(s2.exact_scores(u["tw"], u["qn"], u["x"], u["xn"])[s2.PLANTED_Q])[-K] < 0
    p = s2.plain_case("fp16", s2.N_OF["fp16"], 600, with_nan_row=s2.FEW_ROWS[1])
    thr = s2.floors(p)
    sc = s2.exact_scores(p["tw"], p["qn"], p["x"], p["xn"])
    assert thr[3] > sc[3].max() and np.isnan(thr[4]) and thr[5] == -INF and np.isfinite(thr[np.arange(s2.Q) > 5]).all()
    assert len({r // 256 for r in s2.FEW_ROWS}) == 2 and max(s2.FEW_ROWS) < 2560 - 256       # whole tiles only, k - 2 rows of them


# ----------------------------------------------------------------------------------------------------------------- planted defects
def quota_arrays(n=400, seed=0):
    """A synthetic list of n candidates with distinct U (fp32 numbers as float64), L = U - 0.02, k = 5: L_k = the 5th largest
    U - 0.02, and all but the lowest few are needed -> the quota path: the 256 largest U selected, bound = the 256th."""
    rng = np.random.default_rng(seed)
    U = s2.r32(np.sort(rng.uniform(0.59, 0.6, size=n))[::-1])
    assert len(np.unique(U)) == n
    rows = rng.permutation(5000)[:n].astype(np.int64)
    sel = rows[:256].copy()
    return rows, U, U - 0.02, sel, float(U[255])


def fs(rows, U, L, nsel, sel, bound, **kw):
    return s2.check_final_select(rows, U, L, K, nsel, sel, bound, np.ones(len(rows), bool), **kw)


def test_final_select_checker_rejects_planted_defects():
    rows, U, L, sel, bound = quota_arrays()
    assert fs(rows, U, L, 256, sel, bound) == (None, 1)                   # (the bound's own candidate is all the band leaves open)
    assert fs(rows, U, L, 256, sel, bound, band=0.0) == (None, 0)
    dup = sel.copy()
    dup[7] = dup[8]
    assert "twice" in fs(rows, U, L, 256, dup, bound)[0]
    alien = sel.copy()
    alien[0] = 6000
    assert "not in the list" in fs(rows, U, L, 256, alien, bound)[0]
    assert "nsel" in fs(rows, U, L, 257, np.concatenate([sel, rows[256:257]]), bound)[0]
    # a selected row missing although U > bound: the best row swapped for the 257th
    miss = sel.copy()
    miss[0] = rows[256]
    r = fs(rows, U, L, 256, miss, float(U[256]))
    assert r[0] and "left out" in r[0]
    # bound one ulp too small, visible where U is known to the bit: a tie class of 100 at the bound, split by the quota
    Ut = U.copy()
    Ut[200:300] = U[200]
    b = float(Ut[255])
    assert fs(rows, Ut, Ut - 0.02, 256, sel, b, band=0.0) == (None, 0)
    assert "left out" in fs(rows, Ut, Ut - 0.02, 256, sel, nextf(b, up=False), band=0.0)[0]
    assert "U < bound" in fs(rows, Ut, Ut - 0.02, 256, sel, nextf(b), band=0.0)[0]
    # ... and under the band the split tie class is one value, not 100 don't-cares
    ties = np.arange(len(rows))
    ties[200:300] = 200
    assert fs(rows, Ut, Ut - 0.02, 256, sel, b, ties=ties) == (None, 0)
    # the quota path taken with need == 200: L_k above all but the 200 largest U
    Lq = np.full(len(rows), 0.1)
    Lq[:K] = (U[199] + U[200]) / 2
    r = fs(rows, U, Lq, 256, sel, bound)
    assert r[0] and "only 200 candidates" in r[0]
    # the needed path: selected <=> U >= L_k, bound = -inf
    assert fs(rows, U, Lq, 200, rows[:200], -INF) == (None, 0)
    assert "left out, and bound = -inf" in fs(rows, U, Lq, 199, rows[:199], -INF)[0]
    assert "selected on the needed path" in fs(rows, U, Lq, 201, rows[:201], -INF)[0]
    assert "no k-th largest" in fs(rows, U, np.full(len(rows), -INF), 200, rows[:200], -INF)[0]
    assert "quota path needs" in fs(rows[:200], U[:200], L[:200], 200, rows[:200], 0.5)[0]
    # a sentinel candidate selected; and counted as live
    live = np.ones(len(rows), bool)
    live[3] = False
    Us, Ls = U.copy(), L.copy()
    Us[3], Ls[3] = -INF, -INF
    assert "does not count" in s2.check_final_select(rows, Us, Ls, K, 256, sel, bound, live)[0]
    ok = np.concatenate([sel[:3], sel[4:], rows[256:257]])
    assert s2.check_final_select(rows, Us, Ls, K, 256, ok, float(U[256]), live)[0] is None


def test_band_is_tight():
    assert BAND < 2.0 ** -18 and BAND >= 6 * 2.0 ** -24
    rows, U, L, sel, bound = quota_arrays()
    # an unselected candidate one ulp-of-2^-18 above the bound is caught; one inside the band is a don't-care
    Ub = U.copy()
    Ub[256] = bound * (1 + 2.0 ** -18)
    assert "left out" in fs(rows, Ub, Ub - 0.02, 256, sel, bound)[0]
    Ub[256] = bound * (1 + 2.0 ** -23)
    assert fs(rows, Ub, Ub - 0.02, 256, sel, bound) == (None, 2)
    Ub = U.copy()
    Ub[100] = bound * (1 - 2.0 ** -18)
    assert "U < bound" in fs(rows, Ub, Ub - 0.02, 256, sel, bound)[0]


def test_intervals_statement():
    """The formula on hand-made constants: scale, widening, NaN, and the sentinel under a selection only."""
    qb = np.array([3.0, 0.5, 0.25, 6.0], np.float32)                     # {qn 2^-f, y, 2^-f = 1/4, qn}
    rowp = np.array([[2.0, 4.0, 0.5, 0], [0, INF, 1, 0], [0, np.nan, 0, 0], [1.0, 0.0, 1.0, 0]], np.float32)
    xn = np.array([1.0, np.nan, 1.0, 0.0], np.float32)
    cd = np.array([10.0, 1.0, -INF, -3.0], np.float32)
    U, L = s2.intervals(cd, [0, 1, 2, 3], qb, rowp, xn, eps=0.5, sel=True)
    w = 2.0 ** -21
    assert U[0] == s2.r32((10 + 2) * 8 / 6.5 * (1 + w)) and L[0] == s2.r32((10 - 2) * 8 / 6.5 * (1 - w))
    assert U[1] == INF and L[1] == -INF                                   # unboundable: never dropped
    assert U[2] == -INF and L[2] == -INF and s2.counting([0, 1, 2, 3], rowp, True).tolist() == [True, True, False, True]
    assert U[3] == s2.r32(-3 * 4 / 0.5 * (1 - w)) and L[3] == s2.r32(-3 * 4 / 0.5 * (1 + w))
    U2, _ = s2.intervals(cd, [0, 1, 2, 3], qb, rowp, xn, eps=0.5, sel=False)
    assert U2[2] == INF and s2.counting([2], rowp, False).all()           # without a selection nothing is a sentinel
    t = s2.tie_classes(np.array([1, 1, 1, 2], np.float32), [0, 0, 3, 0], rowp, xn)
    assert t[0] == t[1] and len(set(t.tolist())) == 3


def rescore_arrays():
    rng = np.random.default_rng(3)
    tw = rng.standard_normal(16).astype(np.float32)
    x = rng.standard_normal((50, 16)).astype(np.float32)
    x[20], x[40] = x[10], x[10]                                           # three equal scores
    x[33, 2] = np.nan
    xn = so.wnorms_np(np.nan_to_num(x))
    qn = np.float32(np.linalg.norm(tw))
    sc = s2.exact_scores(tw[None], np.array([qn]), x, xn)[0]
    return tw, qn, x, xn, sc


def test_rescore_checker_rejects_planted_defects():
    tw, qn, x, xn, sc = rescore_arrays()
    sel = np.array([40, 3, 10, 33, 20, 7, 12, 45])
    best = int(np.argmax(np.where(np.isin(np.arange(50), sel), sc, -INF)))
    x[[10, 20, 40]] = x[best] if best not in (10, 20, 40) else x[10]     # the equal scores are the best ones: ranks 0 .. 2 (or 3)
    sc = s2.exact_scores(tw[None], np.array([qn]), x, xn := so.wnorms_np(np.nan_to_num(x)))[0]
    off = s2.OFFSET
    want_s, want_i = s2.topk_of(np.where(np.isin(np.arange(50), sel), sc, -INF), 5, np.isin(np.arange(50), sel), idx_offset=off)
    assert set((want_i[:3] - off).tolist()) <= {10, 20, 40, best} and (np.diff(want_i[:3]) > 0).all()
    chk = lambda s, i, k=5, few=False, rows=sel: s2.check_rescore(rows, tw, qn, x, xn, k, off, s, i, few)
    assert chk(want_s, want_i) is None
    assert s2.check_rescore(sel, None, None, None, None, 5, off, want_s, want_i, False, scores=sc) is None
    one = want_s.copy()
    one[2] = np.nextafter(one[2], np.float32(INF))
    assert "rank 2" in chk(one, want_i)                                  # a score one ulp off
    desc = want_i.copy()
    desc[[0, 1]] = desc[[1, 0]]
    assert "rank 0" in chk(want_s, desc)                                 # two equal scores in row-descending order
    assert "rank 0" in chk(want_s, want_i & 0xFFFFFFFF)                  # out_i missing the offset's high word
    others = sel[sel != want_i[4] - off]                                 # scored from other rows than the selected: the 5th is not theirs
    assert "rank 4" in chk(want_s, want_i, rows=others)
    # fewer than k rows: the tail from n, the -inf scorer returned last; under few from `have`, the -inf scorer not returned
    three = np.array([33, 7, 12])
    ws, wi = s2.topk_of(np.where(np.isin(np.arange(50), three), sc, -INF), 5, np.isin(np.arange(50), three), idx_offset=off)
    assert wi[2] == 33 + off and wi[3] == -1 and chk(ws, wi, rows=three) is None
    assert "rank 2" in chk(ws, wi, few=True, rows=three)                 # a few tail that returns a -inf scorer
    fs_, fi = ws.copy(), wi.copy()
    fi[2] = -1
    assert chk(fs_, fi, few=True, rows=three) is None and "rank 2" in chk(fs_, fi, rows=three)


def test_certificate_checker_rejects_planted_defects():
    out_s = np.array([0.9, 0.8, 0.7, 0.6, 0.5], np.float32)
    cc = s2.check_certificate
    assert cc(out_s, -INF, 0, 17, 5, False, 0) is None and cc(out_s, nextf(0.5, up=False), 0, 256, 5, False, 0) is None
    assert "expected 1" in cc(out_s, 0.5, 0, 256, 5, False, 0)           # redo == 0 with out_s[k-1] == bound: the comparison is strict
    assert cc(out_s, 0.5, 0, 256, 5, False, 1) is None
    assert "expected 0" in cc(out_s, -INF, 0, 17, 5, False, 1)           # redo == 1 with nothing to justify it
    assert "expected 0" in cc(out_s, nextf(0.5, up=False), 0, 256, 5, False, 1)
    assert "expected 1" in cc(out_s, -INF, 1, 17, 5, False, 0)           # overflow reaches the certificate
    assert "expected 1" in cc(out_s, -INF, 0, 3, 5, False, 0) and cc(out_s, -INF, 0, 3, 5, False, 1) is None
    assert cc(out_s, -INF, 0, 3, 5, True, 0) is None and "expected 0" in cc(out_s, -INF, 0, 3, 5, True, 1)
    assert "expected 1" in cc(out_s, 0.1, 0, 3, 5, True, 0) and "expected 1" in cc(out_s, -INF, 1, 3, 5, True, 0)


def test_soundness_checker_rejects_planted_defects():
    sc = np.linspace(0.0, 0.99, 100).astype(np.float32)
    rows = np.arange(60, 100)
    live = np.ones(40, bool)
    sel = np.arange(90, 100)
    want = s2.topk_of(sc, 5)
    cs = lambda **kw: s2.check_soundness(**{**dict(rows=rows, live=live, sel_rows=sel, score_q=sc, k=5, nsel=10, bound=float(sc[89]), redo=0,
                                                   out_s=want[0], out_i=want[1], want_s=want[0], want_i=want[1]), **kw})
    assert cs() is None and cs(bound=-INF) is None
    assert "scores" in cs(bound=float(sc[88]))                            # a bound that does not dominate what was left out
    assert "scores" in cs(bound=-INF, sel_rows=np.array([99, 98, 97, 96, 94]), nsel=5, redo=1,
                          out_s=sc[[99, 98, 97, 96, 94]], out_i=np.array([99, 98, 97, 96, 94]))
    assert "not the oracle's" in cs(out_i=want[1][::-1].copy())
    assert cs(out_i=want[1][::-1].copy(), redo=1) is None
