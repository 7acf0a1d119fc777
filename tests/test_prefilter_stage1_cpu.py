"""CPU: the statements of tests/prefilter_stage1_reference.py stand on their own -- the phase table the GPU file relies on is the
driver's schedule, the layout export ends where the workspace ends, every integer-grid case meets its exactness budget and is
what the statements of the query and row constants make of it, every sandwich case leaves at most 2 % of a query's rows
undecided -- and each checker rejects the defect it exists for."""
import ctypes

import numpy as np
import pytest

from sky_embeddings_amd import ops
from tests import prefilter_stage1_reference as sr

K = sr.K


# ------------------------------------------------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize("key", list(sr.PHASES), ids=lambda k: f"N{k[0]}-{'thr0' if k[1] else 'nofloor'}-{'resident' if k[2] else 'fp32'}")
def test_phase_table_is_the_drivers_schedule(key):
    N, thr0, resident = key
    s = sr.schedule(N, K, thr0, resident)
    T = N // 256 if resident else -(-N // 256)
    assert (s["cap"], s["first"], s["direct_end"], s["T"]) == (4096, 8, 9, T)
    assert s["ends"] == [8, 9, T // 32, T // 8, T // 2, T] and s["has_tail"] == (resident and N % 256 != 0)
    assert s["first_rows"] == 2048
    assert s["launches"] == sr.PHASES[key]
    # what the GPU file relies on: a final select never follows a compaction of a take-all slice unless the table says so
    if not thr0 and T == 8:
        assert ("select", 0) not in s["launches"]                 # the take-all slots are still in place when the call returns


@pytest.mark.parametrize("n_live", [9, 8])
def test_phase_table_under_a_selection(n_live):
    s = sr.schedule(2560, K, False, True, n_live=n_live, last_live=1)
    assert s["launches"] == sr.PHASES_SEL[n_live] and not s["has_tail"] and s["first_rows"] == 2048
    flags = sr.selection(2560, (3,) if n_live == 9 else (3, 6), 5)
    live = [t for t in range(10) if flags[t * 256:(t + 1) * 256].any()]
    assert len(live) == n_live and live[-1] == 9 and 0.4 < flags.mean() < 0.5


def test_larger_k_moves_the_direct_slice():
    """The table holds for k = 5 only: the direct slice ends at ceil(96 k / 256) tiles once that exceeds first + 1."""
    assert sr.schedule(2560, 25, False, False)["launches"] == [("mode0", 0, 8), ("select", 0), ("mode1", 8, 10), ("select", 1)]
    assert sr.schedule(2560, 200, False, False)["cap"] == 8192


# ---------------------------------------------------------------------------------------------------------------------- the layout
SIZES = dict(qh=lambda Q, Qp, D, cap, capw: Qp * D * 2, ql=lambda Q, Qp, D, cap, capw: Qp * D * 2, qbase=lambda Q, Qp, D, cap, capw: Q * 16,
             qpar=lambda Q, Qp, D, cap, capw: Qp * 16, tau=lambda Q, *_: Q * 4, bound=lambda Q, *_: Q * 4, cnt=lambda Q, *_: Q * 4,
             overflow=lambda Q, *_: Q * 4, nsel=lambda Q, *_: Q * 4, sel_i=lambda Q, *_: Q * 256 * 4,
             cand_i=lambda Q, Qp, D, cap, capw: Q * cap * 4, cand_d=lambda Q, Qp, D, cap, capw: Q * cap * 4,
             wg_list=lambda Q, Qp, D, cap, capw: 256 * capw * 16, wg_count=lambda *_: 256 * 4)


@pytest.mark.parametrize("Q,D,k", [(261, 128, K), (261, 288, K), (1300, 128, K), (1300, 192, K), (700, 192, K), (300, 128, K), (2100, 128, 200)])
def test_layout_export_ends_where_the_workspace_ends(Q, D, k):
    lay = ops.topk_prefilter_ws_layout(Q, D, k)
    Qp = -(-Q // 256) * 256
    assert lay["cap"] == sr.cap_of(k) and lay["capw"] == max(4 * Q, 8192)
    offs = [lay[f] for f in ops.WS_FIELDS]
    assert offs[0] == 0 and offs == sorted(offs) and all(o % 256 == 0 for o in offs)
    ends = offs[1:] + [ops.lib().skyemb_topk_prefilter_ws_bytes(Q, D, k)]
    for f, o, e in zip(ops.WS_FIELDS, offs, ends):
        size = SIZES[f](Q, Qp, D, lay["cap"], lay["capw"])
        assert e - o == -(-size // 256) * 256, (f, o, e, size)     # the last line: last offset + size = skyemb_topk_prefilter_ws_bytes


def test_layout_export_refuses_another_count():
    out = (ctypes.c_int64 * 17)(*([-5] * 17))
    for n in (0, 15, 17):
        assert ops.lib().skyemb_topk_prefilter_ws_layout(300, 128, K, ctypes.addressof(out), n) != 0
        assert b"16 values" in ops.lib().skyemb_last_error() and list(out) == [-5] * 17
    assert ops.lib().skyemb_topk_prefilter_ws_layout(300, 128, K, None, 16) != 0


@pytest.mark.parametrize("D", [128, 192, 288])
def test_eps_a_is_the_librarys(D):
    import torch
    for lo in (False, True):
        assert sr.eps_a("fp32", D, lo) == ops.topk_prefilter_eps_a(D, lo, False)
        assert sr.eps_a("fp16", D, lo) == ops.topk_prefilter_eps_a(D, lo, True) == ops.topk_prefilter_eps_a_resident(D, torch.float16, lo)
        assert sr.eps_a("bf16", D, lo) == ops.topk_prefilter_eps_a_resident(D, torch.bfloat16, lo)


# ------------------------------------------------------------------------------------------------------------------ the grid cases
@pytest.mark.parametrize("D", [128, 192])
@pytest.mark.parametrize("lo", [False, True], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("fmt", sr.FMTS)
def test_grid_case_is_exact_and_is_what_the_statements_make_of_it(fmt, lo, D):
    """exact_grid_case asserts its own bit budget; here its construction is held to the statements: the query split recovers H
    and L, 2^-f is the case's, the image of an fp32 row is m 2^12 or m 2^13, and both pass counts differ."""
    Q, N = (700 if lo else 1300), sr.TAKE_ALL_N[fmt]
    g = sr.exact_grid_case(fmt, lo, Q, N, D, seed=D + lo)
    ofmt = "bf16" if fmt == "bf16" else "fp16"
    qref = sr.query_constants(g["tw"], np.ones(Q, np.float32), fmt, D, sr.eps_a_f32(fmt, D, lo))
    assert sr.same16(qref["qh"], sr.bits16(g["H"], ofmt)) is None and sr.same16(qref["ql"], sr.bits16(g["L"], ofmt)) is None
    assert np.array_equal(qref["s"], np.ldexp(np.float32(1), -g["f"]).astype(np.float32)) and not qref["flagged"].any()
    rref = sr.row_constants(g["x"], np.ones(N, np.float32), fmt, D)
    assert not rref["unb"].any() and not rref["nanrow"].any()
    if fmt == "fp32":
        img = rref["image"].astype(np.float64)
        assert np.array_equal(img, g["x"].astype(np.float64) * np.ldexp(1.0, -rref["e"])[:, None])
        assert set(np.unique(np.abs(img[img != 0]) / 2.0 ** 12)) <= {1.0, 2.0, 3.0} and np.array_equal(g["rexp"] >= 12, np.ones(N, bool))
    else:
        assert (rref["scale"] == 1).all()
    # dot^ restated from the statements' own images, in float64 (exact: integers below 2^24 times a power of two)
    a = sr.widen16(qref["qh"], ofmt).astype(np.float64) + (sr.widen16(qref["ql"], ofmt).astype(np.float64) if lo else 0.0)
    b = rref["image"].astype(np.float64) if fmt == "fp32" else g["x"].astype(np.float64)
    assert np.array_equal((a[:64] @ b.T).astype(np.float32), g["dot"][:64])
    assert g["dot"].shape == (Q, N) and (g["dot"] != g["dot_other"]).mean() > 0.99


def test_grid_budget_fails_where_it_must():
    """D = 352 > 341 breaks the fp16 budget: the function's own assertion is what says so."""
    with pytest.raises(AssertionError):
        sr.exact_grid_case("fp16", True, 300, 256, 352, seed=0)
    sr.exact_grid_case("bf16", True, 64, 256, 352, seed=0)


def test_chain_all_is_the_reference_chain():
    from tests import prefilter_lp_reference as lpr
    rng = np.random.default_rng(3)
    tw, x = rng.standard_normal((5, 96), dtype=np.float32), rng.standard_normal((40, 96), dtype=np.float32)
    got = sr.chain_all(tw, x)
    for q in range(5):
        assert np.array_equal(got[q].view(np.uint32), lpr.fma_chain(tw[q], x).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------- the sandwich cases
@pytest.mark.parametrize("lo", [False, True], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("fmt", sr.FMTS)
def test_sandwich_cases_leave_little_undecided(fmt, lo):
    """The condition on the inputs: at most 2 % of a query's rows in the don't-care band, at least k must-be-in rows -- at the
    known floor of the MODE 2 case, and over the whole window in which the device may publish tau for the others."""
    c = sr.pair_case(fmt, lo, sr.SQ, 2048, sr.SD, sr.sandwich_seed(fmt))
    thr0 = sr.floor_of_first_rows(c, 1024, K)
    must_in, must_out = sr.sandwich(thr0, c["score"], c["hw"], c["contract"])
    share = (~must_in & ~must_out).mean(axis=1)
    print(fmt, lo, "mode2: don't-care share max", share.max(), "must-in min", must_in.sum(axis=1).min(), "median hw", np.median(c["hw"]))
    assert share.max() <= 0.02 and must_in.sum(axis=1).min() >= K
    assert (must_out.mean(axis=1) > 0.9).all()                    # and the threshold is worth something
    for N, seen in ((2304, 2048), (2560, 2304)):
        c = sr.pair_case(fmt, lo, sr.SQ, N, sr.SD, sr.sandwich_seed(fmt))
        tau_lo, tau_hi = sr.tau_window(c, np.arange(N) < seen, K)
        must_in, must_out, share = sr.sandwich_window(c, tau_lo, tau_hi)
        print(fmt, lo, N, "don't-care share max", share.max(), "must-in min", must_in.sum(axis=1).min())
        assert share.max() <= 0.02 and must_in.sum(axis=1).min() >= K and (must_out.mean(axis=1) > 0.9).all()


@pytest.mark.parametrize("lo", [False, True], ids=["hi", "hi+lo"])
def test_sandwich_case_under_a_selection(lo):
    c = sr.pair_case("fp16", lo, sr.SQ, 2560, sr.SD, sr.sandwich_seed("fp16"))
    flags = sr.selection(2560, (3,), 5)
    live = [t for t in range(10) if flags[t * 256:(t + 1) * 256].any()]
    seen = flags & (np.arange(2560) < (live[7] + 1) * 256)          # the selected rows of the first eight live tiles
    tau_lo, tau_hi = sr.tau_window(c, seen, K)
    must_in, must_out, share = sr.sandwich_window(c, tau_lo, tau_hi, allowed=flags)
    assert share.max() <= 0.02 and must_in.sum(axis=1).min() >= K and not must_in[:, ~flags].any()


# --------------------------------------------------------------------------------------------------------------- planted defects
def _rows(fmt, D=128, N=300):
    q, w, x = sr.gaussian_case(fmt, 8, N, D, 99, subnormal_rows=2 if fmt == "fp16" else 0)
    x = x.copy()
    x[5] = 0
    x[6, 3] = np.inf
    xn = np.sqrt((x.astype(np.float64) ** 2 * w).sum(axis=1)).astype(np.float32)
    return sr.row_constants(x, xn, fmt, D)


@pytest.mark.parametrize("fmt", sr.FMTS)
def test_row_checker_rejects_planted_defects(fmt):
    ref = _rows(fmt)
    good = sr.model_rowp(ref, 512)
    assert sr.check_rowp(good, ref) is None
    assert ref["unb"][6] and not ref["unb"][5] and (good[5] == 0).sum() >= 2
    i = 17
    bad = good.copy()                                              # nx' one ulp below the float64 norm
    f = np.float32(ref["nx_lo"][i])
    bad[i, 1] = f if float(f) < ref["nx_lo"][i] else np.nextafter(f, np.float32(0))
    assert float(bad[i, 1]) < ref["nx_lo"][i] and "not an upper bound" in sr.check_rowp(bad, ref)
    bad = good.copy()                                              # a sentinel row that is finite
    bad[300 + 44, 1] = 1.0
    assert "sentinel" in sr.check_rowp(bad, ref)
    bad = good.copy()                                              # an unboundable row with a finite norm
    bad[6] = (0.0, 3.0e38, 1.0, 0.0)
    assert "unboundable" in sr.check_rowp(bad, ref)
    bad = good.copy()                                              # a neighbour's scale / weighted norm
    bad[i, [0, 2]] = good[i + 1, [0, 2]] * np.float32(2)
    assert sr.check_rowp(bad, ref) is not None
    bad = good.copy()                                              # an nx' far above what the roundings allow (a doubled term)
    bad[i, 1] *= np.float32(1.001)
    assert "exceeds" in sr.check_rowp(bad, ref)
    if fmt == "fp32":
        img = ref["image"].view(np.uint16).copy()
        pad = np.zeros((512, 128), np.uint16)
        pad[:300] = img
        assert sr.check_image(pad, ref) is None
        pad[9, 77] ^= 1
        assert "differ" in sr.check_image(pad, ref)
        pad[9, 77] ^= 1
        pad[400, 0] = 1
        assert "padding" in sr.check_image(pad, ref)
    if fmt == "fp16":
        sub = np.flatnonzero(~ref["unb"] & (ref["nx_lo"] > ref["norm"] * 1.5))    # the planted subnormal rows: the additive term dominates
        assert len(sub) >= 1
        bad = good.copy()
        bad[sub[0], 1] = np.float32(ref["norm"][sub[0]] * (1 + 128 * 2.0 ** -22) * 1.0001)      # the term forgotten
        assert "not an upper bound" in sr.check_rowp(bad, ref)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_query_checker_rejects_planted_defects(fmt):
    rng = np.random.default_rng(4)
    Q, D = 261, 128
    tw = rng.standard_normal((Q, D), dtype=np.float32)
    tw[7] = 0
    qn = np.abs(rng.standard_normal(Q, dtype=np.float32)) + 1
    e32 = sr.eps_a_f32(fmt, D, True)
    ref = sr.query_constants(tw, qn, fmt, D, e32)
    qh, ql = np.zeros((512, D), np.uint16), np.zeros((512, D), np.uint16)
    qh[:Q], ql[:Q] = ref["qh"], ref["ql"]
    qb = sr.model_qbase(ref)
    assert sr.check_query(qh, ql, qb, ref) is None and (ql[:Q] != 0).mean() > 0.9
    # qbase.y without its (1 + D 2^-22): the kernel's arithmetic minus the factor -- fp32 sum of squares, sqrtf, one product
    bad = qb.copy()
    qp = (tw * ref["s"][:, None]).astype(np.float32)
    bad[:, 1] = np.float32(e32) * np.sqrt((qp * qp).sum(axis=1, dtype=np.float32))
    assert "is below eps_a" in sr.check_query(qh, ql, bad, ref)
    assert "second pass" in sr.check_query(qh, np.zeros_like(ql), qb, ref, lo=True)      # ql zeroed under hi + lo
    bad = qb.copy()
    bad[3, 0] = qb[3, 3]                                           # qn in the place of qn 2^-f
    assert (ref["s"][3] != 1) and "qbase[3].x" in sr.check_query(qh, ql, bad, ref)
    bad_h = qh.copy()
    bad_h[300, 5] = 0x3C00                                         # a padding row that is not zero
    assert "padding" in sr.check_query(bad_h, ql, qb, ref)
    flags = ref["flagged"].astype(np.int32)
    assert sr.check_flags(flags, flags, ref) is None and not flags.any()
    flags[7] = 1
    assert "overflow[7]" in sr.check_flags(flags, flags, ref)


def test_scale_rules_of_the_planted_queries():
    D = 128
    tw = np.zeros((5, D), np.float32)
    tw[0, 3], tw[1, 3], tw[2, 3], tw[3, 3] = 2.0 ** -120, 2.0 ** -51, 2.0 ** 80, 1.5
    for fmt, want in (("fp16", [1, 0, 0, 0, 0]), ("bf16", [1, 1, 1, 0, 0])):
        ref = sr.query_constants(tw, np.ones(5, np.float32), fmt, D, sr.eps_a_f32(fmt, D, False))
        assert ref["flagged"].tolist() == [bool(v) for v in want], (fmt, ref["s"])
    assert ref["s"].tolist() == [2.0 ** 99, 2.0 ** 30, 2.0 ** -100, 2.0 ** -21, 1.0]


def test_bf16_window_edges():
    D = 128
    step = 2.0 ** -7
    vals = [2.0 ** -60, 2.0 ** -60 * (1 + step), 2.0 ** -60 * (1 - step / 2), 2.0 ** 120, 2.0 ** 120 * (1 - step / 2), 2.0 ** 120 * (1 + step)]
    x = np.zeros((len(vals) + 2, D), np.float32)
    x[:, 0] = 1.0
    for i, v in enumerate(vals):
        x[i, 9] = v
    assert np.array_equal(sr.store(x, "bf16"), x)                 # every planted value is a bf16 number
    xn = np.ones(len(x), np.float32)
    xn[-2], xn[-1] = np.inf, np.nan
    ref = sr.row_constants(x, xn, "bf16", D)
    assert ref["unb"].tolist() == [False, False, True, True, False, True, True, True]


def test_list_checkers_reject_planted_defects():
    g = sr.exact_grid_case("fp16", True, 40, 2048 + 44, 128, seed=1)
    Q, N, cap = 40, 2092, 4096
    dot = g["dot"]
    cnt = np.full(Q, N, np.int32)
    ci = np.full((Q, cap), -1515870811, np.int32)
    cd = np.full((Q, cap), np.nan, np.float32)
    ci[:, :2048], cd[:, :2048] = np.arange(2048), dot[:, :2048]
    order = np.random.default_rng(0).permutation(44) + 2048
    ci[:, 2048:N], cd[:, 2048:N] = order, dot[:, order]
    assert sr.check_take_all(cnt, ci, cd, dot, 2048) is None and sr.check_tail_appends(cnt, ci, cd, dot, 2048, N) is None
    bad = cd.copy()                                                # one dot^ swapped with its neighbour row's
    bad[11, [100, 101]] = bad[11, [101, 100]]
    assert dot[11, 100] != dot[11, 101] and "query 11, slot 100" in sr.check_take_all(cnt, ci, bad, dot, 2048)
    assert "differ" in sr.check_take_all(cnt, ci, cd, g["dot_other"], 2048)     # the lo pass missing altogether
    bad = ci.copy()                                                # cand_i[q][slot] != slot in a take-all list
    bad[3, 77] = 78
    assert "cand_i[3][77]" in sr.check_take_all(cnt, bad, cd, dot, 2048)
    bad = ci.copy()                                                # a tail row twice, another missing
    bad[5, 2050] = bad[5, 2051]
    assert "once each" in sr.check_tail_appends(cnt, bad, cd, dot, 2048, N)
    bad = ci.copy()
    bad[5, 2050] = N + 3                                           # a padding row appended
    assert "once each" in sr.check_tail_appends(cnt, bad, cd, dot, 2048, N)
    assert "cnt[0]" in sr.check_tail_appends(cnt + 1, ci, cd, dot, 2048, N)
    # the sandwich
    c = sr.pair_case("fp16", False, sr.SQ, 2048, sr.SD, sr.sandwich_seed("fp16"))
    must_in, must_out = sr.sandwich(sr.floor_of_first_rows(c, 1024, K), c["score"], c["hw"], c["contract"])
    lists = [np.flatnonzero(~must_out[q]) for q in range(sr.SQ)]  # everything not provably out: a legal list
    assert sr.check_sandwich(lists, must_in, must_out) is None
    assert sr.check_sandwich([np.flatnonzero(must_in[q]) for q in range(sr.SQ)], must_in, must_out) is None      # and the least legal one
    bad = list(lists)
    gone = int(np.flatnonzero(must_in[9])[0])
    bad[9] = lists[9][lists[9] != gone]                            # one must-be-in row missing
    assert f"query 9: row {gone}" in sr.check_sandwich(bad, must_in, must_out)
    bad = list(lists)
    bad[2] = np.append(lists[2], np.flatnonzero(must_out[2])[0])   # a must-be-out row present
    assert "query 2" in sr.check_sandwich(bad, must_in, must_out) and "below the threshold" in sr.check_sandwich(bad, must_in, must_out)
    bad = list(lists)
    bad[4] = np.append(lists[4], lists[4][0])
    assert "twice" in sr.check_sandwich(bad, must_in, must_out)
    allowed = np.ones(2048, bool)
    allowed[lists[0][0]] = False
    assert "deselected" in sr.check_sandwich(lists, must_in, must_out, allowed)
    # the pair bound
    qr, rr = c["qref"], c["rref"]
    cs = sr.chain_scaled(sr.chain_all(c["tw"][:20], c["x"]), dict(s=qr["s"][:20]), rr)
    ok, ratio = sr.check_pair_bound(cs.astype(np.float32), cs, qr["y_lo"][:20], rr["nx_lo"])
    assert ok is None and ratio < 0.01
    off = cs.astype(np.float32)
    off[3, 5] += np.float32(2.5 * qr["y_hi"][3] * rr["nx_hi"][5])
    assert "query 3, row 5" in sr.check_pair_bound(off, cs, qr["y_lo"][:20], rr["nx_lo"])[0]
