"""GPU: the weighted-MSE forms of the two-stage token search QUANTITY BY QUANTITY, against the statements of
tests/token_mse_stage_reference.py: the shared-weight query images and constants (mse_query_kernel), the first test row, threshold
and flags (mse_state_kernel), every dot^ of both routes to the bit on integer-grid inputs and inside the proven bound on ordinary
ones, the candidate lists of a direct slice at a known threshold image by image, the state token_rescore_body<DIST> republishes after
staged slices, the counting fold under top_t and the lists under a selection.  tests/test_token_mse_stage_cpu.py shows that every
checker used here rejects the defect it exists for and asserts the conditions of the inputs.

Everything goes through the C ABI with the guarded buffers of tests/prefilter_gpu_harness.MseTokenSearch.  Cases (d) print one MARGIN
line, cases (e) - (g) one STAGE line each (profiles/mse_stage_margins.json keeps them)."""
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import prefilter_stage1_reference as sr
from tests import token_mse_pq_reference as pqr
from tests import token_mse_prefilter_reference as mpr
from tests import token_mse_stage_reference as ms
from tests import token_prefilter_select_reference as tps
from tests import token_prefilter_stage_reference as tr
from tests.prefilter_gpu_harness import FILL32, MseTokenSearch, set_lo

INF, F = ms.INF, np.float32
OFFSET = 2 ** 33 + 7


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()
    return _ops


def same_bits(a, b):
    """Bit equality of two float32 arrays, any NaN equal to any NaN."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(((sr.f32bits(a) == sr.f32bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def widen(u16, dt):
    return sr.widen16(u16, ms.FMT[dt])


@functools.lru_cache(maxsize=None)
def small_bank(dt, D, seed=3):
    """Any legal small bank: 2048 rows, P = 1."""
    rng = np.random.default_rng(seed + D)
    return mpr.to16(rng.standard_normal((2048, 1, D)).astype(F), dt)


# ------------------------------------------------------------------------------------- a. shared-weight query images and constants
QA = 261


def planted_queries(D, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((QA, D)).astype(F)
    c = ms.weights_shared(rng, D)
    c[::7] = 0.0                                                       # weights with zeros
    t[0] = 0.0                                                         # a zero query
    t[1] *= F(2.0 ** -115)                                             # |tw| near 2^-121: the e >= -126 clamp
    t[2] *= F(2.0 ** -48)                                              # bf16: a scale above 2^30
    t[3] *= F(2.0 ** 90)                                               # bf16: the clamp at 2^-100; A^ overflows to inf
    t[4] *= F(1e25)                                                    # A^ overflows to inf
    t[5] *= F(2.0 ** -73)                                              # fp16: a scale at 2^90
    t[6] *= F(2.0 ** -52)                                              # A^ below 2^-100: A_dn = 0
    t[7] *= F(300.0)
    t[8] = 0.0
    t[8, 1] = 1.5                                                      # one nonzero element
    return c, t


@pytest.mark.parametrize("D", [128, 160])
@pytest.mark.parametrize("lo", [0, 1])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_shared_query_images_and_constants(ops, monkeypatch, dt, lo, D):
    set_lo(monkeypatch, lo)
    c, t = planted_queries(D, 11 + lo)
    xw = small_bank(dt, D)
    s = MseTokenSearch(ops, dt, c, t, xw, 5, "min")
    assert s.guards_ok
    qc = mpr.query_constants(c, t, dt, bool(lo))
    fl, ok = qc["flagged"], ~qc["flagged"]
    assert fl[0] and fl[1] and fl[3] and fl[4] and fl[5] and ok[7] and ok[8] and ok[9:].all() and fl[2] == (dt == "bf16"), np.flatnonzero(fl)
    Q = QA
    assert np.array_equal(s.ws["overflow"] != 0, fl), np.flatnonzero((s.ws["overflow"] != 0) != fl)
    assert np.array_equal(s.redo != 0, fl)
    assert np.array_equal(widen(s.ws["qh"][:Q], dt)[ok], qc["qh"][ok])
    if lo:
        assert np.array_equal(widen(s.ws["ql"][:Q], dt)[ok], qc["ql"][ok])
    assert s.ws["qh"].shape[0] == 512 and (s.ws["qh"][Q:] == 0).all() and (s.ws["ql"][Q:] == 0).all()
    r = ms.check_query_constants(s.ws["qbase"], qc, D, mpr.eps_mse(D, bool(lo), dt), ok)
    assert r is None, r
    assert (ok & (qc["A64"] < 2.0 ** -101)).any() or dt == "bf16"       # (bf16: such a query's scale is outside the window)
    assert np.isnan(s.ws["qpar"][Q:]).all() and not np.isnan(s.ws["qpar"][:Q][ok]).any()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_a_bad_weight_flags_every_query(ops, monkeypatch, dt):
    set_lo(monkeypatch, 0)
    D = 128
    xw = small_bank(dt, D)
    for bad in (-0.25, np.nan, 1025.0):
        c, t = planted_queries(D, 17)
        c[9] = bad
        s = MseTokenSearch(ops, dt, c, t, xw, 5, "min")
        assert s.guards_ok and (s.ws["overflow"] != 0).all() and (s.redo == 1).all(), bad
        assert (s.ws["qbase"][:, 3] != 0).all() and (s.ws["qbase"][:, 0] == 0).all(), bad


# ------------------------------------------------------------------------------------------- b. the first test row and the state
FLOORS = [-0.7, 0.0, np.nan, -INF, INF, -1.0e38, -3.0]


@pytest.mark.parametrize("pq", [False, True], ids=["shared", "perquery"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_first_test_row_and_state(ops, monkeypatch, dt, pq):
    """Fewer images with a finite distance than k: no slice can raise the threshold, so what the search leaves IS the first
    threshold, and the test row every slice republished is the first one's (the same rule on the same tau and qbase)."""
    set_lo(monkeypatch, 1)
    D, Q, k = 128, 40, 8
    rng = np.random.default_rng(5 + pq)
    xw = small_bank(dt, D).reshape(32, 64, D).copy()                   # one direct slice: nothing is staged
    xw[5:, :, 3] = np.nan                                              # five images with a finite distance
    t = rng.standard_normal((Q, D)).astype(F)
    t[7] = 0.0
    t[9] *= F(1e25)
    c = ms.weights_pq(rng, Q, D) if pq else ms.weights_shared(rng, D)
    for floors in (None, np.array([FLOORS[q % len(FLOORS)] for q in range(Q)], F)):
        s = MseTokenSearch(ops, dt, c, t, xw, k, "min", thr0=floors)
        assert s.guards_ok
        tau = ms.first_tau(floors, Q)
        assert same_bits(s.ws["tau"], tau), (s.ws["tau"], tau)
        want, bad = ms.model_mse_qpar(tau, s.ws["qbase"], D, ms.gamma_f32(D))
        assert same_bits(s.ws["qpar"][:Q], want), np.argwhere(sr.f32bits(s.ws["qpar"][:Q]) != sr.f32bits(want))[:4]
        assert np.isnan(s.ws["qpar"][Q:]).all()
        flags = ms.model_mse_flags(s.ws["qbase"], bad, dt)
        assert np.array_equal(s.ws["overflow"] != 0, flags) and np.array_equal(s.redo != 0, flags), (s.redo, flags)
        assert flags[7] and flags[9] and not flags[0]
        if floors is not None:
            assert bad[np.isposinf(floors)].all() and not bad[~np.isposinf(floors)].any()       # a floor of +inf: a defined refusal
        assert (s.ws["cnt"] == 0).all() and (s.rn <= 5).all() and (floors is not None or (s.rn[~flags] == 5).all())


# ------------------------------------------------------------------------------------------------------- c. every dot^, to the bit
PAIR_Q, PAIR_K = 300, 32
PAIRS = [(dt, lo, R, D, pq) for dt in ("f16", "bf16") for lo in (0, 1) for R in (2048, 2092) for D in (128, 160) for pq in (False, True)]
pair_id = lambda a: f"{a[0]}-{'hilo' if a[1] else 'hi'}-R{a[2]}-D{a[3]}-{'perquery' if a[4] else 'shared'}"


@functools.lru_cache(maxsize=4)
def grid_answer(dt, R, D, pq):
    """The contract's top-k on the integer-grid inputs (they do not depend on lo)."""
    g = ms.exact_grid_case(dt, 1, PAIR_Q, R, D, pq)
    return ms.topk_of_keys(ms.keys_of(ms.contract(g["c"], g["t"], g["x"]), 1, "min"), PAIR_K, OFFSET)


@pytest.mark.parametrize("a", PAIRS, ids=pair_id)
def test_every_dot_to_the_bit(ops, monkeypatch, a):
    dt, lo, R, D, pq = a
    set_lo(monkeypatch, lo)
    g = ms.exact_grid_case(dt, lo, PAIR_Q, R, D, pq)
    s = MseTokenSearch(ops, dt, g["c"], g["t"], g["x"].reshape(R, 1, D), PAIR_K, "min", idx_offset=OFFSET)
    assert s.guards_ok and (s.redo == 0).all() and (s.ws["overflow"] == 0).all()
    dots, written = s.dots()
    assert (written == R).all(), (written.min(), written.max())        # every row once, nothing behind the lists
    assert not np.isnan(dots).any()                                    # R slots, R distinct rows
    r = sr.check_dots(dots, g["dot"])
    assert r is None, r
    want_s, want_i = grid_answer(dt, R, D, pq)
    assert np.array_equal(s.out_i, want_i) and same_bits(s.out_s, want_s)


# ------------------------------------------------------------------------------- d. every pair inside the proven bound, the bound sound
def worst_mantissas(dt, n):
    """The n numbers of [1, 2) of the format whose squares round UP by the most, measured on the format itself."""
    bits = 10 if dt == "f16" else 7
    m = (1.0 + np.arange(2 ** bits) * 2.0 ** -bits).astype(F)
    v = m.astype(np.float64) ** 2
    err = (mpr.to16((m * m).astype(F), dt).astype(np.float64) - v) / np.exp2(np.floor(np.log2(v)))
    return m[np.argsort(err)[-n:]]


@functools.lru_cache(maxsize=4)
def ordinary_pairs(dt, R, D, pq):
    rng = np.random.default_rng(R + D + 7 * pq)
    x = ms.scaled_bank(rng, R, 1, D, dt, (-4.5, 1.5) if dt == "f16" else (-3.0, 3.0))       # six decades; fp16: rows of subnormals
    if pq:                                                             # rows of equal elements whose squares round up by half an ulp
        vals = np.concatenate([worst_mantissas(dt, 16) * sc for sc in (0.125, 1.0, 8.0, 16.0)]).astype(F)
        x[100:100 + len(vals), 0, :] = vals[:, None]
        x[100:100 + len(vals):2, 0, ::3] *= -1.0
    t = rng.standard_normal((PAIR_Q, D)).astype(F)
    c = ms.weights_pq(rng, PAIR_Q, D) if pq else ms.weights_shared(rng, D)
    if dt == "f16":
        x[50:53, 0, :] = (2.0 ** -17 * rng.integers(1, 8, (3, D)) * rng.choice([-1.0, 1.0], (3, D))).astype(F)
    flat = np.ascontiguousarray(x.reshape(R, D))
    if dt == "f16":
        assert ((np.abs(flat) > 0) & (np.abs(flat) < 2.0 ** -14)).all(axis=1).any()          # a row made of subnormals
    return c, t, x, flat, ms.contract(c, t, flat)


@pytest.mark.parametrize("a", PAIRS, ids=pair_id)
def test_every_pair_inside_the_bound(ops, monkeypatch, a):
    dt, lo, R, D, pq = a
    set_lo(monkeypatch, lo)
    c, t, x, flat, dist = ordinary_pairs(dt, R, D, pq)
    s = MseTokenSearch(ops, dt, c, t, x, PAIR_K, "min")
    assert s.guards_ok
    dots, written = s.dots()
    qb, rp = s.ws["qbase"], s.rowp[:R]
    ok = ((s.ws["overflow"] == 0) & (s.redo == 0))[:, None] & np.isfinite(rp[:, 1])[None, :]
    assert ok.mean() > 0.5 and not np.isnan(dots[ok]).any()            # every boundable row is listed for every unflagged query
    with np.errstate(all="ignore"):
        tw = ((c if pq else c[None, :]) * t).astype(F)
    r1, m1 = ms.check_pair_bound(dots, ms.real_dot(tw, qb[:, 2], flat, c if pq else None), qb, rp, ok)
    r2, m2 = ms.check_lower_bound(ms.lower_bound(dots, qb, rp), dist, D, ok)
    print("MARGIN", json.dumps(dict(case=pair_id(a), pairs=int(ok.sum()), error_over_bound=round(m1, 5), L_over_rhs=round(m2, 6))))
    assert r1 is None, r1
    assert r2 is None, r2


# ----------------------------------------------------------------------------------------- e - g. the lists, image by image
def run(ops, case, thr0, flags=None):
    return MseTokenSearch(ops, case["dt"], case["c"], case["t"], case["xw"], case["k"], case["combine"], case["top_t"], flags, thr0, OFFSET)


def record(name, case, must_in, must_out, listed, scope, **more):
    pairs = np.repeat(scope[None, :], case["Q"], axis=0)
    line = dict(case=name, P=case["P"], combine=case["combine"], dt=case["dt"], lo="hi+lo" if case["lo"] else "hi", pq=case["pq"], N=case["N"],
                k=case["k"], **tr.counts(must_in & pairs, must_out & pairs, listed, pairs), **more)
    print("STAGE", json.dumps(line))


def slice_sandwich(s, case, sched, taus, flags=None):
    """The LAST slice's complete candidate sets against the threshold in force during it, with the device's own constants; what is
    left of every earlier slice: nothing that was must-be-out against that slice's own threshold; nothing outside the selection or
    outside [0, N) anywhere.  -> (must_in, must_out, listed) of the last slice."""
    n = len(sched["slices"])
    last = sched["images"][-1]
    assert (s.ws["overflow"] == 0).all() and (s.ws["cnt"] <= s.cap).all()
    must_in, must_out = ms.case_classes(case, taus[n - 1], s.ws["qbase"], s.rowp, flags)
    must_in, must_out = must_in & last[None, :], must_out & last[None, :]
    lists = [s.candidates(q, last) for q in range(s.Q)]
    r = sr.check_sandwich(lists, must_in, must_out, allowed=flags)
    assert r is None, r
    for q in range(s.Q):
        row = s.ws["cand_i"][q]
        every = row[row != FILL32].astype(np.int64)
        assert len(every) == 0 or (every.min() >= 0 and every.max() < s.N), q
        assert flags is None or flags[every].all(), (q, "a deselected image is listed")
    for i in range(n - 1):
        _, mo = ms.case_classes(case, taus[i], s.ws["qbase"], s.rowp, flags)
        for q in range(s.Q):
            rem = s.candidates(q, sched["images"][i])
            assert not mo[q][rem].any(), (i, q, "a remnant of an earlier slice was must-be-out against that slice's threshold")
    return must_in, must_out, sum(len(l) for l in lists)


def published_state(s, case, taus, flags=None):
    """What token_rescore_body<DIST> leaves: tau, the test row, the running list and its length, cnt, the outputs, the flags."""
    Q, k, D = s.Q, s.k, case["D"]
    keys = case["keys"] if flags is None else np.where(flags[None, :], case["keys"], F(-INF)).astype(F)
    assert s.guards_ok
    assert same_bits(s.ws["tau"], taus[-1]), (s.ws["tau"], taus[-1])
    want, bad = ms.model_mse_qpar(s.ws["tau"], s.ws["qbase"], D, ms.gamma_f32(D))
    assert same_bits(s.ws["qpar"][:Q], want), np.argwhere(sr.f32bits(s.ws["qpar"][:Q]) != sr.f32bits(want))[:4]
    assert np.isnan(s.ws["qpar"][Q:]).all() and not bad.any()
    assert (s.ws["cnt"] == 0).all()
    assert np.array_equal(s.redo != 0, s.ws["overflow"] != 0) and (s.redo == 0).all(), s.redo
    finite = (keys > -INF).sum(axis=1)
    ref_s, ref_i = ms.topk_of_keys(keys, k, OFFSET)
    for q in range(Q):
        assert s.rn[q] == min(k, finite[q]), (q, s.rn[q], finite[q])
        got = s.list[q, :s.rn[q]].tolist()
        assert len(set(got)) == len(got) and set(got) == tr.expected_list(keys[q], k), q
    assert np.array_equal(s.out_i, ref_i), np.argwhere(s.out_i != ref_i)[:4]
    assert same_bits(s.out_s, ref_s)


def probes(s, case, images, flags=None):
    have = np.zeros(case["N"], bool)
    have[s.candidates(ms.QSTAR, images)] = True
    r = ms.check_probes(case, have | ~images, flags)
    assert r is None, r
    r = ms.check_probes(case, have & images, flags)
    assert r is None, r
    assert (case["kind"] == 1).any() and (case["kind"] == 2).any()


@pytest.mark.parametrize("a", ms.SANDWICH, ids=lambda a: f"P{a[0]}-{a[1]}-{a[2]}-{'hilo' if a[3] else 'hi'}-N{a[4]}")
def test_sandwich_at_a_known_threshold(ops, monkeypatch, a):
    """The floor is the k-th best key over the first half of the images.  From P = 4 on the plan is ONE direct slice (with the tail
    tile of the ragged banks); at P = 1 the same shape and k give a direct slice of three tiles and two staged ones, and the last
    slice's lists are held to the threshold in force during it, the remnants of the earlier ones to theirs."""
    set_lo(monkeypatch, a[3])
    case = ms.sandwich_case(*a)
    sched = case["sched"]
    assert (len(sched["slices"]) == 1) == (a[0] > 1), sched["slices"]
    s = run(ops, case, case["thr0"])
    taus = ms.slice_taus(case["keys"], case["thr0"], case["k"], sched["images"])
    must_in, must_out, listed = slice_sandwich(s, case, sched, taus)
    record("sandwich", case, must_in, must_out, listed, sched["images"][-1], slices=len(sched["slices"]))
    probes(s, case, sched["images"][-1])
    published_state(s, case, taus)


@pytest.mark.parametrize("a", ms.STAGED, ids=lambda a: f"{a[0]}-{a[1]}-{'hilo' if a[2] else 'hi'}-N{a[3]}-{'perquery' if a[4] else 'shared'}")
def test_staged_slices_and_published_state(ops, monkeypatch, a):
    from sky_embeddings_amd import _lib
    combine, dt, lo, N, pq = a
    set_lo(monkeypatch, lo)
    case = ms.staged_case(*a)
    P, k, D, Q = case["P"], case["k"], case["D"], case["Q"]
    thr0 = case["thr0"] if combine == "min" else None                  # with a floor ('min') and without ('max')
    Np, Ds = (-(-N * P // 256) * 256 // P, 2 * D) if pq else (N, D)
    plan = ops.prefilter_plan(_lib.PF_TOKENS, _lib.PF_BANK_BF16 if dt == "bf16" else _lib.PF_BANK_F16, Q, Np, Ds, k, P,
                              ops.COMBINE_CODES["max" if combine == "min" else "min"], thr0=thr0 is not None, lo=lo)
    got = [(sl.mode, sl.t0, sl.t1, bool(sl.tail)) for sl in plan.slice[:plan.n_slices]]
    T = Np * P // 256
    assert got == [(1, 0, 8, False), (2, 8, 16, False), (2, 16, T, bool(Np * P % 256))], got
    assert [(t0, t1) for t0, t1, _, _ in case["sched"]["slices"]] == [(0, 8), (8, 16), (16, T)]
    s = run(ops, case, thr0)
    taus = ms.slice_taus(case["keys"], thr0, k, case["sched"]["images"])
    must_in, must_out, listed = slice_sandwich(s, case, case["sched"], taus)
    record("staged", case, must_in, must_out, listed, case["sched"]["images"][-1], slices=3)
    published_state(s, case, taus)
    g, dst = case["tie"]                                               # a duplicated image: listed, re-scored, the lower image first
    assert s.out_i[0, 0] == g + OFFSET and s.out_i[0, 1] == dst + OFFSET and dst in s.candidates(0, case["sched"]["images"][-1])


@pytest.mark.parametrize("a", ms.TOPT, ids=lambda a: f"top{a[0]}-{a[1]}-{'hilo' if a[2] else 'hi'}")
def test_counting_fold_under_top_t(ops, monkeypatch, a):
    set_lo(monkeypatch, a[2])
    case = ms.topt_case(*a)
    sched = case["sched"]
    s = run(ops, case, case["thr0"])
    taus = ms.slice_taus(case["keys"], case["thr0"], case["k"], sched["images"])
    must_in, must_out, listed = slice_sandwich(s, case, sched, taus)
    record("top_t", case, must_in, must_out, listed, sched["images"][-1], top_t=a[0])
    probes(s, case, sched["images"][-1])
    published_state(s, case, taus)


@pytest.mark.parametrize("a", ms.SELECTED, ids=lambda a: f"{a[0]}-{a[1]}-{'hilo' if a[2] else 'hi'}")
def test_lists_under_a_selection(ops, monkeypatch, a):
    set_lo(monkeypatch, a[2])
    case = ms.selected_case(*a)
    f = ms.selection_of(case)
    tiles, cum, last_live, de, sched = ms.selected_schedule(case, f)
    thr0 = ms.selected_floor(case, f)
    s = run(ops, case, thr0, f)
    assert s.tiles.tolist() == tiles.tolist() and s.cum == cum.tolist() and s.last_live == last_live and s.direct_end == de
    N, P, D = case["N"], case["P"], case["D"]
    rows = np.repeat(f, P)
    assert np.array_equal(sr.f32bits(s.rowp[:N * P][~rows]), np.tile(sr.f32bits(tps.SENTINEL), ((~rows).sum(), 1)))
    B64, _, nx64, ub = mpr.row_constants(case["c"], case["flat"], case["dt"])
    rp, slack = s.rowp[:N * P][rows].astype(np.float64), 2.0 * D * 2.0 ** -22
    assert not ub.any() and (rp[:, 0] <= B64[rows]).all() and (rp[:, 0] >= B64[rows] * (1.0 - slack)).all()
    assert (rp[:, 1] >= nx64[rows]).all() and (rp[:, 1] <= nx64[rows] * (1.0 + slack)).all() and (rp[:, 2] == 1.0).all()
    keys = np.where(f[None, :], case["keys"], F(-INF)).astype(F)
    taus = ms.slice_taus(keys, thr0, case["k"], sched["images"])
    must_in, must_out, listed = slice_sandwich(s, case, sched, taus, f)
    record("selected", case, must_in, must_out, listed, sched["images"][-1] & f, slices=len(sched["slices"]), selected=int(f.sum()))
    published_state(s, case, taus, f)
    # garbage, NaN included, in the deselected images changes no bit
    dirty = dict(case)
    dirty["xw"] = case["xw"].copy()
    dirty["xw"][~f] = np.where(np.arange(D) % 3 == 0, np.nan, 3.0e4).astype(F)
    s2 = run(ops, dirty, thr0, f)
    assert s2.guards_ok and np.array_equal(sr.f32bits(s2.rowp), sr.f32bits(s.rowp))
    for name in ("tau", "qpar", "qbase", "nsel", "overflow"):
        assert np.array_equal(s2.ws[name].view(np.uint32), s.ws[name].view(np.uint32)), name
    assert np.array_equal(s2.out_i, s.out_i) and np.array_equal(sr.f32bits(s2.out_s), sr.f32bits(s.out_s))
    for q in range(s.Q):
        assert sorted(s2.list[q, :s.rn[q]].tolist()) == sorted(s.list[q, :s.rn[q]].tolist())
        last = sched["images"][-1]                                     # (what is left of earlier slices depends on the order of the appends)
        assert sorted(s2.candidates(q, last).tolist()) == sorted(s.candidates(q, last).tolist()), q
