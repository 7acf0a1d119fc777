"""CPU: the checkers of tests/token_mse_stage_reference.py reject the defects they exist for -- each is run on a MODEL of the device's
output (the constants of the statements, dot^ = the operands' product rounded to fp32, the test of the instruction, the fold) with
one planted slip -- and the conditions of the inputs of tests/test_token_mse_stage_gpu.py, asserted on the reference alone: enough
must-in images, a small undecided share, lists and staging regions that cannot fill, probes in the classes the cases need."""
import numpy as np
import pytest

from tests import prefilter_stage1_reference as sr
from tests import token_mse_pq_reference as pqr
from tests import token_mse_prefilter_reference as mpr
from tests import token_mse_stage_reference as ms
from tests import token_prefilter_stage_reference as tr

F, INF = np.float32, ms.INF


def model_lists(case, tau, images, qbase=None, rowp=None, **fold):
    """The candidate lists a correct device leaves for the images in `images` at key thresholds tau: the instruction's test on the
    model's constants, folded."""
    mc = case["model"]
    qbase = mc["qbase"] if qbase is None else qbase
    rowp = mc["rowp"] if rowp is None else rowp
    qpar, _ = ms.model_mse_qpar(tau, qbase, case["D"], ms.gamma_f32(case["D"]))
    with np.errstate(all="ignore"):
        passed = ms.pair_test_value(mc["dot16"].astype(F), qpar, rowp) >= 0
    cand = ms.fold_pass_bits(passed, case["P"], case["combine"], case["top_t"], **fold) & images[None, :]
    return cand, tr.lists_of(cand)


def last_slice(case, thr0):
    sched = case["sched"]
    taus = ms.slice_taus(case["keys"], thr0, case["k"], sched["images"])
    return sched, taus, taus[len(sched["slices"]) - 1], sched["images"][-1]


# ------------------------------------------------------------------------------------------------------- the model of the test row
def test_one_rounding():
    a = float(F(1.0 + 2.0 ** -12))
    assert ms._fma32(a, a, -(1.0 + 2.0 ** -11)) == 2.0 ** -24           # two roundings give 0
    assert ms.round_f32(2 ** 24 + 1) == 2.0 ** 24 and ms.round_f32(2 ** 24 + 3) == 2.0 ** 24 + 4
    assert ms.round_f32(2.0 ** -149 * 0.5) == 0.0 and ms.round_f32(2.0 ** -149 * 1.5) == 2.0 ** -148
    assert ms.round_f32(2.0 ** 128) == INF and np.isnan(ms._fma32(INF, 2.0 ** -20, -INF))


def test_the_test_row_by_hand():
    """One row per clamp, every operation exact: D = 128, gamma = 2^-20, qbase = {A, 2^-10, 2^-3, 0}."""
    D, g32 = 128, F(2.0 ** -20)
    open38 = float(F(3.0e38))
    x = -(2.0 ** -4 - 2.0 ** -23)
    y = 2.0 ** -10 * (1.0 + 2.0 ** -19)
    row = lambda tau, A=256 * 2.0 ** -20, z=2.0 ** -3: ms.model_mse_qpar(np.array([tau], F), np.array([[A, 2.0 ** -10, z, 0.0]], F), D, g32)
    # theta = 2: T = 256 (1 + 2^-20) (+ 2^-126, lost), T - A = 256, h = 2^-4 (the halving), g = 16 (1 + 2^-19)
    qp, bad = row(-2.0)
    assert qp[0].tolist() == [x, y, 16.0 + 2.0 ** -15, 0.0] and not bad[0]
    # no threshold, by -inf, by a key at -3e38 and by a key whose D theta overflows: theta or T clamp to 3e38
    want_g = float(F(F(F(open38) * F(2.0 ** -4)) * F(1.0 + 2.0 ** -19)))
    for tau in (-INF, -open38, -1.0e38):
        qp, bad = row(tau, A=1.0)
        assert qp[0].tolist() == [x, y, want_g, 0.0] and not bad[0], tau
    # the clamp of g: a scale of 2^100
    qp, bad = row(-INF, A=1.0, z=2.0 ** 100)
    assert qp[0, 2] == F(3.0e38) and qp[0, 0] == -F(2.0 ** 99 * (1 - 2.0 ** -19)) and not bad[0]
    # g below fp32's range: a threshold far below A_dn times a large scale (-inf, and -inf + |-inf| 2^-19 is not a number)
    qp, bad = row(-1.0, A=2.0 ** 100, z=2.0 ** 60)
    assert bad[0] and np.isnan(qp[0, 2])
    # a floor of +inf: theta = -inf, T and g are not numbers: refused
    qp, bad = row(INF)
    assert bad[0] and np.isnan(qp[0, 2]) and qp[0, 0] == F(x)
    # a key threshold of 0: T = 2^-126
    qp, bad = row(0.0, A=0.0)
    assert qp[0, 2] == F(2.0 ** -4 * 2.0 ** -126 * (1 + 2.0 ** -19)) and not bad[0]
    flags = ms.model_mse_flags(np.array([[1, 2.0 ** -10, 2.0 ** -3, 0], [1, 2.0 ** -10, 2.0 ** -3, 1], [1, 0, 1, 0], [1, 2.0 ** 60, 1, 0],
                                         [1, 1, 2.0 ** 90, 0], [1, 1, 2.0 ** 30, 0], [1, 1, 2.0 ** -100, 0], [1, np.nan, 1, 0]], F), np.zeros(8, bool), "f16")
    assert flags.tolist() == [False, True, True, True, True, False, False, True]
    flags = ms.model_mse_flags(np.array([[1, 1, 2.0 ** 29, 0], [1, 1, 2.0 ** 30, 0], [1, 1, 2.0 ** -100, 0], [1, 1, 2.0 ** -99, 0]], F),
                               np.array([False, False, False, True]), "bf16")
    assert flags.tolist() == [False, True, True, True]


def test_h_without_the_halving_is_caught():
    case = ms.sandwich_case(*ms.SANDWICH[2])
    _, taus, tau, last = last_slice(case, case["thr0"])
    mc = case["model"]
    twice = mc["qbase"].copy()
    twice[:, 2] *= F(2.0)                                              # h = qb.z instead of qb.z / 2 in the test row
    qpar, _ = ms.model_mse_qpar(tau, twice, case["D"], ms.gamma_f32(case["D"]))
    good, _ = ms.model_mse_qpar(tau, mc["qbase"], case["D"], ms.gamma_f32(case["D"]))
    assert not np.array_equal(sr.f32bits(qpar), sr.f32bits(good))      # the bit comparison of the published row
    with np.errstate(all="ignore"):
        passed = ms.pair_test_value(mc["dot16"].astype(F), qpar, mc["rowp"]) >= 0
    lists = tr.lists_of(ms.fold_pass_bits(passed, case["P"], case["combine"]) & last[None, :])
    must_in, must_out = ms.case_classes(case, tau)
    assert sr.check_sandwich(lists, must_in & last[None, :], must_out & last[None, :]) is not None


# --------------------------------------------------------------------------------------------------------------- the constants
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("pq", [False, True])
def test_query_constant_checker(dt, pq):
    rng = np.random.default_rng(3)
    D, Q, lo = 160, 50, True
    t = rng.standard_normal((Q, D)).astype(F)
    c = ms.weights_pq(rng, Q, D) if pq else ms.weights_shared(rng, D)
    x = mpr.to16(rng.standard_normal((300, D)).astype(F), dt)
    mc = ms.model_constants(c, t, x, dt, lo)
    qc, ok = mc["qc"], ~mc["qc"]["flagged"]
    eps = pqr.eps_pq(D, lo, dt) if pq else mpr.eps_mse(D, lo, dt)
    Ds = 2 * D if pq else None
    assert ok.all() and ms.check_query_constants(mc["qbase"], qc, D, eps, ok, Ds) is None
    # eps without its 2^-22 (the term that pays for fl(c o t))
    short = mc["qbase"].copy()
    short[:, 1] = (short[:, 1].astype(np.float64) * (eps - 2.0 ** -22) / eps).astype(F)
    if not (pq and dt == "bf16"):      # (there eps_pq is 2^-8 and more: 2^-22 of it is less than the slack the statement grants above)
        assert "half-width is not a bound" in ms.check_query_constants(short, qc, D, eps, ok, Ds)
    # A raised instead of lowered
    raised = mc["qbase"].copy()
    raised[:, 0] = (qc["A64"] * (1.0 + D * 2.0 ** -22)).astype(F)
    assert "not a lower bound" in ms.check_query_constants(raised, qc, D, eps, ok, Ds)
    # a wrong scale
    scaled = mc["qbase"].copy()
    scaled[3, 2] *= F(2.0)
    assert ms.check_query_constants(scaled, qc, D, eps, ok, Ds) is not None


def test_gamma_zero_is_caught_on_a_chain_that_rounds_down():
    """A pair whose contract value lost 2^-24 at every one of its n roundings, dist^ = dist (1 - 2^-24)^n, under the tightest sound
    bound L = D dist: inside the statement with gamma, outside with gamma = 0."""
    D = 128
    n = mpr.chain_roundings(D)
    real = np.array([[0.731, 12.5, 3.0e-7]])
    dist32 = (real * (1.0 - 2.0 ** -24) ** n).astype(F)
    dist32 = np.where(dist32.astype(np.float64) > real * (1.0 - 2.0 ** -24) ** n, np.nextafter(dist32, F(0)), dist32)
    ok = np.ones((1, 3), bool)
    assert ms.check_lower_bound(real * D, dist32, D, ok)[0] is None
    assert ms.check_lower_bound(real * D, dist32, D, ok, gamma=0.0)[0] is not None


def test_pair_bound_checker():
    g = ms.exact_grid_case("f16", 1, 300, 2048, 128, False)
    mc = ms.model_constants(g["c"], g["t"], g["x"], "f16", True)
    ok = np.ones(g["dot"].shape, bool)
    assert np.array_equal(mc["dot16"].astype(F), g["dot"])             # the grid's dot^ IS the operands' product
    real = ms.real_dot(mc["qc"]["tw"], mc["qc"]["s"], g["x"])
    assert ms.check_pair_bound(g["dot"], real, mc["qbase"], mc["rowp"], ok)[0] is None
    hi_only = ms.exact_grid_case("f16", 0, 300, 2048, 128, False)["dot"]              # the lo pass left out: outside the hi + lo bound
    assert ms.check_pair_bound(hi_only, real, mc["qbase"], mc["rowp"], ok)[0] is not None
    assert sr.check_dots(hi_only, g["dot"]) is not None


# ------------------------------------------------------------------------------------------------------- the fold and the lists
@pytest.mark.parametrize("a", [ms.SANDWICH[2], ms.SANDWICH[5], ms.SANDWICH[7]], ids=str)
def test_fold_defects_are_caught(a):
    case = ms.sandwich_case(*a)
    _, taus, tau, last = last_slice(case, case["thr0"])
    must_in, must_out = ms.case_classes(case, tau)
    mi, mo = must_in & last[None, :], must_out & last[None, :]
    cand, lists = model_lists(case, tau, last)
    assert sr.check_sandwich(lists, mi, mo) is None and ms.check_probes(case, cand[ms.QSTAR] | ~last) is None
    assert ms.check_probes(case, cand[ms.QSTAR] & last) is None
    # OR and AND swapped
    wrong, wl = model_lists(case, tau, last, wrong=True)
    assert sr.check_sandwich(wl, mi, mo) is not None
    assert ms.check_probes(case, wrong[ms.QSTAR] | ~last) is not None or ms.check_probes(case, wrong[ms.QSTAR] & last) is not None
    # one token left out of the fold: the probe that token alone decides tells ('min': the 'in' probe of that position is lost;
    # 'max': its 'out' probe is listed)
    telling = 1 if case["combine"] == "min" else 2
    for p in sorted(set(case["probe_p"][case["kind"] == telling].tolist()))[:8]:
        skipped, _ = model_lists(case, tau, last, skip=p)
        r = ms.check_probes(case, skipped[ms.QSTAR] | ~last) or ms.check_probes(case, skipped[ms.QSTAR] & last)
        assert r is not None, p
    # a duplicate in a list
    twice = [np.concatenate([l, l[:1]]) for l in lists]
    assert "listed twice" in sr.check_sandwich(twice, mi, mo)


@pytest.mark.parametrize("a", ms.TOPT, ids=str)
def test_a_counting_fold_off_by_one_is_caught(a):
    case = ms.topt_case(*a)
    _, taus, tau, last = last_slice(case, case["thr0"])
    must_in, must_out = ms.case_classes(case, tau)
    cand, lists = model_lists(case, tau, last)
    assert sr.check_sandwich(lists, must_in & last[None, :], must_out & last[None, :]) is None
    assert ms.check_probes(case, cand[ms.QSTAR] | ~last) is None and ms.check_probes(case, cand[ms.QSTAR] & last) is None
    if a[0] == case["P"]:
        return                                                         # top_t = P is the plain AND fold
    for off in (1, -1):
        c2, l2 = model_lists(case, tau, last, off_by=off)
        r = ms.check_probes(case, c2[ms.QSTAR] | ~last) or ms.check_probes(case, c2[ms.QSTAR] & last)
        assert r is not None and sr.check_sandwich(l2, must_in & last[None, :], must_out & last[None, :]) is not None, off


def test_a_stale_threshold_is_caught():
    case = ms.staged_case(*ms.STAGED[1])                               # no floor: every slice raises the thresholds
    sched, taus, tau, last = last_slice(case, None)
    assert len(taus) == 4 and (taus[-1] > taus[-2]).any()              # the last slice moves thresholds
    assert not np.array_equal(sr.f32bits(taus[-1]), sr.f32bits(taus[-2]))                    # what the bit comparison of tau sees
    must_in, must_out = ms.case_classes(case, tau)
    _, stale = model_lists(case, taus[0], last)                        # the last slice run under the first threshold
    assert sr.check_sandwich(stale, must_in & last[None, :], must_out & last[None, :]) is not None


# ----------------------------------------------------------------------------------------------------- conditions of the inputs
def conditions(case, thr0, flags=None, sched=None, probes=True):
    sched = case["sched"] if sched is None else sched
    keys = case["keys"] if flags is None else np.where(flags[None, :], case["keys"], F(-INF)).astype(F)
    taus = ms.slice_taus(keys, thr0, case["k"], sched["images"])
    n = len(sched["slices"])
    last = sched["images"][-1] & (True if flags is None else flags)
    assert not case["model"]["qc"]["flagged"].any() and not case["model"]["ub"].any()
    must_in, must_out = ms.case_classes(case, taus[n - 1], flags=flags)
    assert (must_in.sum(axis=1) >= case["k"]).all()                    # at least k must-in images per query
    assert ms.undecided_share(must_in, must_out, last).max() <= 0.02
    if probes:
        assert ms.check_probes(case, must_in[ms.QSTAR] | ~last, flags) is None       # every 'in' probe must-in
        assert ms.check_probes(case, ~must_out[ms.QSTAR] & last, flags) is None      # every 'out' probe must-out
        pos = set(case["probe_p"][case["kind"] == 1].tolist()), set(case["probe_p"][case["kind"] == 2].tolist())
        if 4 * case["P"] <= case["N"] // 2:
            assert pos[0] == pos[1] == set(range(case["P"]))           # every token position, both kinds
    # no list and no staging region can fill: the model's candidates of every slice at the threshold in force during it
    scope = np.ones(case["N"], bool) if flags is None else flags
    qt = sr.qtile(case["lo"])
    for i, (t0, t1, mode, _) in enumerate(sched["slices"]):
        cand, _ = model_lists(case, taus[i], sched["images"][i] & scope)
        assert cand.sum(axis=1).max() <= sr.cap_of(case["k"]) // 2
        if mode == "staged":
            # (the model's count: a device may also list the undecided pairs, at most 2 % -- a quarter of headroom covers them)
            assert max(cand[q0:q0 + qt].sum() for q0 in range(0, case["Q"], qt)) <= sr.SCAP * 3 // 4


@pytest.mark.parametrize("a", ms.SANDWICH, ids=str)
def test_conditions_of_the_sandwich_cases(a):
    case = ms.sandwich_case(*a)
    conditions(case, case["thr0"])


@pytest.mark.parametrize("a", ms.STAGED, ids=str)
def test_conditions_of_the_staged_cases(a):
    case = ms.staged_case(*a)
    conditions(case, case["thr0"] if a[0] == "min" else None, probes=False)
    g, dst = case["tie"]
    assert g < dst and np.array_equal(case["xw"][g], case["xw"][dst]) and case["keys"][0, g] == case["keys"][0].max()


@pytest.mark.parametrize("a", ms.TOPT, ids=str)
def test_conditions_of_the_top_t_cases(a):
    case = ms.topt_case(*a)
    conditions(case, case["thr0"])


@pytest.mark.parametrize("a", ms.SELECTED, ids=str)
def test_conditions_of_the_selected_cases(a):
    case = ms.selected_case(*a)
    f = ms.selection_of(case)
    tiles, cum, last_live, de, sched = ms.selected_schedule(case, f)
    assert len(sched["slices"]) == 3 and 2 not in tiles.tolist() and 0.4 < f.mean() < 0.6
    conditions(case, ms.selected_floor(case, f), f, sched, probes=False)


@pytest.mark.parametrize("pq", [False, True])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_conditions_of_the_take_all_cases(dt, pq):
    """One direct slice without a floor: every row is listed, within cap; no query flagged, no row unboundable on the grid."""
    for R in (2048, 2092):
        sched = ms.schedule_of(R, 1, 32, pq)
        assert len(sched["slices"]) == 1 and R <= sr.cap_of(32)
        for D in (128, 160):
            g = ms.exact_grid_case(dt, 1, 300, R, D, pq)
            mc = ms.model_constants(g["c"], g["t"], g["x"], dt, True)
            assert not mc["qc"]["flagged"].any() and not mc["ub"].any()
            assert np.array_equal(mc["dot16"].astype(F), g["dot"])     # the grid's one admissible value is the operands' product
            qpar, bad = ms.model_mse_qpar(np.full(300, -INF, F), mc["qbase"], D, ms.gamma_f32(D))
            assert not bad.any() and (ms.pair_test_value(g["dot"], qpar, mc["rowp"]) >= 0).all()
