"""CPU: the statements of tests/token_prefilter_stage_reference.py against hand-derived cases and brute force, the condition of
the planted inputs for every parameter set of tests/test_token_prefilter_stage_gpu.py (each planted image in its class, no list and
no staging region full -- from the reference alone), and the planted defects: a fold that ORs under 'min', ANDs under 'max' or
leaves one token out is rejected by the very check the GPU file applies to the device's lists."""
import numpy as np
import pytest

from tests import prefilter_stage1_reference as sr
from tests import token_prefilter_reference as tpr
from tests import token_prefilter_select_reference as tps
from tests import token_prefilter_stage_reference as tr

INF = tr.INF
D, S = "direct", "staged"

# (N, P, k, n_live, direct_sel, last_live) -> (T, direct_end, slices); ends = direct_end, T // 32, T // 8, T // 2, T
SCHEDULES = [
    # one slice: 96 * 24 rows = 9 tiles reach all 8
    ((2048, 1, 24, None, None, 0), (8, 8, [(0, 8, D, False)])),
    # exactly two: ceil(96 * 14 / 256) = 6 of 10 tiles; 10 // 32, 10 // 8 and 10 // 2 lie at or below 6
    ((2560, 1, 14, None, None, 0), (10, 6, [(0, 6, D, False), (6, 10, S, False)])),
    # all five: 1, 2, 8, 32, 64
    ((16384, 1, 1, None, None, 0), (64, 1, [(0, 1, D, False), (1, 2, S, False), (2, 8, S, False), (8, 32, S, False), (32, 64, S, False)])),
    # the T // 128 rule lifts the first end from 1 to 4
    ((131072, 1, 1, None, None, 0), (512, 4, [(0, 4, D, False), (4, 16, S, False), (16, 64, S, False), (64, 256, S, False), (256, 512, S, False)])),
    # a tail: 2309 images of 4 tokens = 36 tiles and 20 rows; 96 * 4 rows = 2 tiles; 36 // 32 = 1 is dropped
    ((2309, 4, 1, None, None, 0), (36, 2, [(0, 2, D, False), (2, 4, S, False), (4, 18, S, False), (18, 36, S, True)])),
    # a selection, 10 live tiles, the tail tile among them: 9 positions for the slices
    ((2309, 4, 1, 10, 3, 1), (9, 3, [(0, 3, D, False), (3, 4, S, False), (4, 9, S, True)])),
    # the same list without the tail tile
    ((2309, 4, 1, 10, 3, 0), (10, 3, [(0, 3, D, False), (3, 5, S, False), (5, 10, S, False)])),
    # the caller's first end beyond the whole live tiles: clipped, one slice with the tail
    ((2309, 4, 1, 3, 3, 1), (2, 2, [(0, 2, D, True)])),
    # P = 64, k = 6: ceil(96 * 6 * 64 / 256) = 144 tiles reach all 133
    ((532, 64, 6, None, None, 0), (133, 133, [(0, 133, D, False)])),
]


@pytest.mark.parametrize("args,want", SCHEDULES, ids=[str(a) for a, _ in SCHEDULES])
def test_token_schedule_table(args, want):
    N, P, k, n_live, direct_sel, last_live = args
    got = tr.token_schedule(N, P, k, n_live, direct_sel, last_live)
    assert (got["T"], got["direct_end"], got["slices"]) == want
    assert got["ends"] == [want[1], want[0] // 32, want[0] // 8, want[0] // 2, want[0]]


def test_token_schedule_images_and_the_older_restatements():
    """The slices' image ranges partition the images; the tail's ride with the last slice; and the row ranges agree with
    tests/token_prefilter_reference.slices (and, under a selection, with token_prefilter_select_reference.slices)."""
    rng = np.random.default_rng(3)
    for N, P, k in [(2309, 4, 1), (2048, 1, 24), (16384, 1, 1), (1349, 16, 1), (40, 64, 2), (5000, 2, 7)]:
        s = tr.token_schedule(N, P, k)
        total = np.sum(s["images"], axis=0)
        assert (total == 1).all()
        old = tpr.slices(N * P, P, k)
        assert [(a * 256, N * P if tail or b == s["T"] else b * 256, m) for a, b, m, tail in s["slices"]] == old
        for (a, b, m, tail), im in zip(s["slices"], s["images"]):
            want = np.zeros(N, bool)
            want[a * 256 // P:(N if tail or b * 256 >= N * P else b * 256 // P)] = True
            assert np.array_equal(im, want)
        f = rng.random(N) < 0.3
        f[:256 // P] = False
        _, tiles, cum, last = tps.prepare(np.zeros((-(-N * P // 256) * 256, 4), np.float32), f, P)
        de = tps.direct_end(cum, len(tiles), k)
        s = tr.token_schedule(N, P, k, len(tiles), de, last, tiles)
        assert [(a, len(tiles) if b == s["T"] else b, m) for a, b, m, _ in s["slices"]] == tps.slices(tiles, cum, last, N * P, k)
        seen = np.sum(s["images"], axis=0)
        assert (seen <= 1).all() and (seen[f] == 1).all()           # every selected image in exactly one slice


@pytest.mark.parametrize("P", tr.PS)
def test_image_sandwich_against_brute_force(P):
    rng = np.random.default_rng(P)
    Q, N = 3, 40
    state = rng.integers(0, 3, size=(Q, N * P))                     # 0 don't-care (or given up on), 1 must-in, 2 must-out
    state[0, :P] = 1
    state[0, P:2 * P] = 2
    state[1, :P] = 0
    mi, mo = state == 1, state == 2
    for combine in ("min", "max"):
        gi, go = tr.image_sandwich(mi, mo, P, combine)
        for q in range(Q):
            for i in range(N):
                rows = state[q, i * P:(i + 1) * P].tolist()
                if combine == "min":
                    wi, wo = all(r == 1 for r in rows), any(r == 2 for r in rows)
                else:
                    wi, wo = any(r == 1 for r in rows), all(r == 2 for r in rows)
                assert (gi[q, i], go[q, i]) == (wi, wo), (combine, q, i, rows)
        assert gi[0, 0] and go[0, 1] and not gi[1, 0] and not go[1, 0]


def no_overflow(c, flags=None, sched=None, thr0="case"):
    """The condition of every GPU case, from the reference alone: per slice and query the images that may be listed (must-in and
    don't-care) fit the list, and per staged (query tile x bank tile) item the staging region's SCAP slots."""
    sched = c["sched"] if sched is None else sched
    thr0 = c["thr0"] if isinstance(thr0, str) else thr0
    combined = c["combined"] if flags is None else np.where(flags[None, :], c["combined"], np.float32(-INF))
    taus = tr.slice_taus(combined, thr0, c["k"], sched["images"])
    cap = sr.cap_of(c["k"])
    worst = 0
    for i, ((t0, t1, mode, tail), im) in enumerate(zip(sched["slices"], sched["images"])):
        _, must_out = tr.image_classes(c, taus[i], flags)
        may = ~must_out & im[None, :] & (np.ones(c["N"], bool) if flags is None else flags)[None, :]
        assert may.sum(axis=1).max() <= cap, (i, int(may.sum(axis=1).max()))
        worst = max(worst, int(may.sum(axis=1).max()))
        if mode == S:
            ipt = c["ipt"]
            per_tile = may[:, :c["T"] * ipt].reshape(c["Q"], c["T"], ipt).sum(axis=(0, 2))     # Q <= 128: one query tile
            assert c["Q"] <= 128 and per_tile.max() <= tr.SCAP, (i, int(per_tile.max()))
    return worst


@pytest.mark.parametrize("args", tr.SINGLE, ids=str)
def test_planted_single_slice_cases_and_the_wrong_folds(args):
    """planted_case asserts its own condition; then the mutants: ideal row bits (a row passes iff it is not must-be-out) folded
    wrongly give lists that check_sandwich rejects -- for the swapped operation and for EVERY token left out."""
    P, combine = args[:2]
    c = tr.single_case(*args)
    assert len(c["sched"]["slices"]) == 1 and c["sched"]["tail_live"] == args[4] and (c["N"] * P % 256 != 0) == args[4]
    no_overflow(c)
    tau = c["thr0"]
    mi_rows, mo_rows = sr.sandwich(tau, c["score"], c["hw"], c["rows"])
    must_in, must_out = tr.image_classes(c, tau)
    ideal = ~mo_rows
    assert sr.check_sandwich(tr.lists_of(tr.fold_pass_bits(ideal, P, combine)), must_in, must_out) is None
    if P > 1:
        r = sr.check_sandwich(tr.lists_of(tr.fold_pass_bits(ideal, P, combine, wrong="swap")), must_in, must_out)
        assert r is not None and (("more than the interval below" in r) if combine == "min" else ("not in the list" in r)), r
    for p in range(P):
        r = sr.check_sandwich(tr.lists_of(tr.fold_pass_bits(ideal, P, combine, skip=p)), must_in, must_out)
        assert r is not None, p
        # ... and it is q*'s probe of that token that shows it
        cand = tr.fold_pass_bits(ideal, P, combine, skip=p)[tr.QSTAR]
        probe = (c["kind"] == tr.KINDS.index("min-probe" if combine == "min" else "max-probe")) & (c["probe_p"] == p)
        assert probe.sum() >= 256 // P and (cand[probe].all() if combine == "min" else not cand[probe].any()), p


@pytest.mark.parametrize("args", tr.STAGED + [tr.TIES + (True,)], ids=str)
def test_planted_staged_cases(args):
    c = tr.staged_case(*args)
    assert len(c["sched"]["slices"]) >= 2 and c["sched"]["slices"][-1][2] == S and c["sched"]["tail_live"]
    for thr0 in (c["thr0"], None):
        no_overflow(c, thr0=thr0)
    with np.errstate(invalid="ignore"):
        taus = tr.slice_taus(c["combined"], tr.staged_floor(c), c["k"], c["sched"]["images"])
    assert not (np.diff(taus.astype(np.float64), axis=0) < 0).any() and (taus[-1] > taus[0]).any()     # a threshold that rises
    if c["tie"]:
        a, b = c["tie"]
        assert c["combined"][0, a] == c["combined"][0, b] == c["combined"][0].max()
        assert a < b and c["k"] == 1 and tr.expected_list(c["combined"][0], 1) == {int(tr.image_key(c["combined"][0, a], a))}
    # the mutants on the last slice, against the threshold in force there
    P, combine = c["P"], c["combine"]
    tau = taus[len(c["sched"]["slices"]) - 1]
    _, mo_rows = sr.sandwich(tau, c["score"], c["hw"], c["rows"])
    must_in, must_out = tr.image_classes(c, tau)
    last = c["sched"]["images"][-1]
    assert not (~must_in & ~must_out)[tr.QSTAR][c["kind"] != 0].any()          # no planted image is a don't-care at that threshold
    only = lambda cand: [np.flatnonzero(row & last) for row in cand]
    mi_l, mo_l = must_in & last[None, :], must_out & last[None, :]
    assert sr.check_sandwich(only(tr.fold_pass_bits(~mo_rows, P, combine)), mi_l, mo_l) is None
    assert sr.check_sandwich(only(tr.fold_pass_bits(~mo_rows, P, combine, wrong="swap")), mi_l, mo_l) is not None
    for p in range(P):
        assert sr.check_sandwich(only(tr.fold_pass_bits(~mo_rows, P, combine, skip=p)), mi_l, mo_l) is not None, p


@pytest.mark.parametrize("args", [(P, ("min", "max")[n % 2], ("fp16", "bf16")[(n // 2) % 2]) for n, P in enumerate(tr.PS)], ids=str)
def test_open_cases(args):
    """No floor: every image without a NaN row is must-be-in (its rows score at or above -inf), none is must-be-out."""
    c = tr.open_case(*args)
    tau = np.full(c["Q"], -INF, np.float32)
    must_in, must_out = tr.image_classes(c, tau)
    nan_img = np.isnan(c["flat"]).any(axis=1).reshape(c["N"], c["P"]).any(axis=1)
    assert nan_img.sum() >= 2 and must_in[:, ~nan_img].all() and not must_out.any() and c["N"] <= sr.cap_of(c["k"])
    if c["combine"] == "min":
        assert not must_in[:, nan_img].any()
    elif c["P"] > 1:
        assert must_in[:, nan_img].all()


SELECTED = tr.SELECTED


@pytest.mark.parametrize("args", SELECTED, ids=str)
def test_selected_cases(args):
    """Under the selection: whole tiles dead, the live list ends in the tail tile, the image with the unboundable row is deselected
    and the planted images that stay keep their classes; the wrong folds are still rejected."""
    c = tr.selected_case(args)
    f = tr.selection_of(c)
    tiles, cum, last_live, de, sched = tr.selected_schedule(c, f)
    assert last_live == 1 and sched["tail_live"] and 0 not in tiles and c["lead"] + 1 not in tiles and len(tiles) < -(-c["N"] * c["P"] // 256)
    ub = c["rref"]["unb"].reshape(c["N"], c["P"]).any(axis=1)
    assert ub.sum() == 1 and not f[ub].any()
    assert (len(sched["slices"]) > 1) == (args[-1] == "staged")
    thr0 = tr.selected_floor(c, f)
    no_overflow(c, f, sched, thr0=thr0)
    combined = np.where(f[None, :], c["combined"], np.float32(-INF))
    taus = tr.slice_taus(combined, thr0, c["k"], sched["images"])
    tau = taus[len(sched["slices"]) - 1]
    must_in, must_out = tr.image_classes(c, tau, f)
    last = sched["images"][-1]
    planted = (c["kind"] != 0) & f
    assert last[planted].all() and not (~must_in & ~must_out)[tr.QSTAR][planted].any() and planted.sum() > 128 // c["P"]
    _, mo_rows = sr.sandwich(tau, c["score"], c["hw"], c["rows"])
    ideal = ~mo_rows & np.repeat(f, c["P"])[None, :]
    only = lambda cand: [np.flatnonzero(row & last) for row in cand]
    mi_l, mo_l = must_in & last[None, :], must_out & last[None, :]
    assert sr.check_sandwich(only(tr.fold_pass_bits(ideal, c["P"], c["combine"])), mi_l, mo_l, allowed=f) is None
    if c["P"] > 1:
        assert sr.check_sandwich(only(tr.fold_pass_bits(ideal, c["P"], c["combine"], wrong="swap")), mi_l, mo_l, allowed=f) is not None


def test_model_qpar_hand_cases():
    """Powers of two, so that every step but the named one is exact: eps = 2^-20, qbase = {4, 1, 0.5, .}."""
    f = np.float32
    qb = np.array([[4.0, 1.0, 0.5, 9.0]] * 3 + [[1.0, 3.0, 0.5, 9.0]], dtype=f)
    tau = np.array([-2.0, 2.0, 0.0, -INF], dtype=f)
    got = tr.model_qpar(tau, qb, eps=2.0 ** -20)
    c = f(1.0 + 2.0 ** -19)
    big = float(f(-3.0e38))
    want = np.array([
        [8.0 + 2.0 ** -16, c, 2.0 ** -20 * (1 + 2.0 ** -19), 0.0],       # negative tau: a, b grow in magnitude (lowered)
        [-(8.0 - 2.0 ** -16), c, -(2.0 ** -20 * (1 - 2.0 ** -19)), 0.0],
        [-0.0, c, -0.0, 0.0],
        [-big, f(3.0) * c, -float(f(big * 2.0 ** -21 * (1 + 2.0 ** -19))), 0.0],   # -inf: t = -3e38, a lowered past the clamp and put back
    ], dtype=f)
    assert np.array_equal(sr.f32bits(got), sr.f32bits(want)), (got, want)
    assert f(big * (1 + 2.0 ** -19)) < f(big)                       # (the lowered a does cross the clamp)


def test_slice_taus_hand_cases():
    sc = np.array([[0.5, -INF, 0.5, -0.25, 0.75, -INF]], dtype=np.float32)
    sl = [np.array([1, 1, 0, 0, 0, 0], bool), np.array([0, 0, 1, 1, 0, 0], bool), np.array([0, 0, 0, 0, 1, 1], bool)]
    assert tr.slice_taus(sc, None, 2, sl)[:, 0].tolist() == [-INF, -INF, 0.5, 0.5]          # fewer than k finite; a tie at the k-th place
    assert tr.slice_taus(sc, np.array([np.nan], np.float32), 2, sl)[:, 0].tolist() == [-INF, -INF, 0.5, 0.5]
    assert tr.slice_taus(sc, np.array([-0.1], np.float32), 2, sl)[:, 0].tolist() == [np.float32(-0.1)] * 2 + [0.5, 0.5]
    assert tr.slice_taus(sc, None, 3, sl)[:, 0].tolist() == [-INF, -INF, -0.25, 0.5]        # a negative threshold
    assert tr.slice_taus(sc, None, 5, sl)[:, 0].tolist() == [-INF] * 4                      # never k finite images
    assert tr.slice_taus(sc, np.array([0.9], np.float32), 1, sl)[:, 0].tolist() == [np.float32(0.9)] * 4


def test_image_key_and_expected_list():
    k = lambda s, i: int(tr.image_key(np.float32(s), i))
    assert k(2.0, 1) > k(2.0, 2) > k(1.0, 0) > k(0.0, 5) > k(-1.0, 0) > k(-2.0, 0) > k(-INF, 0) > 0
    sc = np.array([1.0, 2.0, 2.0, -INF], np.float32)
    assert tr.expected_list(sc, 1) == {k(2.0, 1)} and tr.expected_list(sc, 2) == {k(2.0, 1), k(2.0, 2)}
    assert tr.expected_list(sc, 4) == {k(2.0, 1), k(2.0, 2), k(1.0, 0)}
    bits, img = tr.key_parts(np.array(sorted(tr.expected_list(sc, 4)), np.uint64))
    assert sorted(img.tolist()) == [0, 1, 2] and set(bits.tolist()) == set(sr.f32bits(np.array([1.0, 2.0], np.float32)).tolist())


@pytest.mark.parametrize("P,tiles_all", tr.PREPARE_SHAPES)
def test_prepare_restatement_at_the_large_shapes(P, tiles_all):
    N = tr.prepare_shape(P, tiles_all)
    assert N % 32 != 0 and (N * P) % 256 != 0 and -(-N * P // 256) == tiles_all
    rowp = tr.prepare_rowp(N, P)
    for kind in tr.PREPARE_SELECTIONS:
        f = tr.prepare_selection(kind, N, P, tiles_all)
        a, b = tps.prepare(rowp, f, P), tr.prepare_loop(rowp, f, P)
        assert np.array_equal(sr.f32bits(a[0]), sr.f32bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
        assert len(a[1]) >= 1 and (kind != "all" or len(a[1]) == tiles_all) and (kind != "last" or a[1].tolist() == [tiles_all - 1])
        if kind == "seam" and tiles_all > 1024:
            assert a[1].tolist() == [1023, 1024]
