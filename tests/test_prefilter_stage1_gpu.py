"""GPU: stage 1 of the two-stage many-query search, quantity by quantity and PAIR BY PAIR, against the statements of
tests/prefilter_stage1_reference.py: the row constants and the fp16 image of the three preparation kernels, the query images and
constants, every matrix-core dot product (to the bit, on integer-grid inputs), the proven bound on every pair of ordinary data,
and the candidate lists and thresholds of each append path at a threshold that is known.  tests/test_prefilter_stage1_cpu.py pins
the phase table this file relies on and shows that every checker rejects the defect it exists for.

Everything goes through the C ABI.  Outputs and the workspace lie in pre-filled buffers with 256 guard bytes on either side; the
guards are checked after every call.  The workspace is read through skyemb_topk_prefilter_ws_layout."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import similarity_oracle as so
from tests import prefilter_stage1_reference as sr
from tests.prefilter_stage1_reference import EPS, K
from tests.prefilter_gpu_harness import FILL32, Search, patterns16, prepare, set_lo


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()
    return _ops


# ------------------------------------------------------------------------------------------------------------ a: row constants, image
def planted_rows(fmt, N, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D)) * 10.0 ** rng.uniform(-3, 3, size=(N, 1))           # six decades of scale
    x[1] = 0
    x[2, 5] = np.inf
    x[3, D - 1] = np.nan
    x[4] = rng.standard_normal(D) * 2.0 ** -17                                           # fp16 subnormals only
    x[5, 9] = 2.0 ** -16                                                                  # exactly one subnormal
    x[5, :9] = np.abs(x[5, :9]) + 0.01
    x[5, 10:] = np.abs(x[5, 10:]) + 0.01
    x[6] = rng.standard_normal(D) * 2.0 ** -122                                          # fp32 route: e < -126
    x[6, 0] = 2.0 ** -120
    x[N - 10, 1] = -np.inf                                                               # ... and in the tail tile
    x[N - 1] = 0
    if fmt == "bf16":
        step = 2.0 ** -7
        for i, v in enumerate([2.0 ** -60, 2.0 ** -60 * (1 + step), 2.0 ** -60 * (1 - step / 2), 2.0 ** 120, 2.0 ** 120 * (1 - step / 2),
                               2.0 ** 120 * (1 + step)]):
            x[7 + i] = rng.standard_normal(D)
            x[7 + i, 3 + i] = v
    x = sr.store(x, fmt)
    w = (rng.random(D, dtype=np.float32) + 0.1).astype(np.float32)
    xn = so.wnorms_np(np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0), w)
    bad = ~np.isfinite(x.astype(np.float64)).all(axis=1)
    xn[bad] = np.where(np.isnan(x[bad]).any(axis=1), np.nan, np.inf)
    if fmt == "bf16":
        xn[11] = 1.5e38                # (the oracle's own chain overflows on 2^240: the element rule is tested apart from the norm rule)
        xn[13], xn[14] = np.inf, np.nan                                                   # finite rows whose weighted norm is not
    return x, xn


ROW_CASES = [("fp32", 128), ("fp32", 288), ("fp32", 132), ("fp16", 128), ("fp16", 288), ("bf16", 128), ("bf16", 288)]


@pytest.mark.parametrize("fmt,D", ROW_CASES, ids=[f"{f}-D{d}" for f, d in ROW_CASES])
def test_row_constants_and_image_per_element(ops, fmt, D):
    N = 300
    x, xn = planted_rows(fmt, N, D, 1000 + D)
    ref = sr.row_constants(x, xn, fmt, D)
    want_unb = {2, N - 10} | ({6} if fmt == "fp32" else set()) | ({3} if fmt != "fp32" else set()) | ({6, 9, 10, 12, 13, 14} if fmt == "bf16" else set())
    assert set(np.flatnonzero(ref["unb"]).tolist()) == want_unb, np.flatnonzero(ref["unb"])
    assert ref["nanrow"].sum() == (fmt == "fp32")
    bank, xn_d, rowp, side = prepare(ops, fmt, x, xn)
    got = rowp.np(np.float32, 512, 4)
    r = sr.check_rowp(got, ref)
    print(fmt, D, "nx' / norm - 1 over the ordinary rows: max", np.nanmax(np.where(ref["unb"] | ref["nanrow"] | (ref["norm"] == 0), np.nan,
                                                                                got[:N, 1] / np.maximum(ref["nx_lo"], 1e-300) - 1)))
    assert r is None, r
    if fmt == "fp32":
        r = sr.check_image(side.np(np.uint16, 512, D), ref)
        assert r is None, r
    else:
        tail = side.np(np.uint16, 256, D)
        assert np.array_equal(tail[:N - 256], patterns16(bank)[256:N]) and (tail[N - 256:] == 0).all()
    # N = 256 and no tail tile: nothing but rowp's 256 rows is written
    x2, xn2 = x[:256], xn[:256]
    _, _, rowp2, side2 = prepare(ops, fmt, x2, xn2)
    assert rowp2.n == 256 * 16 and (side2 is None) == (fmt != "fp32")
    ref2 = sr.row_constants(x2, xn2, fmt, D)
    r = sr.check_rowp(rowp2.np(np.float32, 256, 4), ref2)
    assert r is None, r
    if fmt == "fp32":
        assert side2.n == 256 * D * 2 and sr.check_image(side2.np(np.uint16, 256, D), ref2) is None


# ------------------------------------------------------------------------------------------------------------ b: query constants
@pytest.mark.parametrize("lo", [False, True], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("D", [128, 288])
@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_query_constants_per_element(ops, monkeypatch, fmt, D, lo):
    set_lo(monkeypatch, lo)
    rng = np.random.default_rng(D + 7)
    Q, N = 261, 2048
    tw = (rng.standard_normal((Q, D)) * 10.0 ** rng.uniform(-6, 6, size=(Q, 1))).astype(np.float32)
    tw[0] = 0
    tw[1] = rng.uniform(-1, 1, D).astype(np.float32) * np.float32(2.0 ** -121)
    tw[1, 3] = 2.0 ** -120                                              # the scale clamp
    tw[2] = rng.uniform(-1, 1, D).astype(np.float32) * np.float32(2.0 ** -52)
    tw[2, 4] = 2.0 ** -51                                               # bf16: 2^-f = 2^30, outside (Q)
    tw[3] = rng.uniform(-1, 1, D).astype(np.float32) * np.float32(2.0 ** 79)
    tw[3, 5] = 2.0 ** 80                                                # bf16: clamped at 2^-100
    qn = (np.abs(rng.standard_normal(Q)) + 0.5).astype(np.float32)
    x = sr.store(rng.standard_normal((N, D)), fmt)
    xn = so.wnorms_np(x, None)
    s = Search(ops, fmt, tw, qn, x, xn, K)
    ref = sr.query_constants(tw, qn, fmt, D, sr.eps_a_f32(fmt, D, lo))
    assert np.flatnonzero(ref["flagged"]).tolist() == ([1] if fmt == "fp16" else [1, 2, 3])
    assert s.guards_ok
    r = sr.check_query(s.ws["qh"], s.ws["ql"], s.ws["qbase"], ref, lo)
    assert r is None, r
    r = sr.check_flags(s.ws["overflow"], s.redo, ref)
    assert r is None, r
    assert np.isnan(s.ws["qpar"][Q:]).all()                            # the padding of the last query tile lets no pair pass


# ------------------------------------------------------------------------------------------- c: every dot^, to the bit (take-all)
TAKE_ALL = [(fmt, lo, D) for fmt in sr.FMTS for lo in (False, True) for D in (128, 192)]


@pytest.mark.parametrize("fmt,lo,D", TAKE_ALL, ids=[f"{f}-{'hi+lo' if l else 'hi'}-D{d}" for f, l, d in TAKE_ALL])
def test_every_dot_product_to_the_bit(ops, monkeypatch, fmt, lo, D):
    """Integer-grid inputs (exact_grid_case): all Q x N accumulators of the tile kernel, every wave, fragment, block and k-step,
    in both operand formats and both pass counts; the tail tile's direct appends; then the final answer on the redo = 0 queries."""
    set_lo(monkeypatch, lo)
    Q, N = (700 if lo else 1300), sr.TAKE_ALL_N[fmt]
    assert sr.schedule(N, K, False, fmt != "fp32")["launches"] == sr.PHASES[(N, False, fmt != "fp32")]
    g = sr.exact_grid_case(fmt, lo, Q, N, D, seed=D + lo)
    tw, qn = so.prep_queries_np(g["tw"], None)
    assert np.array_equal(tw, g["tw"])
    xn = so.wnorms_np(g["x"], None)
    s = Search(ops, fmt, tw, qn, g["x"], xn, K)
    assert s.guards_ok
    r = sr.check_take_all(s.ws["cnt"], s.ws["cand_i"], s.ws["cand_d"], g["dot"], 2048)
    assert r is None, r
    if N > 2048:
        r = sr.check_tail_appends(s.ws["cnt"], s.ws["cand_i"], s.ws["cand_d"], g["dot"], 2048, N)
        assert r is None, r
    assert (s.ws["cnt"] == N).all() and (s.ws["overflow"] == 0).all()
    assert (s.ws["cand_i"][:, N:] == FILL32).all()                     # nothing behind the lists
    ref_s, ref_i = so.cosine_topk_np(g["tw"], g["x"], K, None)
    ok = s.redo == 0
    print(fmt, lo, D, "queries certified:", int(ok.sum()), "of", Q)
    assert set(np.unique(s.redo).tolist()) <= {0, 1}
    assert np.array_equal(s.out_i[ok], ref_i[ok]) and np.array_equal(s.out_s[ok].view(np.uint32), ref_s[ok].view(np.uint32))


# ----------------------------------------------------------------------------------------------- d: the bound on ordinary data
@pytest.mark.parametrize("fmt,lo,D", TAKE_ALL, ids=[f"{f}-{'hi+lo' if l else 'hi'}-D{d}" for f, l, d in TAKE_ALL])
def test_every_pair_within_the_proven_bound(ops, monkeypatch, fmt, lo, D):
    """|dot^ - chain(tw, x) 2^-(e+f)| <= qbase.y nx' for EVERY pair of the take-all shapes, with the device's own constants: the
    project's inequality, no tolerance.  Largest error / bound observed on the MI355X (profiles/r20_prefilter_stage1_margins.json;
    nothing is asserted about how small it is)."""
    set_lo(monkeypatch, lo)
    Q, N = (700 if lo else 1300), sr.TAKE_ALL_N[fmt]
    c = sr.pair_case(fmt, lo, Q, N, D, 40 + D, 4 if fmt == "fp16" else 0)
    if fmt == "fp16":
        assert (c["rref"]["nx_lo"] > 1.5 * c["rref"]["norm"]).sum() >= 2          # the planted subnormal rows carry their term
    s = Search(ops, fmt, c["tw"], c["qn"], c["x"], c["xn"], K)
    assert s.guards_ok and (s.ws["cnt"] == N).all()
    lst = np.sort(s.ws["cand_i"][:, :N], axis=1)
    assert (lst == np.arange(N)[None, :]).all()
    r = sr.check_rowp(s.rowp, c["rref"])
    assert r is None, r
    r = sr.check_query(s.ws["qh"], s.ws["ql"], s.ws["qbase"], c["qref"], lo)
    assert r is None, r
    chain = sr.chain_scaled(sr.chain_all(c["tw"], c["x"]), c["qref"], c["rref"])
    r, ratio = sr.check_pair_bound(s.dense_dots(N), chain, s.ws["qbase"][:, 1], s.rowp[:N, 1])
    print(f"MARGIN {fmt} {'hi+lo' if lo else 'hi'} D{D} {ratio:.6f}")
    assert r is None, r


# ------------------------------------------------------------------ e: the candidate test and the append paths at a known threshold
def listed_pairs_within_bound(s, c):
    chain = sr.chain_scaled(sr.chain_all(c["tw"], c["x"]), c["qref"], c["rref"])
    y, nx = s.ws["qbase"][:, 1].astype(np.float64), s.rowp[:, 1].astype(np.float64)
    for q, rows in enumerate(s.lists()):
        rows = rows.astype(np.int64)
        err = np.abs(s.ws["cand_d"][q, :len(rows)].astype(np.float64) - chain[q, rows])
        if not (err <= y[q] * nx[rows]).all():
            return f"query {q}: the dot^ of listed row {rows[np.argmax(~(err <= y[q] * nx[rows]))]} is outside the bound"
    return None


def constants_ok(s, c, lo):
    return sr.check_rowp(s.rowp, c["rref"]) or sr.check_query(s.ws["qh"], s.ws["ql"], s.ws["qbase"], c["qref"], lo)


SANDWICH = [(fmt, lo) for fmt in sr.FMTS for lo in (False, True)]
SANDWICH_IDS = [f"{f}-{'hi+lo' if l else 'hi'}" for f, l in SANDWICH]


@pytest.mark.parametrize("fmt,lo", SANDWICH, ids=SANDWICH_IDS)
def test_staged_appends_at_a_known_floor(ops, monkeypatch, fmt, lo):
    """MODE 2 + bucket_kernel alone (N = 2048, thr0 = the oracle's k-th best over the first 1024 rows): no duplicates, every
    must-be-in row, no must-be-out row, every listed dot^ inside the bound."""
    set_lo(monkeypatch, lo)
    N = 2048
    assert sr.schedule(N, K, True, fmt != "fp32")["launches"] == [("mode2", 0, 8), ("select", 1)]
    c = sr.pair_case(fmt, lo, sr.SQ, N, sr.SD, sr.sandwich_seed(fmt))
    thr0 = sr.floor_of_first_rows(c, 1024, K)
    s = Search(ops, fmt, c["tw"], c["qn"], c["x"], c["xn"], K, thr0=thr0)
    assert s.guards_ok and constants_ok(s, c, lo) is None
    assert np.array_equal(s.ws["tau"].view(np.uint32), thr0.view(np.uint32)) and (s.ws["overflow"] == 0).all() and (s.ws["cnt"] <= s.cap).all()
    must_in, must_out = sr.sandwich(thr0, c["score"], c["hw"], c["contract"])
    print(fmt, lo, "list lengths", s.ws["cnt"].min(), s.ws["cnt"].max(), "must-in", must_in.sum(axis=1).min(), must_in.sum(axis=1).max())
    r = sr.check_sandwich(s.lists(), must_in, must_out) or listed_pairs_within_bound(s, c)
    assert r is None, r


@pytest.mark.parametrize("N", [2304, 2560])
@pytest.mark.parametrize("fmt,lo", SANDWICH, ids=SANDWICH_IDS)
def test_direct_appends_and_the_published_threshold(ops, monkeypatch, fmt, lo, N):
    """No floor.  N = 2304: take-all over tiles 0-7, a select that publishes tau and compacts, MODE 1 on tile 8, the final select --
    MODE 1 alone, under a tau that comes from rows 0 .. 2047.  N = 2560 (k = 5: the direct slice is one tile, so the driver runs
    MODE 1 on tile 8, a second non-final select that raises tau, then MODE 2 on tile 9): tau comes from rows 0 .. 2303.  Either way
    tau is a lower bound of the k-th best exact score over the rows it was taken from and not below it by more than 2 hw_max (+ the
    slack of sandwich()), and with that tau as the known threshold the sandwich holds over all N rows."""
    set_lo(monkeypatch, lo)
    seen = 2048 if N == 2304 else 2304
    assert sr.schedule(N, K, False, fmt != "fp32")["launches"] == sr.PHASES[(N, False, fmt != "fp32")]
    c = sr.pair_case(fmt, lo, sr.SQ, N, sr.SD, sr.sandwich_seed(fmt))
    s = Search(ops, fmt, c["tw"], c["qn"], c["x"], c["xn"], K)
    assert s.guards_ok and constants_ok(s, c, lo) is None
    assert (s.ws["overflow"] == 0).all() and (s.ws["cnt"] <= s.cap).all()
    tau = s.ws["tau"].astype(np.float64)
    tau_lo, tau_hi = sr.tau_window(c, np.arange(N) < seen, K)
    print(fmt, lo, N, "kth - tau: max", (tau_hi - tau).max(), "min", (tau_hi - tau).min(), "allowed", (tau_hi - tau_lo).min(), "lists", s.ws["cnt"].min(), s.ws["cnt"].max())
    assert (tau <= tau_hi).all(), int(np.argmax(tau > tau_hi))
    assert (tau >= tau_lo).all(), int(np.argmax(tau < tau_lo))
    must_in, must_out = sr.sandwich(tau, c["score"], c["hw"], c["contract"])
    assert (must_in.sum(axis=1) >= K).all() and (~must_in & ~must_out).mean(axis=1).max() <= 0.02
    r = sr.check_sandwich(s.lists(), must_in, must_out) or listed_pairs_within_bound(s, c)
    assert r is None, r
    ref_s, ref_i = so.cosine_topk_np(c["q"], c["x"], K, c["w"])
    ok = s.redo == 0
    assert ok.sum() >= sr.SQ * 9 // 10 and np.array_equal(s.out_i[ok], ref_i[ok]) and np.array_equal(s.out_s[ok].view(np.uint32), ref_s[ok].view(np.uint32))


@pytest.mark.parametrize("dead", [(3,), (3, 6)], ids=["9-live-tiles", "8-live-tiles"])
@pytest.mark.parametrize("lo", [False, True], ids=["hi", "hi+lo"])
def test_lists_under_a_selection(ops, monkeypatch, lo, dead):
    """A resident fp16 bank of 2560 rows under a random 50 % selection.  One dead tile: 9 live tiles -- take-all over positions 0-7,
    select, MODE 1 on position 8, final select: no deselected row in any list, the sandwich over the selected rows at the tau read
    back, the take-all survivors still in slot order.  Two dead tiles: 8 live tiles, the take-all slice is the whole search and
    stays as stored: slot = position * 256 + local, a deselected row's dot^ is -inf."""
    set_lo(monkeypatch, lo)
    N = 2560
    c = sr.pair_case("fp16", lo, sr.SQ, N, sr.SD, sr.sandwich_seed("fp16"))
    flags = sr.selection(N, dead, 5)
    s = Search(ops, "fp16", c["tw"], c["qn"], c["x"], c["xn"], K, flags=flags)
    live = [t for t in range(10) if t not in dead]
    assert s.guards_ok and s.tiles.tolist() == live
    assert sr.schedule(N, K, False, True, n_live=len(live), last_live=1)["launches"] == sr.PHASES_SEL[len(live)]
    # the masked constants: the statement's for a selected row, the sentinel for every other
    keep = np.flatnonzero(flags)
    assert s.rowp.shape == (N, 4) and np.isnan(s.rowp[~flags, 1]).all() and (sr.f32bits(s.rowp[~flags][:, [0, 2, 3]]) == 0).all()
    sub = {k_: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (N,) else v) for k_, v in c["rref"].items()}
    sub["N"] = len(keep)
    assert sr.check_rowp(s.rowp[keep], sub) is None
    y, nx = s.ws["qbase"][:, 1].astype(np.float64), s.rowp[:, 1].astype(np.float64)
    chain = sr.chain_scaled(sr.chain_all(c["tw"], c["x"]), c["qref"], c["rref"])
    if len(live) == 8:
        slot_rows = (np.array(live)[:, None] * 256 + np.arange(256)[None, :]).reshape(-1)
        assert (s.ws["cnt"] == 2048).all() and (s.ws["cand_i"][:, :2048] == slot_rows[None, :]).all()
        cd = s.ws["cand_d"][:, :2048]
        on = flags[slot_rows]
        assert np.isneginf(cd[:, ~on]).all() and np.isfinite(cd[:, on]).all()
        err = np.abs(cd[:, on].astype(np.float64) - chain[:, slot_rows[on]])
        assert (err <= y[:, None] * nx[slot_rows[on]][None, :]).all()
        assert (s.ws["cand_i"][:, 2048:] == FILL32).all()
    else:
        tau = s.ws["tau"].astype(np.float64)
        seen = flags & (np.arange(N) < (live[7] + 1) * 256)
        tau_lo, tau_hi = sr.tau_window(c, seen, K)
        assert (tau <= tau_hi).all() and (tau >= tau_lo).all()
        must_in, must_out = sr.sandwich(tau, c["score"], c["hw"], c["contract"])
        r = sr.check_sandwich(s.lists(), must_in & flags, must_out & flags, allowed=flags)
        assert r is None, r
        for q, rows in enumerate(s.lists()):
            first = rows[rows < (live[7] + 1) * 256]
            assert np.array_equal(first, np.sort(first)) and np.array_equal(first, rows[:len(first)]), q     # survivors keep the slot order
            err = np.abs(s.ws["cand_d"][q, :len(rows)].astype(np.float64) - chain[q, rows])
            assert (err <= y[q] * nx[rows]).all(), q
    # and the answer: the oracle over the selected rows
    ref_s, ref_i = so.cosine_topk_np(c["q"], c["x"][keep], K, c["w"])
    ok = s.redo == 0
    assert ok.sum() >= sr.SQ * 9 // 10 and np.array_equal(s.out_i[ok], keep[ref_i[ok]]) and np.array_equal(s.out_s[ok].view(np.uint32), ref_s[ok].view(np.uint32))


@pytest.mark.parametrize("fmt,lo", SANDWICH, ids=SANDWICH_IDS)
def test_overflowing_lists_are_refused_not_overrun(ops, monkeypatch, fmt, lo):
    """thr0 = -1 for every query: every pair passes, and an item's 256 x qtile pairs (44 x 256 in the ragged last query tile) meet a
    staging list of 2048 entries.  A defined refusal, not a fault: EVERY query comes back redo = 1 -- an item whose staging list
    overflows hands back all its queries, whichever pairs happened to find a slot --, and counts, indices and dot^ stay inside
    their arrays: nothing outside [0, N), nothing listed twice, nothing written behind a list, every listed dot^ inside the bound."""
    set_lo(monkeypatch, lo)
    N = 2048
    c = sr.pair_case(fmt, lo, sr.SQ, N, sr.SD, sr.sandwich_seed(fmt))
    s = Search(ops, fmt, c["tw"], c["qn"], c["x"], c["xn"], K, thr0=np.full(sr.SQ, -1.0, np.float32))
    assert s.guards_ok
    assert (s.redo == 1).all(), np.flatnonzero(s.redo != 1).tolist()
    assert (s.ws["overflow"] == 1).all()
    assert (s.ws["cnt"] >= 0).all() and (s.ws["cnt"] <= N).all()
    for q, rows in enumerate(s.lists()):
        assert len(rows) == 0 or (rows.min() >= 0 and rows.max() < N), q
        assert len(np.unique(rows)) == len(rows), q
        assert (s.ws["cand_i"][q, len(rows):] == FILL32).all(), q
    assert listed_pairs_within_bound(s, c) is None
