"""GPU: the patch-token route of the two-stage many-query search IMAGE BY IMAGE, against the statements of
tests/token_prefilter_stage_reference.py: the fold of the pass bits over an image's P rows (every token position and every image
position of a tile decides a planted image of the designated query on its own), the threshold and test parameters
token_rescore_body publishes after every slice, the running list, and skyemb_token_prefilter_select_prepare element by element at
shapes that cross its 64-tile wave seam and its 1024-tile round seam.  tests/test_token_prefilter_stage_cpu.py shows that the
planted images are in the classes the cases need, that no list or staging region can fill, and that the sandwich rejects a fold
that ORs, ANDs or leaves a token out.

Everything goes through the C ABI with the guarded buffers of tests/prefilter_gpu_harness.TokenSearch and idx_offset = 2^33 + 7.
Each case prints one STAGE line (profiles/r22_token_prefilter_stage.json keeps them)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import prefilter_stage1_reference as sr
from tests import token_prefilter_select_reference as tps
from tests import token_prefilter_stage_reference as tr
from tests import token_search_reference as tsr
from tests.prefilter_gpu_harness import FILL32, Guarded, TokenSearch, dev, ptr, set_lo, stream

INF = tr.INF
OFFSET = 2 ** 33 + 7
KIND = {name: i for i, name in enumerate(tr.KINDS)}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()
    return _ops


def run(ops, c, thr0, flags=None):
    return TokenSearch(ops, c["fmt"], c["tw"], c["qn"], c["xw"], c["xn"], c["k"], c["combine"], thr0, flags, OFFSET)


def record(case, c, must_in, must_out, listed, scope=None, **more):
    """scope (boolean [N]): the images the classes were stated for (the last slice, the selection); the zero query is left out."""
    pairs = np.ones((c["Q"], c["N"]), dtype=bool) if scope is None else np.repeat(scope[None, :], c["Q"], axis=0)
    hide(c, pairs)
    line = dict(case=case, P=c["P"], combine=c["combine"], fmt=c["fmt"], lo="hi+lo" if c["lo"] else "hi", Q=c["Q"], N=c["N"], k=c["k"],
                **tr.counts(must_in, must_out, listed, pairs), **more)
    print("STAGE", json.dumps(line))


def hide(c, *masks):
    """The planted zero query is handed back by the route (redo): its list serves nothing, so no class is stated for it."""
    if c["zero_q"] is not None:
        for m in masks:
            m[c["zero_q"]] = False
    return masks


def slice_sandwich(s, c, sched, taus, flags=None):
    """The LAST slice's complete candidate sets against the threshold in force during it; what is left of every earlier slice:
    nothing that was must-be-out against that slice's own threshold; nothing outside the selection anywhere.
    -> (must_in, must_out, listed) of the last slice."""
    n = len(sched["slices"])
    last = sched["images"][-1]
    must_in, must_out = tr.image_classes(c, taus[n - 1], flags)
    must_in, must_out = hide(c, must_in & last[None, :], must_out & last[None, :])
    lists = [s.candidates(q, last) for q in range(s.Q)]
    r = sr.check_sandwich(lists, must_in, must_out, allowed=flags)
    assert r is None, r
    for q in range(s.Q):
        every = s.candidates(q)
        assert len(every) == 0 or (every.min() >= 0 and every.max() < s.N), q
        assert flags is None or flags[every].all(), (q, "a deselected image is listed")
    for i in range(n - 1):
        _, mo = hide(c, *tr.image_classes(c, taus[i], flags))
        for q in range(s.Q):
            rem = s.candidates(q, sched["images"][i])
            assert not mo[q][rem].any(), (i, q, "a remnant of an earlier slice was must-be-out against that slice's threshold")
    return must_in, must_out, sum(len(l) for q, l in enumerate(lists) if q != c["zero_q"])


def probes_of_qstar(s, c, images=None, flags=None):
    """q*'s planted images one by one: every probe that must be absent is absent, every one that must be present is present."""
    have = np.zeros(c["N"], dtype=bool)
    have[s.candidates(tr.QSTAR, images)] = True
    on = np.ones(c["N"], dtype=bool) if flags is None else flags
    kind, P = c["kind"], c["P"]
    if c["combine"] == "min":
        absent = (kind == KIND["min-probe"]) | (kind == KIND["all-low"]) | ((kind == KIND["max-probe"]) if P > 1 else False)
        present = (kind == KIND["all-high"]) | ((kind == KIND["max-probe"]) if P == 1 else False)
    else:
        present = (kind == KIND["max-probe"]) | (kind == KIND["all-high"]) | ((kind == KIND["min-probe"]) if P > 1 else False)
        absent = (kind == KIND["all-low"]) | ((kind == KIND["min-probe"]) if P == 1 else False)
    wrong = np.flatnonzero(absent & on & have)
    assert len(wrong) == 0, ("listed", wrong[:8].tolist(), c["probe_p"][wrong[:8]].tolist())
    lost = np.flatnonzero(present & on & ~have)
    assert len(lost) == 0, ("not listed", lost[:8].tolist(), c["probe_p"][lost[:8]].tolist())
    assert (absent & on).sum() >= 1 and (present & on).sum() >= 1


def published_state(s, c, taus, flags=None):
    """What token_rescore_body leaves: tau, qpar, the running list and its length, cnt, the outputs, the flags, the guards."""
    Q, k, zq = s.Q, s.k, c["zero_q"]
    combined = c["combined"] if flags is None else np.where(flags[None, :], c["combined"], np.float32(-INF))
    keep = np.arange(Q) != (-1 if zq is None else zq)
    assert s.guards_ok
    assert np.array_equal(sr.f32bits(s.ws["tau"])[keep], sr.f32bits(taus[-1])[keep]), (s.ws["tau"], taus[-1])
    want = tr.model_qpar(s.ws["tau"], s.ws["qbase"])
    assert np.array_equal(sr.f32bits(s.ws["qpar"][:Q]), sr.f32bits(want)), np.argwhere(sr.f32bits(s.ws["qpar"][:Q]) != sr.f32bits(want))[:4]
    assert np.isnan(s.ws["qpar"][Q:]).all()
    assert (s.ws["cnt"] == 0).all()
    assert np.array_equal(s.redo != 0, s.ws["overflow"] != 0) and (s.redo != 0).tolist() == [q == zq for q in range(Q)], s.redo
    # (an image scoring above -inf that stage 1 did not list lay below a finite tau, which k such images had set: the count of
    # must-in or listed images with a finite score reaches k exactly when the count of all of them does)
    finite = (combined > -INF).sum(axis=1)
    ref_s, ref_i = tsr.topk_of_scores(combined, k, OFFSET)
    for q in np.flatnonzero(keep):
        assert s.rn[q] == min(k, finite[q]), (q, s.rn[q], finite[q])
        got = s.list[q, :s.rn[q]].tolist()
        assert len(set(got)) == len(got) and set(got) == tr.expected_list(combined[q], k), q
        assert np.array_equal(s.out_i[q], ref_i[q]) and np.array_equal(sr.f32bits(s.out_s[q]), sr.f32bits(ref_s[q])), (q, s.out_i[q], ref_i[q])


# ------------------------------------------------------------------------------------------------------------ a. one slice, a floor
@pytest.mark.parametrize("args", tr.SINGLE, ids=lambda a: f"P{a[0]}-{a[1]}-{a[2]}-{'hilo' if a[3] else 'hi'}-{'tail' if a[4] else 'whole'}")
def test_fold_single_slice(ops, monkeypatch, args):
    set_lo(monkeypatch, args[3])
    c = tr.single_case(*args)
    s = run(ops, c, c["thr0"])
    taus = tr.slice_taus(c["combined"], c["thr0"], c["k"], c["sched"]["images"])
    must_in, must_out, listed = slice_sandwich(s, c, c["sched"], taus)
    record("single", c, must_in, must_out, listed)
    probes_of_qstar(s, c)
    published_state(s, c, taus)


# ------------------------------------------------------------------------------------------------------------ b. one slice, no floor
OPEN = [(P, ("min", "max")[n % 2], ("fp16", "bf16")[(n // 2) % 2]) for n, P in enumerate(tr.PS)]


@pytest.mark.parametrize("args", OPEN, ids=lambda a: f"P{a[0]}-{a[1]}-{a[2]}")
def test_fold_open(ops, monkeypatch, args):
    set_lo(monkeypatch, False)
    c = tr.open_case(*args)
    s = run(ops, c, None)
    tau = np.full(c["Q"], -INF, np.float32)
    must_in, must_out = tr.image_classes(c, tau)
    lists = [s.candidates(q) for q in range(s.Q)]
    r = sr.check_sandwich(lists, must_in, must_out)
    assert r is None, r
    clean = ~np.isnan(c["flat"]).any(axis=1).reshape(c["N"], c["P"]).any(axis=1)
    for q in range(s.Q):
        assert np.array_equal(np.sort(lists[q][clean[lists[q]]]), np.flatnonzero(clean)), q          # exactly once each
    record("open", c, must_in, must_out, sum(len(l) for l in lists))
    published_state(s, c, tr.slice_taus(c["combined"], None, c["k"], c["sched"]["images"]))


# ------------------------------------------------------------------------------------- c, d. staged slices and the published state
@pytest.mark.parametrize("args", tr.STAGED + [tr.TIES + (True,)], ids=lambda a: f"P{a[0]}-{a[1]}-{a[2]}-{'hilo' if a[3] else 'hi'}{'-ties' if len(a) > 4 else ''}")
def test_staged_slices_and_published_state(ops, monkeypatch, args):
    set_lo(monkeypatch, args[3])
    c = tr.staged_case(*args)
    thr0 = tr.staged_floor(c)                                          # with a floor ('min') and without ('max')
    s = run(ops, c, thr0)
    taus = tr.slice_taus(c["combined"], thr0, c["k"], c["sched"]["images"])
    must_in, must_out, listed = slice_sandwich(s, c, c["sched"], taus)
    record("staged-ties" if c["tie"] else "staged", c, must_in, must_out, listed, c["sched"]["images"][-1], slices=len(c["sched"]["slices"]))
    probes_of_qstar(s, c, c["sched"]["images"][-1])
    published_state(s, c, taus)
    if c["tie"]:
        a, b = c["tie"]
        assert s.out_i[0, 0] == a + OFFSET and b in s.candidates(0, c["sched"]["images"][-1])     # listed, re-scored, and the lower image kept


# ------------------------------------------------------------------------------------------------------------------ e. a selection
@pytest.mark.parametrize("args", tr.SELECTED, ids=lambda a: f"P{a[0]}-{a[1]}-{a[2]}-{'hilo' if a[3] else 'hi'}-{a[-1] if a[-1] == 'staged' else 'single'}")
def test_fold_under_a_selection(ops, monkeypatch, args):
    set_lo(monkeypatch, args[3])
    c = tr.selected_case(args)
    f = tr.selection_of(c)
    tiles, cum, last_live, de, sched = tr.selected_schedule(c, f)
    thr0 = tr.selected_floor(c, f)
    s = run(ops, c, thr0, f)
    assert s.tiles.tolist() == tiles.tolist() and s.cum == cum.tolist() and s.last_live == last_live and s.direct_end == de
    combined = np.where(f[None, :], c["combined"], np.float32(-INF))
    taus = tr.slice_taus(combined, thr0, c["k"], sched["images"])
    must_in, must_out, listed = slice_sandwich(s, c, sched, taus, f)
    record("selected", c, must_in, must_out, listed, sched["images"][-1] & f, slices=len(sched["slices"]), selected=int(f.sum()), live_tiles=len(tiles))
    probes_of_qstar(s, c, sched["images"][-1], f)
    published_state(s, c, taus, f)


# ----------------------------------------------------------------------------------------------- f. the preparation, per element
@pytest.mark.parametrize("P,tiles_all", tr.PREPARE_SHAPES)
def test_select_prepare_per_element(ops, P, tiles_all):
    L = ops.lib()
    N = tr.prepare_shape(P, tiles_all)
    rowp = tr.prepare_rowp(N, P)
    rowp_d = dev(rowp)
    for kind in tr.PREPARE_SELECTIONS:
        f = tr.prepare_selection(kind, N, P, tiles_all)
        want_rowp, want_tiles, want_cum, want_last = tps.prepare(rowp, f, P)
        bits = np.zeros(-(-N // 32) * 32, dtype=np.uint8)
        bits[:N] = f
        words = dev(np.packbits(bits, bitorder="little").view(np.uint32).view(np.int32))
        out, tiles, cum, info = Guarded(rowp.nbytes), Guarded(tiles_all * 4), Guarded(tiles_all * 4), Guarded(8)
        rc = L.skyemb_token_prefilter_select_prepare(ptr(words), N, P, ptr(rowp_d), out.ptr(), tiles.ptr(), cum.ptr(), info.ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0, L.skyemb_last_error()
        assert all(g.intact() for g in (out, tiles, cum, info)), kind
        n_live, last = info.np(np.int32, 2).tolist()
        assert (n_live, last) == (len(want_tiles), want_last), (kind, n_live, last)
        got_t, got_c = tiles.np(np.int32, tiles_all), cum.np(np.int32, tiles_all)
        assert np.array_equal(got_t[:n_live], want_tiles) and np.array_equal(got_c[:n_live], want_cum), kind
        assert (got_t[n_live:] == FILL32).all() and (got_c[n_live:] == FILL32).all(), (kind, "written past n_live")
        assert np.array_equal(out.np(np.uint32, -1, 4), sr.f32bits(want_rowp)), kind                 # a NaN as its bit pattern
