"""GPU: the two-stage many-query weighted-MSE search under ``top_t`` and under a selection of images --
``distance_topk_tokens(queries, TokenBank.resident(bank).prepare_mse_top_t(), k, 'MSE', combine, top_t=.., select=Selection(flags)
.prepare_mse(bank))``.

The reference of every case is the same call over the same device bank in a plain ``TokenBank`` with a Selection never asked (the
grouped route); distances are compared as int32 bits and indices must be equal.  D = 160 is a shape the grouped kernels do not take,
so there the library calls are compared with the NumPy restatement of the contract (tests/token_mse_prefilter_reference
.contract_distances) under the rules of tests/token_mse_select_topt_reference.py.

Selections: the route asks for at least 2048 selected token rows (hence 8 live whole tiles) and k <= selected images; the counts of
every selection used here are checked on the CPU (``ref.select_route_takes``).  A 10 % selection in runs of whole tiles meets that
only on a bank of at least 80 tiles, so it runs on (5120, 16); on (1024, 16) it is the case BELOW the limits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import token_distance_reference as tdr
from tests import token_mse_prefilter_reference as mpr
from tests import token_mse_select_topt_reference as ref

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
D = 128


@pytest.fixture(autouse=True)
def _min_q(monkeypatch):
    from sky_embeddings_amd import search
    for name in ("TOKEN_MSE_PREFILTER_MIN_Q", "TOKEN_MSE_PREFILTER_MIN_Q_SMALL", "TOKEN_MSE_TOPT_PREFILTER_MIN_Q",
                 "TOKEN_MSE_SELECT_PREFILTER_MIN_Q", "TOKEN_MSE_SELECT_TOPT_PREFILTER_MIN_Q"):
        monkeypatch.setattr(search, name, 17)


def _to16(x, dt):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DTYPES[dt])
    return t, t.float().numpy()


def _bank(rng, N, P, dt, d=D):
    """Images of very different scale whose tokens share a direction, as a 16-bit tensor and the fp32 array it widens to."""
    x = (rng.standard_normal((N, 1, d)) * rng.uniform(0.3, 2.0, (N, 1, 1)) + 0.7 * rng.standard_normal((N, P, d))).astype(np.float32)
    return _to16(x, dt)


def _flags(kind, N, P, rng):
    """half: 50 % at random; runs10: 10 % of the images in runs of whole 256-row tiles; all; most: one image dropped from every other
    tile."""
    ipt = 256 // P                                                 # images per tile
    f = np.zeros(N, bool)
    if kind == "all":
        f[:] = True
    elif kind == "half":
        f[:] = rng.random(N) < 0.5
    elif kind == "most":
        f[:] = True
        f[::2 * ipt] = False
    else:
        assert kind == "runs10"
        tiles = N // ipt
        n_runs, run = 4, tiles // 40                               # four runs of tiles / 40 whole tiles: 10 % of the images
        starts = rng.choice(np.arange(0, tiles - run, 2 * run), n_runs, replace=False)
        for s in starts:
            f[s * ipt:(s + run) * ipt] = True
    return f


def _search(q, bank, w, k, combine, off=0, top_t=None, flags=None, resident=True):
    """(distances, indices, stats) of one search: over the opted-in resident bank, or over the plain one (the grouped route)."""
    from sky_embeddings_amd import search
    qd, xd = torch.from_numpy(q).cuda(), bank.cuda()
    wd = None if w is None else torch.from_numpy(w).cuda()
    sel = None if flags is None else search.Selection(torch.from_numpy(flags), xd.device)
    if resident:
        tb = search.TokenBank.resident(xd, wd, off)
        if top_t:
            tb.prepare_mse_top_t()
        if sel is not None:
            sel.prepare_mse(tb)
    else:
        tb = search.TokenBank(xd, wd, off)
    stats = {}
    s, i = search.distance_topk_tokens(qd, tb, k, "MSE", combine, stats=stats, top_t=top_t, select=sel)
    return s, i, stats


def _both(*a, **kw):
    return _search(*a, **kw), _search(*a, resident=False, **kw)


def _assert_same(got, want):
    assert torch.equal(got[1], want[1]), (got[2], torch.nonzero(got[1] != want[1])[:5].tolist())
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), got[2]


def _assert_two_stage(st, combine, top_t=None, flags=None, P=None, N=None):
    assert st["path"] == "prefiltered" and st["combine"] == combine and st["metric"] == "MSE", st
    assert st["redone"] == 0, st                                   # benign data: no query is flagged, a list holds every image
    if top_t:
        assert st["top_t"] == top_t, st
    if flags is not None:
        tiles = ref.live_tiles(flags, P)[0]
        assert st["selected"] == int(flags.sum()) and st["tiles"] == (len(tiles), -(-N * P // 256)), st


# (N, P, dtype, SKYEMB_PREFILTER_LO, Q, k, idx_offset, top_t) under distance 'max': top_t in {1, 2, min(P, 16) - 1, min(P, 16)} on a
# ragged bank whose images straddle tiles, a bank of 64-token images (the 16-lane merges of the sort), a row bank and a 64-tile bank
TOPT = [
    (523, 4, "f16", 0, 130, 8, 0, 1), (523, 4, "bf16", 1, 300, 1, 7, 2), (523, 4, "f16", 1, 300, 256, 0, 3), (523, 4, "bf16", 0, 130, 8, 0, 4),
    (40, 64, "f16", 1, 300, 8, 3, 1), (40, 64, "bf16", 0, 130, 1, 0, 2), (40, 64, "f16", 0, 130, 8, 0, 15), (40, 64, "bf16", 1, 130, 8, 0, 16),
    (2092, 1, "bf16", 0, 130, 256, 1000, 1), (2092, 1, "f16", 1, 300, 8, 0, 1),
    (1024, 16, "f16", 0, 130, 8, 0, 2), (1024, 16, "bf16", 1, 300, 256, 5, 15), (1024, 16, "f16", 1, 130, 1, 0, 16),
    (1024, 16, "bf16", 0, 130, 8, 0, 1),
]


@pytest.mark.parametrize("c", TOPT, ids=lambda c: "N%d-P%d-%s-lo%d-Q%d-k%d-off%d-t%d" % c)
def test_max_under_top_t_is_bit_exact(c, monkeypatch):
    N, P, dt, lo, Q, k, off, top_t = c
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", str(lo))
    rng = np.random.default_rng(N + P + Q + k + top_t)
    bank, xw = _bank(rng, N, P, dt)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    q[3] = xw[N // 2, P - 1]                                       # a query that is itself a bank row
    w = (rng.random(D, dtype=np.float32) + 0.05) if (N + Q + top_t) % 2 else None
    got, want = _both(q, bank, w, k, "max", off, top_t)
    print(got[2])
    _assert_same(got, want)
    assert want[2]["path"] == "tokens"
    _assert_two_stage(got[2], "max", top_t)
    if top_t == 1:                                                 # a[0]: the query's own image is the best, at distance 0
        assert got[1][3, 0].item() == off + N // 2 and got[0][3, 0].item() == 0.0


@pytest.mark.parametrize("c", [(523, 4, "f16", 2), (40, 64, "bf16", 16), (1024, 16, "f16", 7)], ids=lambda c: "N%d-P%d-%s-t%d" % c)
def test_min_under_top_t_is_the_plain_min(c):
    N, P, dt, top_t = c
    rng = np.random.default_rng(N + top_t)
    bank, _ = _bank(rng, N, P, dt)
    q = rng.standard_normal((130, D)).astype(np.float32)
    got, want = _both(q, bank, None, 8, "min", 0, top_t)
    plain = _search(q, bank, None, 8, "min")
    _assert_same(got, want)
    _assert_same(got, plain)
    _assert_two_stage(got[2], "min", top_t)
    assert plain[2]["path"] == "prefiltered" and "top_t" not in plain[2]


# (N, P, dtype, lo, Q, k, idx_offset, selection, top_t, combine)
SEL = [
    (1024, 16, "f16", 0, 130, 8, 0, "half", None, "max"), (1024, 16, "bf16", 1, 300, 256, 3, "half", 2, "max"),
    (1024, 16, "f16", 1, 130, 1, 0, "all", 15, "max"), (1024, 16, "bf16", 0, 130, 8, 0, "half", None, "min"),
    (5120, 16, "f16", 0, 130, 8, 0, "runs10", None, "max"), (5120, 16, "bf16", 1, 130, 8, 9, "runs10", 4, "max"),
    (5120, 16, "f16", 1, 130, 256, 0, "runs10", None, "min"),
    (523, 4, "bf16", 0, 130, 8, 7, "all", 3, "max"), (2092, 1, "f16", 1, 300, 8, 0, "all", None, "min"),
    (40, 64, "bf16", 1, 130, 8, 0, "all", 2, "max"), (40, 64, "f16", 0, 130, 1, 0, "most", 15, "max"),
]


@pytest.mark.parametrize("c", SEL, ids=lambda c: "N%d-P%d-%s-lo%d-Q%d-k%d-off%d-%s-t%s-%s" % c)
def test_under_a_selection_is_bit_exact(c, monkeypatch):
    N, P, dt, lo, Q, k, off, kind, top_t, combine = c
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", str(lo))
    rng = np.random.default_rng(N + P + Q + k)
    flags = _flags(kind, N, P, rng)
    assert ref.select_route_takes(flags, P, k), (int(flags.sum()), ref.live_tiles(flags, P)[3])
    if kind == "runs10":
        assert abs(flags.mean() - 0.10) < 0.005 and len(ref.live_tiles(flags, P)[0]) == 32
    bank, xw = _bank(rng, N, P, dt)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    w = (rng.random(D, dtype=np.float32) + 0.05) if (N + Q) % 2 else None
    got, want = _both(q, bank, w, k, combine, off, top_t, flags)
    print(got[2])
    _assert_same(got, want)
    assert want[2]["path"] == "tokens"
    _assert_two_stage(got[2], combine, top_t, flags, P, N)
    ids = got[1].cpu().numpy()
    assert flags[ids[ids >= 0] - off].all()                        # only selected images are returned


def test_selections_below_the_limits_take_the_grouped_route():
    """10 % of (1024, 16) in runs of whole tiles is 6 tiles, 1536 rows: below 2048 rows, served whole by the grouped route; so is a
    selection of fewer than k images, which leaves a (+inf, -1) tail."""
    rng = np.random.default_rng(41)
    N, P, Q = 1024, 16, 40
    bank, _ = _bank(rng, N, P, "f16")
    q = rng.standard_normal((Q, D)).astype(np.float32)
    flags = np.zeros(N, bool)
    flags[5 * 16:8 * 16] = flags[30 * 16:33 * 16] = True
    assert not ref.select_route_takes(flags, P, 8) and ref.live_tiles(flags, P)[3] == 6
    got, want = _both(q, bank, None, 8, "max", 0, 2, flags)
    _assert_same(got, want)
    assert got[2]["path"] == "tokens" and got[2]["selected"] == 96, got[2]
    few = np.zeros(N, bool)
    few[rng.choice(N, 20, replace=False)] = True
    got, want = _both(q, bank, None, 30, "max", 0, None, few)
    _assert_same(got, want)
    assert got[2]["path"] == "tokens"
    assert (got[1][:, 20:] == -1).all() and torch.isinf(got[0][:, 20:]).all() and (got[1][:, :20] >= 0).all()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("combine,top_t", [("max", 3), ("max", None), ("min", None)])
def test_deselected_garbage_changes_no_bit(dt, combine, top_t):
    """Deselected images filled with NaN, inf and 6e4: the result under the selection is that of the clean bank, bit for bit."""
    rng = np.random.default_rng(43)
    N, P, Q, k = 1024, 16, 130, 8
    flags = _flags("half", N, P, rng)
    x = (rng.standard_normal((N, 1, D)) + 0.7 * rng.standard_normal((N, P, D))).astype(np.float32)
    dirty = x.copy()
    off = np.nonzero(~flags)[0]
    dirty[off[0::3]] = np.nan
    dirty[off[1::3]] = np.inf
    dirty[off[2::3]] = 6e4
    q = rng.standard_normal((Q, D)).astype(np.float32)
    clean = _search(q, _to16(x, dt)[0], None, k, combine, 0, top_t, flags)
    got, want = _both(q, _to16(dirty, dt)[0], None, k, combine, 0, top_t, flags)
    _assert_same(got, want)
    _assert_same(got, clean)
    _assert_two_stage(got[2], combine, top_t, flags, P, N)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_hostile_selected_images_are_decided_by_stage_2(dt):
    """Selected images with an inf element (an unboundable row), with fewer than top_t finite token distances, with duplicated
    tokens, and duplicated images (ties to the lower image)."""
    rng = np.random.default_rng(47)
    N, P, Q, k, top_t = 1024, 16, 130, 12, 3
    flags = _flags("half", N, P, rng)
    flags[100:110] = True
    flags[200:206] = True
    x = (rng.standard_normal((N, 1, D)) + 0.7 * rng.standard_normal((N, P, D))).astype(np.float32)
    x[100, 5, 7] = np.inf                                          # one unboundable row: 15 finite token distances
    x[101, :14] = np.nan                                           # two finite token distances: never returned under top_t = 3
    x[102, :13] = np.nan                                           # three: a[2] is finite
    x[103] = np.nan
    x[104, 1:4] = x[104, 0]                                        # duplicated tokens: a[0] = a[1] = a[2] = a[3]
    x[200:206] = x[105]                                            # six copies of image 105
    bank, xw = _to16(x, dt)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    q[5], q[6], q[7], q[8] = xw[100, 2], xw[102, 15], xw[104, 0], xw[105, 9]
    for combine, t in (("max", top_t), ("max", None), ("min", None)):
        got, want = _both(q, bank, None, k, combine, 0, t, flags)
        _assert_same(got, want)
        assert got[2]["path"] == "prefiltered", got[2]
        ids = got[1].flatten().tolist()
        assert 103 not in ids
        if combine == "max" and t:
            assert 101 not in ids
            assert got[1][5, 0].item() == 100 and got[0][5, 0].item() >= 0.0     # a[2] of the image with the inf row is finite
            assert got[1][7, 0].item() == 104 and got[0][7, 0].item() == 0.0    # the duplicated token three times over: a[2] = 0
        if combine == "max" and not t:
            assert 100 not in ids and 101 not in ids and 102 not in ids          # an infinite token distance: the plain max is +inf
        if combine == "min":
            assert got[1][5, 0].item() == 100 and got[0][5, 0].item() == 0.0
            assert got[1][8].tolist()[:7] == [105, 200, 201, 202, 203, 204, 205]  # ties: the lower image first


def test_a_negative_weight_sends_every_query_back():
    rng = np.random.default_rng(29)
    N, P, Q, k = 1024, 16, 40, 5
    bank, _ = _bank(rng, N, P, "f16")
    flags = _flags("half", N, P, rng)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    w = rng.random(D, dtype=np.float32) + 0.5
    w[9] = -0.25
    got, want = _both(q, bank, w, k, "max", 0, 2, flags)
    _assert_same(got, want)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] == Q, got[2]


def test_the_selection_follows_the_weights():
    """The masked constants are kept per (bank, c): the same Selection and bank searched under other weights are rebuilt, and a
    second search under the same weights reuses them."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(53)
    N, P, Q, k = 1024, 16, 40, 5
    bank, _ = _bank(rng, N, P, "bf16")
    flags = _flags("half", N, P, rng)
    xd = bank.cuda()
    qd = torch.from_numpy(rng.standard_normal((Q, D)).astype(np.float32)).cuda()
    w1, w2 = (torch.from_numpy(rng.random(D, dtype=np.float32) + 0.05).cuda() for _ in range(2))
    tb, plain = search.TokenBank.resident(xd, w1), search.TokenBank(xd, w1)
    sel = search.Selection(torch.from_numpy(flags), xd.device).prepare_mse(tb)
    assert sel._mse[tb] is None                                    # asked, nothing built yet
    for w in (w1, w1, w2):
        tb.set_weights(w)
        plain.set_weights(w)
        before = sel._mse[tb]
        st = {}
        got = search.distance_topk_tokens(qd, tb, k, "MSE", "max", stats=st, select=sel)
        want = search.distance_topk_tokens(qd, plain, k, "MSE", "max", select=search.Selection(torch.from_numpy(flags), xd.device))
        _assert_same((*got, st), want)
        assert st["path"] == "prefiltered"
        if w is w1 and before is not None:
            assert sel._mse[tb] is before                          # the same c: kept
        if w is w2:
            assert sel._mse[tb] is not before and sel._mse[tb][0] is tb.stage1_mse(search.prepare_distance_weights(w, D, xd.device))[1]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("combine,top_t", [("max", 1), ("max", 2), ("max", 3), ("max", 4), ("min", 2)])
def test_d160_against_the_contract(dt, combine, top_t, monkeypatch):
    """D = 160 (five 32-element k-steps; the 16 partials hold unequal numbers of terms): the _top and _top_sel entries against NumPy,
    with idx_offset != 0."""
    from sky_embeddings_amd import ops, search
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", "1" if dt == "f16" else "0")
    rng = np.random.default_rng(160)
    N, P, d, Q, k, off = 523, 4, 160, 130, 8, 11
    bank, xw = _bank(rng, N, P, dt, d)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    cd = (torch.from_numpy(rng.random(d, dtype=np.float32) + 0.05).cuda())
    cd = (cd / cd.sum()).contiguous()
    xd, qd = bank.cuda(), torch.from_numpy(q).cuda()
    tail, rowp = ops.token_mse_rowp(xd, cd)
    a = mpr.contract_distances(cd.cpu().numpy(), q, xw.reshape(N * P, d)).reshape(Q, N, P)
    flags = rng.random(N) < 0.5
    code = ops.COMBINE_CODES[combine]

    def run(launch):
        out_s, out_i = torch.empty(Q, k, device="cuda"), torch.empty(Q, k, device="cuda", dtype=torch.int64)
        redo = torch.empty(Q, device="cuda", dtype=torch.int32)
        launch(out_s, out_i, redo)
        assert int(redo.sum()) == 0
        return (-out_s).cpu().numpy(), out_i.cpu().numpy()

    for fl in (None, flags):
        if fl is None:
            s, i = run(lambda *out: ops.distance_topk_tokens_prefiltered_top(cd, qd, xd, tail, rowp, k, code, top_t, off, *out))
        else:
            sel = search.Selection(torch.from_numpy(fl), xd.device)
            prepared = ops.token_prefilter_select_prepare(sel.words, N, P, rowp)
            tiles, cum, last_live, _ = ref.live_tiles(fl, P)
            assert prepared[2] == len(tiles) and prepared[3] == int(last_live) and prepared[4] == cum.tolist()
            assert prepared[1][:len(tiles)].tolist() == tiles.tolist()
            s, i = run(lambda *out: ops.distance_topk_tokens_prefiltered_top_sel(cd, qd, xd, tail, prepared, ref.direct_end(cum, k), k, code,
                                                                                 top_t, off, *out))
        rs, ri = tdr.topk_of_token_distances(a, k, combine, top_t, fl, idx_offset=off)
        assert np.array_equal(i, ri), (fl is not None)
        assert np.array_equal(s.view(np.uint32), rs.view(np.uint32))
        ms, mi = ref.topk(a, k, combine, top_t, fl, off)               # ... and the rules as this suite restates them
        assert np.array_equal(mi, ri) and np.array_equal(ms.view(np.uint32), rs.view(np.uint32))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_masked_constants_of_the_mse_rows(dt):
    """skyemb_token_prefilter_select_prepare over the MSE row constants: a selected image's rows keep theirs bit for bit -- the
    unboundable {0, inf, 1, 0} included --, every row of a deselected image and every padding row holds {0, NaN, 0, 0}, also where
    rowp held the unboundable constant."""
    from sky_embeddings_amd import ops, search
    rng = np.random.default_rng(59)
    N, P = 523, 4
    x = rng.standard_normal((N, P, D)).astype(np.float32)
    flags = rng.random(N) < 0.5
    flags[[3, 4]] = True, False
    x[3, 1, 5] = np.inf                                            # unboundable, selected
    x[4, 2, 7] = np.inf                                            # unboundable, deselected
    xd = _to16(x, dt)[0].cuda()
    c = search.prepare_distance_weights(None, D, xd.device)
    rowp = ops.token_mse_rowp(xd, c)[1]
    sel = search.Selection(torch.from_numpy(flags), xd.device)
    masked = ops.token_prefilter_select_prepare(sel.words, N, P, rowp)[0].cpu().numpy()
    rp = rowp.cpu().numpy()
    on = np.zeros(masked.shape[0], bool)
    on[:N * P] = np.repeat(flags, P)
    assert np.array_equal(masked[on].view(np.uint32), rp[on].view(np.uint32))
    assert np.isinf(rp[3 * P + 1, 1]) and np.isinf(masked[3 * P + 1, 1]) and np.isinf(rp[4 * P + 2, 1])
    assert np.isnan(masked[~on, 1]).all() and (masked[~on][:, [0, 2, 3]] == 0).all()
