"""GPU: the two-stage many-query search over a resident 16-bit patch-token bank under a selection of images --
``cosine_topk_tokens(queries, TokenBank.resident(bank), k, combine, select=...)``.

The reference of every case is the same call with the same selection over the same device bank in a plain ``TokenBank`` (the
grouped route); scores and indices must be bit-equal.  One case per dtype is also compared with
``tests/token_search_reference.topk_tokens`` on the compacted widened bank."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import token_prefilter_reference as tpr
from tests import token_prefilter_select_reference as tps
from tests import token_search_reference as tsr


@pytest.fixture(autouse=True)
def _min_q(monkeypatch):
    from sky_embeddings_amd import search
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 17)


def _both(q, bank, w, k, combine, select, idx_offset=0):
    """((scores, indices, stats) of the resident bank, the same of the plain one) under ``select`` (bool array, Selection or None)."""
    from sky_embeddings_amd import search
    qd, xd = torch.from_numpy(q).cuda(), bank.cuda()
    wd = None if w is None else torch.from_numpy(w).cuda()
    if isinstance(select, np.ndarray):
        select = search.Selection(torch.from_numpy(select))
    out = []
    for tb in (search.TokenBank.resident(xd, wd, idx_offset), search.TokenBank(xd, wd, idx_offset)):
        stats = {}
        s, i = search.cosine_topk_tokens(qd, tb, k, combine, stats=stats, select=select)
        out.append((s, i, stats))
    return out


def _assert_same(got, ref):
    assert torch.equal(got[1], ref[1]), (got[2], torch.nonzero(got[1] != ref[1])[:5].tolist())
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)), got[2]


@pytest.mark.parametrize("c", tps.CASES, ids=tps.case_id)
def test_two_stage_token_topk_under_a_selection_is_bit_exact(c, monkeypatch):
    """fp16 and bf16, min and max, one and two query passes, P in {1, 4, 16, 32, 64}; N P just above 4096 rows with tails of none,
    one image and 256 - P rows; Q in {17, 130}; k in {1, 7, 100}; weighted and not; idx_offset; selections: all, half, runs of
    whole dead tiles (first and tail tile among them), the tail tile plus eight whole ones, exactly 2048 selected rows.  The cap
    on re-run queries is a condition: in the numpy restatement (tests/test_token_prefilter_select_cpu.py) no query of these cases
    fills a list or a staging region."""
    P, combine, dt, lo, Q, tail, k, weighted, off, kind = c
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", "1" if lo else "0")
    q, bank, xw, w = tps.case_inputs(P, tail, Q, weighted, dt)
    f = tps.case_flags(c)
    got, ref = _both(q, bank, w, k, combine, f, off)
    print(got[2])
    _assert_same(got, ref)
    assert ref[2]["path"] == "tokens"
    assert got[2]["path"] == "prefiltered" and got[2]["combine"] == combine and got[2]["redone"] <= Q // 10, got[2]
    R = xw.shape[0] * P
    _, tiles, cum, last = tps.prepare(np.zeros(((R + 255) // 256 * 256, 4), np.float32), f, P)
    assert got[2]["selected"] == int(f.sum()) and got[2]["tiles"] == (tiles.size, (R + 255) // 256), got[2]
    if kind == "all":                                              # ... and the unselected two-stage search
        und = _both(q, bank, w, k, combine, None, off)[0]
        assert und[2]["path"] == "prefiltered" and "selected" not in und[2]
        _assert_same(got, und)
    if c in tps.ORACLE_CASES:                                      # ... and the numpy oracle on the compacted widened bank
        rs, ri = tps.compacted_topk(q, xw, k, combine, f, w, off)
        assert np.array_equal(got[1].cpu().numpy(), ri) and np.array_equal(got[0].cpu().numpy().view(np.uint32), rs.view(np.uint32))


def test_the_prepared_state_is_the_restatement():
    """Masked constants, live tiles, counts and info of the device against tests/token_prefilter_select_reference.prepare, for
    every P dividing 64 and a bank with a tail."""
    from sky_embeddings_amd import ops, search
    rng = np.random.default_rng(23)
    for P in (1, 2, 4, 8, 16, 32, 64):
        N = (9 * 256 + 64) // P
        x = rng.standard_normal((N, P, 128), dtype=np.float32)
        x[1, 0, 3] = np.inf                                         # unboundable rows, one in a deselected image
        x[N - 1, P - 1, 0] = np.nan
        tb = search.TokenBank.resident(tpr.to16(x, torch.float16)[0].cuda())
        f = rng.random(N) < 0.4
        per_tile = 256 // P
        f[2 * per_tile:4 * per_tile] = False
        f[[1, 0]] = [False, True]
        f[N - 1] = True
        sel = search.Selection(torch.from_numpy(f))
        rowp_sel, tiles, n_live, last_live, cum = sel.token_prefilter(tb)
        assert sel.token_prefilter(tb)[0] is rowp_sel               # cached
        m, rt, rc, rl = tps.prepare(tb.stage1()[1].cpu().numpy(), f, P)
        assert np.array_equal(rowp_sel.cpu().numpy(), m, equal_nan=True)
        assert n_live == rt.size and last_live == rl == 1 and tiles[:n_live].tolist() == rt.tolist() and cum == rc.tolist()
        assert isinstance(cum, list) and 2 not in rt and 3 not in rt


def test_selections_the_route_leaves_to_the_grouped_search():
    """Nothing selected: every entry (-inf, -1), no stage-1 launch; one image short of 2048 selected rows: path 'tokens'."""
    c = next(c for c in tps.CASES if c[0] == 16 and c[9] == "above")
    P, combine, dt, lo, Q, tail, k, weighted, off, kind = c
    q, bank, xw, w = tps.case_inputs(P, tail, Q, weighted, dt)
    N = xw.shape[0]
    got, ref = _both(q, bank, w, k, combine, np.zeros(N, bool), off)
    _assert_same(got, ref)
    assert got[2]["path"] == "tokens" and (got[1] == -1).all() and torch.isneginf(got[0]).all()
    below = tps.selection("below", N, P, tail, k)
    assert below.sum() * P == 2048 - P
    got, ref = _both(q, bank, w, k, combine, below, off)
    _assert_same(got, ref)
    assert got[2]["path"] == "tokens", got[2]
    above = tps.selection("above", N, P, tail, k)
    got, ref = _both(q, bank, w, k, combine, above, off)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered", got[2]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("combine", ["min", "max"])
def test_hostile_rows(dt, combine):
    """NaN, inf, all-NaN, zero and (bf16) out-of-window rows in DESELECTED images change nothing -- the result is that of the
    clean bank, bit for bit; the same rows in selected images are decided as the grouped route decides them."""
    rng = np.random.default_rng(29)
    N, P, D, Q, k = 1280, 4, 128, 40, 12
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = (rng.standard_normal((N, 1, D)) + 0.7 * rng.standard_normal((N, P, D))).astype(np.float32)
    f = rng.random(N) < 0.6
    hostile = np.arange(10, 17)
    y = x.copy()
    y[10, 2] = np.nan
    y[11] = np.nan
    y[12, 1, 7] = np.inf
    y[13, 3] = 0.0
    y[14, :] = np.inf
    if dt == "bf16":
        y[15, 0] = 1e-30 * np.sign(q[0])
        y[16, 1, 3] = 1e+37
    f[hostile] = False
    clean = _both(q, tpr.to16(x, tpr.DTYPES[dt])[0], None, k, combine, f)[0]
    got, ref = _both(q, tpr.to16(y, tpr.DTYPES[dt])[0], None, k, combine, f)
    _assert_same(got, ref)
    _assert_same(got, clean)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] <= Q // 10, got[2]
    f[hostile] = True                                              # ... and selected
    q[20] = 0.0
    got, ref = _both(q, tpr.to16(y, tpr.DTYPES[dt])[0], None, k, combine, f)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] >= 1, got[2]     # the zero query is outside what stage 1 bounds
    flat = got[1].flatten().tolist()
    assert 11 not in flat and ((10 not in flat) if combine == "min" else True)


def test_one_selection_serves_two_banks_and_survives_set_weights():
    from sky_embeddings_amd import search
    rng = np.random.default_rng(31)
    N, P, D, Q, k = 1100, 4, 128, 33, 10
    qd = torch.from_numpy(rng.standard_normal((Q, D), dtype=np.float32)).cuda()
    x = rng.standard_normal((N, P, D), dtype=np.float32)
    w1 = torch.from_numpy(rng.random(D, dtype=np.float32) + 0.05).cuda()
    w2 = torch.from_numpy(1.0 / (rng.random(D, dtype=np.float32) + 0.05) ** 2).cuda()
    sel = search.Selection(torch.from_numpy(rng.random(N) < 0.7))
    banks = {}
    for dtype in (torch.float16, torch.bfloat16):
        xd = tpr.to16(x, dtype)[0].cuda()
        banks[dtype] = (search.TokenBank.resident(xd, w1), search.TokenBank(xd, w1))

    def check(dtype):
        res, plain = banks[dtype]
        st = {}
        got = search.cosine_topk_tokens(qd, res, k, "min", stats=st, select=sel)
        ref = search.cosine_topk_tokens(qd, plain, k, "min", select=sel)
        assert st["path"] == "prefiltered" and st["selected"] == sel.count, st
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1])

    check(torch.float16)
    check(torch.bfloat16)
    check(torch.float16)
    first = {d: sel.token_prefilter(banks[d][0]) for d in banks}
    assert first[torch.float16] is sel.token_prefilter(banks[torch.float16][0]) and first[torch.float16] is not first[torch.bfloat16]
    for tb in banks[torch.bfloat16]:
        tb.set_weights(w2)
    check(torch.bfloat16)
    assert sel.token_prefilter(banks[torch.bfloat16][0]) is not first[torch.bfloat16]        # rebuilt ...
    assert sel.token_prefilter(banks[torch.float16][0]) is first[torch.float16]              # ... and the other bank's kept
    check(torch.float16)


def test_more_near_duplicates_than_a_list_holds_inside_the_selection():
    """14 000 images that are copies of query 3, four in five of them selected (5 600 in the last slice): more candidates than the
    4096-entry list.  The query is flagged, re-run by the grouped route under the selection, and still bit-equal."""
    rng = np.random.default_rng(13)
    N, P, D, Q, k = 16000, 2, 128, 20, 9
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = rng.standard_normal((N, P, D), dtype=np.float32)
    x[1000:15000] = q[3]
    f = np.ones(N, bool)
    f[1000:15000:5] = False
    bank, _ = tpr.to16(x, torch.float16)
    got, ref = _both(q, bank, None, k, "min", f)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] >= 1, got[2]
    assert got[1][3].tolist() == [i for i in range(1000, 1100) if f[i]][:k]
