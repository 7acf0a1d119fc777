"""GPU: the two-stage many-query search over a resident 16-bit patch-token bank -- ``cosine_topk_tokens(queries,
TokenBank.resident(bank), k, combine)`` with combine 'min' | 'max'.

The reference of every case is the same call over the same device bank in a plain ``TokenBank`` (the grouped route); scores and
indices must be bit-equal.  One case is also compared with ``tests/token_search_reference.topk_tokens`` on the widened bank."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import token_prefilter_reference as tpr
from tests import token_search_reference as tsr


@pytest.fixture(autouse=True)
def _min_q(monkeypatch):
    from sky_embeddings_amd import search
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 17)


def _both(q, bank, w, k, combine, idx_offset=0, **kw):
    """((scores, indices, stats) of the resident bank, (scores, indices, stats) of the plain one); bank: a 16-bit tensor."""
    from sky_embeddings_amd import search
    qd, xd = torch.from_numpy(q).cuda(), bank.cuda()
    wd = None if w is None else torch.from_numpy(w).cuda()
    out = []
    for tb in (search.TokenBank.resident(xd, wd, idx_offset), search.TokenBank(xd, wd, idx_offset)):
        stats = {}
        s, i = search.cosine_topk_tokens(qd, tb, k, combine, stats=stats, **kw)
        out.append((s, i, stats))
    return out


def _assert_same(got, ref):
    assert torch.equal(got[1], ref[1]), (got[2], torch.nonzero(got[1] != ref[1])[:5].tolist())
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)), got[2]


@pytest.mark.parametrize("c", tpr.CASES, ids=tpr.case_id)
def test_two_stage_token_topk_is_bit_exact(c, monkeypatch):
    """fp16 and bf16, min and max, one and two query passes, every P dividing 64; N P just above 2048 rows with tails of none, one
    image and 256 - P rows; Q in {17, 130, 257}; k in {1, 7, 100, 150}; weighted and not; idx_offset; planted exact ties.  The cap on
    re-run queries is a condition: in the numpy restatement (tests/test_token_prefilter_cpu.py) no query of these cases fills a
    list or a staging region -- a slice's candidates number at most the bank's images, 32 .. 2303 here, against lists of 4096
    (k <= 128) or 8192, and the staged items stay below their 2048 slots."""
    P, combine, dt, lo, Q, tail, D, k, weighted, off = c
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", "1" if lo else "0")
    q, bank, xw, w = tpr.case_inputs(P, tail, D, Q, weighted, dt)
    got, ref = _both(q, bank, w, k, combine, off)
    print(got[2])
    _assert_same(got, ref)
    assert ref[2]["path"] == "tokens"
    assert got[2]["path"] == "prefiltered" and got[2]["combine"] == combine and got[2]["redone"] <= Q // 10, got[2]
    if D == 768:                                                   # ... and against the numpy oracle on the widened bank
        rs, ri = tsr.topk_tokens(q, xw, k, combine, w, idx_offset=off)
        assert np.array_equal(got[1].cpu().numpy(), ri) and np.array_equal(got[0].cpu().numpy().view(np.uint32), rs.view(np.uint32))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("combine", ["min", "max"])
def test_hostile_rows_are_decided_exactly(dt, combine):
    """One NaN token in an image (-inf under min, ignored under max), an all-NaN image, an inf element, a zero row, a zero query, an
    image whose tokens are copies of query 5's best token; bf16: a row outside the [2^-60, 2^120) window and a query outside the
    scale window."""
    rng = np.random.default_rng(11)
    N, P, D, Q, k = 640, 4, 128, 40, 12
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = (rng.standard_normal((N, 1, D)) + 0.7 * rng.standard_normal((N, P, D))).astype(np.float32)
    x[10, 2] = np.nan
    x[11] = np.nan
    x[12, 1, 7] = np.inf
    x[13, 3] = 0.0
    q[20] = 0.0
    sc = tsr.token_scores(q[5:6], x)[0]
    x[14, :] = x.reshape(N * P, D)[int(np.argmax(sc))]
    if dt == "bf16":
        x[15, 0] = 1e-30 * np.sign(q[0])
        x[16, 1, 3] = 1e+37
        q[21] *= 1e-20
    bank, xw = tpr.to16(x, tpr.DTYPES[dt])
    got, ref = _both(q, bank, None, k, combine)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered", got[2]
    i5 = got[1][5].tolist()
    assert 14 in i5[:3]
    flat = got[1].flatten().tolist()
    assert 11 not in flat and ((10 not in flat) if combine == "min" else True)
    assert got[2]["redone"] >= 1                                   # the zero query is outside what stage 1 bounds


def test_more_near_duplicates_than_a_list_holds():
    """10 000 images that are copies of query 3 (5000 of them in the last slice): more candidates than the 4096-entry list.  The query is flagged, re-run
    by the grouped route, and the result is still bit-equal (ties to the lower image)."""
    rng = np.random.default_rng(13)
    N, P, D, Q, k = 12000, 2, 128, 20, 9
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = rng.standard_normal((N, P, D), dtype=np.float32)
    x[1000:11000] = q[3]
    bank, _ = tpr.to16(x, torch.float16)
    got, ref = _both(q, bank, None, k, "min")
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] >= 1, got[2]
    assert got[1][3].tolist() == list(range(1000, 1000 + k))


def test_everything_else_takes_the_grouped_route(monkeypatch):
    """mean, top_t, select, [Q, D] weights, P = 48, Q = 16 and the switch off, each on a TokenBank.resident: path 'tokens' and the
    plain bank's result."""
    rng = np.random.default_rng(17)
    N, P, D, Q, k = 700, 4, 128, 24, 5
    q = rng.standard_normal((Q, D), dtype=np.float32)
    bank, _ = tpr.to16(rng.standard_normal((N, P, D)), torch.float16)
    flags = torch.from_numpy(rng.random(N) < 0.5)
    wq = torch.from_numpy(rng.random((Q, D), dtype=np.float32) + 0.1).cuda()
    for combine, kw in (("mean", {}), ("min", dict(top_t=2)), ("max", dict(select=flags)), ("min", dict(weights=wq))):
        got, ref = _both(q, bank, None, k, combine, **kw)
        _assert_same(got, ref)
        assert got[2]["path"] == "tokens", (combine, kw.keys(), got[2])
    got, ref = _both(q[:16], bank, None, k, "min")
    _assert_same(got, ref)
    assert got[2]["path"] == "tokens"
    bank48, _ = tpr.to16(rng.standard_normal((64, 48, D)), torch.bfloat16)
    got, ref = _both(q, bank48, None, k, "max")
    _assert_same(got, ref)
    assert got[2]["path"] == "tokens"
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    got, ref = _both(q, bank, None, k, "min")
    _assert_same(got, ref)
    assert got[2]["path"] == "tokens"
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER")
    got, ref = _both(q, bank, None, k, "min")
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered"


def test_set_weights_rebuilds_the_stage1_constants():
    from sky_embeddings_amd import search
    rng = np.random.default_rng(19)
    N, P, D, Q, k = 600, 4, 128, 33, 10
    qd = torch.from_numpy(rng.standard_normal((Q, D), dtype=np.float32)).cuda()
    bank, _ = tpr.to16(rng.standard_normal((N, P, D)), torch.bfloat16)
    xd = bank.cuda()
    w1 = torch.from_numpy(rng.random(D, dtype=np.float32) + 0.05).cuda()
    w2 = torch.from_numpy(1.0 / (rng.random(D, dtype=np.float32) + 0.05) ** 2).cuda()
    res, plain = search.TokenBank.resident(xd, w1), search.TokenBank(xd, w1)
    assert type(res) is type(plain) and torch.equal(res.norms, plain.norms) and res.sample(8)[0].dtype == torch.bfloat16
    for w in (None, w2):
        if w is not None:
            before = res.stage1()[1]
            res.set_weights(w)
            plain.set_weights(w)
            assert res._stage1 is None and res.stage1()[1] is not before
        st = {}
        got = search.cosine_topk_tokens(qd, res, k, "max", stats=st)
        ref = search.cosine_topk_tokens(qd, plain, k, "max")
        assert st["path"] == "prefiltered"
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    tail, rowp = res.stage1()                                      # 2400 rows: 16 B per row up to whole tiles, one tail tile
    assert tail.shape == (256, D) and tail.dtype == torch.bfloat16 and rowp.shape == (2560, 4)
