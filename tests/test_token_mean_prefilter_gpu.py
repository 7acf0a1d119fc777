"""GPU: the two-stage token search under combine 'mean' (cosine_topk_tokens over TokenBank.resident) is bit for bit the grouped
route, stage by stage what tests/token_mean_prefilter_reference.py states, and everything it leaves out stays where it was."""
import functools

import numpy as np
import pytest
import torch

from sky_embeddings_amd import ops, search
from tests import prefilter_gpu_harness as h
from tests import prefilter_stage1_reference as sr
from tests import token_mean_prefilter_reference as mr
from tests import token_prefilter_stage_reference as stage
from tests import token_search_reference as tsr

pytestmark = pytest.mark.gpu
T16 = h.TORCH16
N_TAIL = 2048 + 37


@functools.lru_cache(maxsize=4)
def random_case(fmt, N, P, D, Q=257, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * P + D)
    bank = torch.randn(N, P, D, generator=g).to(T16[fmt]).to(h.DEV)
    q = torch.randn(Q, D, generator=g).to(h.DEV)
    w = (torch.rand(D, generator=g) + 0.1).to(h.DEV)
    return bank, q, w


def both(q, bank, k, w=None, idx_offset=0, eps=1e-6, **kw):
    """(two-stage result and stats, grouped result) over the same bank."""
    st = {}
    got = search.cosine_topk_tokens(q, search.TokenBank.resident(bank, w, idx_offset), k, "mean", eps=eps, stats=st, **kw)
    ref_st = {}
    want = search.cosine_topk_tokens(q, search.TokenBank(bank, w, idx_offset), k, "mean", eps=eps, stats=ref_st, **kw)
    assert ref_st["path"] == "tokens"
    return got, st, want


def assert_equal(got, want):
    assert torch.equal(got[1], want[1]), "image indices differ from the grouped route"
    assert torch.equal(got[0], want[0]), "scores differ from the grouped route"


def abi_search(bank, q, w, k, eps=1e-6):
    """The route through the library calls alone, without a floor: (scores, indices, redo) as numpy.  For shapes the grouped
    kernels do not take (D % 64 != 0), where the public function has no route to compare with."""
    tb = search.TokenBank(bank, w)
    tw, qn = search.prepare_queries(q, tb.weights)
    pooled, tail, rowp = ops.token_mean_pool(bank, tb.norms)
    Q = q.shape[0]
    out_s = torch.empty(Q, k, device=h.DEV)
    out_i = torch.empty(Q, k, device=h.DEV, dtype=torch.int64)
    redo = torch.empty(Q, device=h.DEV, dtype=torch.int32)
    ops.cosine_topk_tokens_mean_prefiltered(tw, qn, bank, tb.norms, pooled, tail, rowp, k, eps, 0, out_s, out_i, redo)
    return out_s.cpu().numpy(), out_i.cpu().numpy(), redo.cpu().numpy()


def no_staging_list_fills(bank, q, w, fmt, k, lo=True, eps=1e-6, contract=None):
    """The CPU statement of stage 1 at these inputs: under the loosest threshold a staged slice can meet no item of 256 / 128
    queries x 256 images passes more than the 2048 pairs its staging list holds, and N fits a candidate list.  That threshold is
    the bootstrap floor, or -- `contract` [Q, N], a search without a floor -- the k-th best contract mean of the first slice."""
    N, P, D = bank.shape
    tb = search.TokenBank(bank, w)
    tw, qn = search.prepare_queries(q, tb.weights)
    if contract is None:
        rq = search._token_request("cosine_topk_tokens", q, tb, k, "mean", search._COSINE, None, None, None)
        floor = search._bootstrap_floor(rq, tw, qn, eps).cpu().numpy()
    else:
        first = stage.token_schedule(N, 1, k)["direct_end"] * 256         # images of the direct-append slice (rows = images)
        floor = -np.sort(-contract[:, :first], axis=1)[:, k - 1]
    pref = mr.pool(bank.float().cpu().numpy(), tb.norms.cpu().numpy(), fmt)
    qref = mr.query_side(tw.cpu().numpy(), qn.cpu().numpy(), fmt, D, lo, eps)
    ok = mr.passes(mr.dot_hat(qref, pref), qref, mr.model_rowp(pref), floor)
    QT = sr.qtile(lo)
    worst = max(int(ok[a:a + QT, b:b + 256].sum()) for a in range(0, ok.shape[0], QT) for b in range(0, N, 256))
    return worst <= sr.SCAP and mr.staged_worst(N, q.shape[0], k), worst


@pytest.mark.parametrize("fmt", ("fp16", "bf16"))
@pytest.mark.parametrize("P", (1, 4, 16, 64))
@pytest.mark.parametrize("D", (128, 160))
def test_bit_equal_to_the_grouped_route(monkeypatch, fmt, P, D):
    monkeypatch.setattr(search, "TOKEN_MEAN_PREFILTER_MIN_Q", 17)
    bank, q, w = random_case(fmt, N_TAIL, P, D)
    if D % 64:
        # the grouped kernels take D % 64 == 0 only, so no grouped route exists at D = 160: the route runs through the library calls
        # and is held to the contract the grouped route is itself pinned to bit for bit (tests/token_search_reference.py)
        sc = tsr.combined_scores(q.cpu().numpy(), bank.float().cpu().numpy(), "mean", w.cpu().numpy())
        fits, worst = no_staging_list_fills(bank, q, w, fmt, 1, contract=sc)
        assert fits, f"the CPU statement lets a staging list fill ({worst} pairs in one item): pick other inputs"
        for k in (1, 100, 256):
            want_s, want_i = tsr.topk_of_scores(sc, k)
            got_s, got_i, redo = abi_search(bank, q, w, k)
            assert not redo.any()
            assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s)
        return
    fits, worst = no_staging_list_fills(bank, q, w, fmt, 1)
    assert fits, f"the CPU statement lets a staging list fill ({worst} pairs in one item): pick other inputs"
    for k in (1, 100, 256):
        got, st, want = both(q, bank, k, w)
        assert st["path"] == "prefiltered" and st["combine"] == "mean" and st["redone"] == 0, st
        assert_equal(got, want)


def test_bit_equal_at_the_flagship_width(monkeypatch):
    monkeypatch.setattr(search, "TOKEN_MEAN_PREFILTER_MIN_Q", 17)
    for fmt in ("fp16", "bf16"):
        bank, q, w = random_case(fmt, 2048, 64, 768, Q=257)
        got, st, want = both(q, bank, 100, w)
        assert st["path"] == "prefiltered" and st["redone"] == 0, st
        assert_equal(got, want)


@pytest.mark.parametrize("fmt", ("fp16", "bf16"))
def test_boundaries(monkeypatch, fmt):
    monkeypatch.setattr(search, "TOKEN_MEAN_PREFILTER_MIN_Q", 17)
    P, D, Q = 4, 128, 40
    g = torch.Generator().manual_seed(3)
    base = torch.randn(300, P, D, generator=g).to(T16[fmt])
    # duplicated images: every image of the first 300 comes back at 300 + i, 600 + i, ...: exact ties at every place
    bank = base.repeat(7, 1, 1)[:N_TAIL].contiguous().to(h.DEV)
    q = (base[:Q, 0].float() + 0.5 * torch.randn(Q, D, generator=g)).to(h.DEV)
    for k in (1, 7, 100):
        got, st, want = both(q, bank, k)
        assert st["path"] == "prefiltered"
        assert_equal(got, want)
    # one ulp either side of the k-th best: images whose last token is nudged by one 16-bit ulp in a few elements
    near = base.clone()
    bits = near.view(torch.int16)
    bits[100:200, P - 1, ::7] += 1
    bits[200:300, P - 1, ::5] -= 1
    bank2 = torch.cat([base, near] * 4)[:N_TAIL].contiguous().to(h.DEV)
    for k in (50, 256):
        got, st, want = both(q, bank2, k, idx_offset=12345)
        assert_equal(got, want)
        assert int(got[1].min()) >= 12345
    # k = N cannot reach the route (k <= 256 < 2048 <= N): the library says so, and the largest k over the smallest bank is served
    assert "k <= 256" in ops.token_mean_prefilter_refusal(40, 2048, 1, 128, 2048)
    small, qs, w = random_case(fmt, 2048, 1, 128, Q=40)
    got, st, want = both(qs, small, 256, w)
    assert st["path"] == "prefiltered"
    assert_equal(got, want)


@pytest.mark.parametrize("fmt", ("fp16", "bf16"))
def test_unboundable_and_degenerate_images(monkeypatch, fmt):
    monkeypatch.setattr(search, "TOKEN_MEAN_PREFILTER_MIN_Q", 17)
    P, D, Q, k = 4, 128, 33, 20
    bank, q, w = random_case(fmt, N_TAIL, P, D, Q=Q, seed=9)
    bank, q = bank.clone(), q.clone()
    # planted near the top of query 0 .. 5 (images made of the query itself) and far from every query (left random)
    tops = [10, 11, 12, 13, 14, 15]
    for j, i in enumerate(tops):
        bank[i] = (q[j] / w.sqrt()).to(T16[fmt])[None, :].expand(P, D)
    lows = [500, 501, 502, 503, 504, 505]
    big = 60000.0 if fmt == "fp16" else 2.0 ** 121
    tiny = 2.0 ** -24 if fmt == "fp16" else 2.0 ** -70
    for a, b in zip(tops, lows):
        for i in (a, b):
            kind = tops.index(a)
            if kind == 0:
                bank[i, 1, 3] = float("nan")
            elif kind == 1:
                bank[i, 2, 5] = float("inf")
            elif kind == 2:
                bank[i, 0] = 0
            elif kind == 3:
                bank[i, 3, 7] = tiny
            elif kind == 4:
                bank[i, 1, 9] = big
            else:
                bank[i, :, :] = bank[i, :, :] * 0 + tiny
    q[Q - 1] = 0                                                   # an all-zero query
    pool = ops.token_mean_pool(bank, search.TokenBank(bank, w).norms)
    rowp = pool[2].cpu().numpy()
    for i in (10, 11, 12, 500, 501, 502):
        assert (rowp[i] == np.array([0, np.inf, 1, 0], np.float32)).all(), i
    got, st, want = both(q, bank, k, w)
    assert st["path"] == "prefiltered" and st["redone"] >= 1     # the zero query at least
    assert_equal(got, want)
    assert 10 not in got[1][0].tolist()                            # the NaN image scores -inf: never returned
    assert 12 in got[1][2].tolist()                                # the image with an all-zero token is still among query 2's best


@pytest.mark.parametrize("fmt", ("fp16", "bf16"))
def test_forced_rerun(monkeypatch, fmt):
    monkeypatch.setattr(search, "TOKEN_MEAN_PREFILTER_MIN_Q", 17)
    P, D, Q = 4, 128, 40
    g = torch.Generator().manual_seed(4)
    one = torch.randn(1, P, D, generator=g).to(T16[fmt])
    bank = one.repeat(4352, 1, 1).contiguous().to(h.DEV)           # identical images: every pair passes, every staging list fills
    q = torch.randn(Q, D, generator=g).to(h.DEV)
    got, st, want = both(q, bank, 10)
    assert st["path"] == "prefiltered" and st["redone"] > 0, st
    assert_equal(got, want)


@pytest.mark.parametrize("fmt", ("fp16", "bf16"))
@pytest.mark.parametrize("P,D", ((4, 128), (64, 160)))
def test_pooled_image_and_constants(fmt, P, D):
    """skyemb_token_mean_pool through the C ABI into guarded buffers, against the statement: the 16-bit rows exact, the fp32 value
    they round inside error term (c), the constants inside the stated interval, sentinels, tail tile, no write outside."""
    N = 256 + 37
    bank, _, w = random_case(fmt, N, P, D, Q=8, seed=21)
    bank = bank.clone()
    bank[5, 1, 2] = float("nan")
    bank[7, 0] = 0
    bank[9] *= 2.0 ** -8
    bank[11, ::2] *= -1                                            # heavy cancellation
    tb = search.TokenBank(bank, w)
    L = ops.lib()
    rows = L.skyemb_bank16_rowp_rows(N)
    pooled, rowp, tail = h.Guarded(N * D * 2), h.Guarded(rows * 16), h.Guarded(256 * D * 2)
    rc = L.skyemb_token_mean_pool(h.ptr(bank), ops.dtype_code(T16[fmt]), h.ptr(tb.norms), N, P, D, pooled.ptr(), rowp.ptr(), tail.ptr(), h.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.skyemb_last_error()
    assert pooled.intact() and rowp.intact() and tail.intact()
    x, xn = bank.float().cpu().numpy(), tb.norms.cpu().numpy()
    ref = mr.pool(x, xn, fmt)
    assert ref["unboundable"][[5, 7]].all() and ref["unboundable"].sum() == 2
    bits = pooled.np(np.uint16, N, D)
    mr.check_pool(bits, rowp.np(np.float32, rows, 4), ref)
    mr.check_error_c(x, xn, ref)
    t = tail.np(np.uint16, 256, D)
    assert (t[:37] == bits[256:]).all() and (t[37:] == 0).all()


def test_everything_else_stays_on_the_grouped_route(monkeypatch):
    monkeypatch.setattr(search, "TOKEN_MEAN_PREFILTER_MIN_Q", 17)
    bank, q, w = random_case("fp16", N_TAIL, 4, 128, Q=40)
    tb = search.TokenBank.resident(bank, w)
    plain = search.TokenBank(bank, w)
    flags = torch.rand(N_TAIL, device=h.DEV) < 0.5
    W = (torch.rand(40, 128, device=h.DEV) + 0.1)
    for kw in (dict(select=flags), dict(top_t=2), dict(weights=W)):
        st = {}
        got = search.cosine_topk_tokens(q, tb, 10, "mean", stats=st, **kw)
        assert st["path"] == "tokens", kw
        assert_equal(got, search.cosine_topk_tokens(q, plain, 10, "mean", **kw))
    st = {}
    got = search.cosine_topk_tokens(q, search.TokenBank(bank.float(), w), 10, "mean", stats=st)
    assert st["path"] == "tokens"
    assert_equal(got, search.cosine_topk_tokens(q, plain, 10, "mean"))
    st = {}
    got = search.cosine_topk_tokens(q[:16], tb, 10, "mean", stats=st)
    assert st["path"] == "tokens"
    assert_equal(got, search.cosine_topk_tokens(q[:16], plain, 10, "mean"))
    assert tb._stage1_mean is None                                 # nothing was pooled for any of them


def test_weights_change_rebuilds_the_pooled_image(monkeypatch):
    monkeypatch.setattr(search, "TOKEN_MEAN_PREFILTER_MIN_Q", 17)
    bank, q, w = random_case("bf16", N_TAIL, 4, 128, Q=40)
    tb = search.TokenBank.resident(bank, w)
    st = {}
    first = search.cosine_topk_tokens(q, tb, 10, "mean", stats=st)
    assert st["path"] == "prefiltered" and tb._stage1_mean is not None
    kept = tb._stage1_mean
    assert search.cosine_topk_tokens(q, tb, 10, "mean")[1].equal(first[1]) and tb._stage1_mean is kept
    w2 = torch.rand(128, device=h.DEV) + 0.1
    tb.set_weights(w2)
    assert tb._stage1_mean is None
    got = search.cosine_topk_tokens(q, tb, 10, "mean", stats=st)
    assert st["path"] == "prefiltered" and tb._stage1_mean is not kept
    assert_equal(got, search.cosine_topk_tokens(q, search.TokenBank.resident(bank, w2), 10, "mean"))
    assert_equal(got, search.cosine_topk_tokens(q, search.TokenBank(bank, w2), 10, "mean"))
