"""GPU: the top-t patch combine (``top_t``, the reference's n_top_sims) of the patch-token bank search
(search.cosine_token_scores / cosine_topk_tokens, csrc/topk_tokens.hip) against the CPU restatement
tests/token_topt_reference.py, bit for bit (np.array_equal on scores and on indices)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import token_search_reference as tsr
from tests import token_topt_reference as ttr

# P -> the t values: lane groups (2, 4), one full tile (16), the first carry merge (32), three tiles -- an odd tile count, the
# carry merged twice (48), many tiles (256)
TS = {2: (1, 2), 4: (1, 3, 4), 16: (1, 5, 16), 32: (1, 5, 16), 48: (2, 16), 256: (16,)}
DS, QS = (64, 768), (1, 3, 16)
LP = (torch.float16, torch.bfloat16)


def _weights(rng, D):
    w = rng.random(D, dtype=np.float32) + 0.1
    return w / w.sum()


def _cuda(*arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


def _plant(bank):
    """One NaN token, one all-zero token, an image with all tokens equal, an image without a finite token score (short for
    every t) and one with exactly one (short for every t >= 2)."""
    N, P, _ = bank.shape
    equal = N // 4 if N // 4 != N // 3 else N // 3 + 1           # five different images, also at N = 8
    assert len({N // 3, N // 2, equal, N // 5, N - 2}) == 5
    bank[N // 3, P // 2, 5] = np.nan
    bank[N // 2, 0] = 0.0
    bank[equal] = bank[equal, 0]
    bank[N // 5, :, 1] = np.nan
    bank[N - 2, 1:, 2] = np.nan
    return bank


def _check_scores(search, qd, tb, s, P, tag):
    for t in TS[P]:
        for combine in ("min", "mean"):
            got = search.cosine_token_scores(qd, tb, combine, top_t=t).cpu().numpy()
            assert np.array_equal(got, ttr.combine_top(s, combine, t)), tag + (combine, t)
    got = search.cosine_token_scores(qd, tb, "max", top_t=TS[P][-1]).cpu().numpy()                 # max: d[0] for every t
    assert np.array_equal(got, tsr.combine_scores(s, "max")), tag + ("max",)
    if P <= 16:                                                                                    # min at t == P: the plain min
        assert torch.equal(search.cosine_token_scores(qd, tb, "min", top_t=P), search.cosine_token_scores(qd, tb, "min"))


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", sorted(TS))
def test_token_scores_top_t_bit_exact(P, D, Q):
    """N at whole 16-row tiles and whole waves (N * P = 2048 or 2304 rows) and ragged."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(1000 * P + D + Q)
    for N in ({2: 1024, 4: 512, 16: 128, 32: 64, 48: 48, 256: 8}[P], {2: 2005, 4: 1003, 16: 259, 32: 131, 48: 91, 256: 19}[P]):
        bank = _plant(rng.standard_normal((N, P, D), dtype=np.float32))
        q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
        s = tsr.token_scores(q, bank, w)
        assert np.isneginf(s[:, N // 5]).all() and (np.isfinite(s[:, N - 2]).sum(axis=1) == 1).all()
        bd, qd, wd = _cuda(bank, q, w)
        _check_scores(search, qd, search.TokenBank(bd, wd), s, P, (P, D, Q, N))


@pytest.mark.parametrize("dtype", LP)
@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("P", (4, 16, 32))
def test_token_scores_top_t_half_precision_banks(P, Q, dtype):
    """A 16-bit bank gives the restatement's result on the widened bank, bit for bit; top-k too."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(31 * P + Q)
    D = 64
    for N in ({4: 512, 16: 128, 32: 64}[P], {4: 1003, 16: 259, 32: 131}[P]):
        b16 = torch.from_numpy(_plant(rng.standard_normal((N, P, D), dtype=np.float32))).to(dtype)
        q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
        s = tsr.token_scores(q, b16.to(torch.float32).numpy(), w)
        qd, wd = _cuda(q, w)
        tb = search.TokenBank(b16.cuda(), wd)
        _check_scores(search, qd, tb, s, P, (P, Q, N, dtype))
        for combine in ("min", "mean"):
            t = TS[P][1]
            ref_s, ref_i = tsr.topk_of_scores(ttr.combine_top(s, combine, t), 10)
            got_s, got_i = search.cosine_topk_tokens(qd, tb, 10, combine, top_t=t)
            assert np.array_equal(got_i.cpu().numpy(), ref_i) and np.array_equal(got_s.cpu().numpy(), ref_s), (P, Q, N, dtype, combine)


def _planted_bank(rng, N, P, D, q0, w, combine, t):
    """Random tokens with one NaN token and exact duplicate images among the best of query 0 under the top-t score: at the end,
    in the middle and near the start of the bank -- inside and outside a strided sample."""
    bank = rng.standard_normal((N, P, D), dtype=np.float32)
    bank[11, P // 2, 3] = np.nan
    best = np.argsort(-ttr.combined_scores_top(q0, bank, combine, t, w)[0])[:3]
    bank[N - 1] = bank[best[0]]
    bank[N // 2 + 1] = bank[best[1]]
    bank[7] = bank[best[2]]
    return bank


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", sorted(TS))
def test_token_topk_top_t_bit_exact(P, D, Q):
    """The N of test_token_search_gpu.test_token_topk_bit_exact where it has the P (about 24 000 rows otherwise); most waves see
    fewer than k finite images at the larger P."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(77 * P + D + Q)
    N = {2: 12001, 4: 6003, 16: 1501, 32: 751, 48: 501, 256: 301}[P]
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    bank = _planted_bank(rng, N, P, D, q[:1], w, "mean", TS[P][-1])
    s = tsr.token_scores(q, bank, w)
    bd, qd, wd = _cuda(bank, q, w)
    tb = search.TokenBank(bd, wd)
    for t in TS[P]:
        for combine in ("min", "mean"):
            sc = ttr.combine_top(s, combine, t)
            for k in (10, 100):
                ref_s, ref_i = tsr.topk_of_scores(sc, k)
                for prune in (True, False):
                    stats = {}
                    got_s, got_i = search.cosine_topk_tokens(qd, tb, k, combine, prune=prune, stats=stats, top_t=t)
                    assert stats["top_t"] == t and stats["path"] == "tokens"
                    assert np.array_equal(got_i.cpu().numpy(), ref_i), (P, D, Q, combine, t, k, prune)
                    assert np.array_equal(got_s.cpu().numpy(), ref_s), (P, D, Q, combine, t, k, prune)
    ref_s, ref_i = tsr.topk_of_scores(tsr.combine_scores(s, "max"), 10)
    got_s, got_i = search.cosine_topk_tokens(qd, tb, 10, "max", top_t=TS[P][0])
    assert np.array_equal(got_i.cpu().numpy(), ref_i) and np.array_equal(got_s.cpu().numpy(), ref_s)


@pytest.mark.parametrize("P,D,Q,N,k,t", [(4, 64, 1, 20600, 10, 2), (16, 64, 1, 20500, 10, 5)])
def test_token_topk_top_t_with_the_pruning_floor(P, D, Q, N, k, t):
    """Banks of at least 8 x 256 x k images: the floor from the image sample (scored with the same top_t) is used, lies strictly
    below the true k-th best top-t score, and leaves the result unchanged."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(N + P)
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    bank = _planted_bank(rng, N, P, D, q[:1], w, "min", t)
    s = tsr.token_scores(q, bank, w)
    bd, qd, wd = _cuda(bank, q, w)
    tb = search.TokenBank(bd, wd)
    tw, qn = search.prepare_queries(qd, tb.weights)
    for combine in ("min", "mean"):
        ref_s, ref_i = tsr.topk_of_scores(ttr.combine_top(s, combine, t), k)
        floor = search.token_pruning_floor(tw, qn, tb, k, combine, top_t=t)
        assert floor is not None and bool((floor.cpu().numpy() < ref_s[:, k - 1]).all()), (combine, floor, ref_s[:, k - 1])
        for prune in (True, False):
            stats = {}
            got_s, got_i = search.cosine_topk_tokens(qd, tb, k, combine, prune=prune, stats=stats, top_t=t)
            assert stats == dict(path="tokens", groups=1, pruned=prune, top_t=t)
            assert np.array_equal(got_i.cpu().numpy(), ref_i), (combine, prune)
            assert np.array_equal(got_s.cpu().numpy(), ref_s), (combine, prune)


def test_more_than_16_queries_run_in_groups_with_top_t():
    """Q = 20: two groups, and per query the result of a Q = 1 call."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(20)
    Q, N, P, D, k, t = 20, 1501, 16, 64, 10, 5
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    bank = _planted_bank(rng, N, P, D, q[:1], w, "min", t)
    bd, qd, wd = _cuda(bank, q, w)
    tb = search.TokenBank(bd, wd)
    for combine in ("min", "mean"):
        ref_s, ref_i = ttr.topk_tokens_top(q, bank, k, combine, t, w)
        stats = {}
        got_s, got_i = search.cosine_topk_tokens(qd, tb, k, combine, stats=stats, top_t=t)
        assert stats["groups"] == 2 and stats["top_t"] == t
        assert np.array_equal(got_i.cpu().numpy(), ref_i) and np.array_equal(got_s.cpu().numpy(), ref_s), combine
        sc = search.cosine_token_scores(qd, tb, combine, top_t=t)
        assert np.array_equal(sc.cpu().numpy(), ttr.combined_scores_top(q, bank, combine, t, w))
        for j in (0, 15, 16, 19):
            one_s, one_i = search.cosine_topk_tokens(qd[j:j + 1], tb, k, combine, top_t=t)
            assert torch.equal(one_s[0], got_s[j]) and torch.equal(one_i[0], got_i[j])
            assert torch.equal(search.cosine_token_scores(qd[j:j + 1], tb, combine, top_t=t)[0], sc[j])


@pytest.mark.parametrize("dtype", (torch.float32,) + LP)
def test_plain_calls_are_the_existing_calls(dtype):
    """top_t=None is the call without the keyword, and top_t = 0 through the `_top` entry points is the existing entry point of
    that bank type: identical outputs, list for list."""
    from sky_embeddings_amd import ops, search
    from sky_embeddings_amd._lib import lib
    rng = np.random.default_rng(21)
    Q, N, P, D, k = 3, 1501, 16, 64, 10
    bank = torch.from_numpy(_plant(rng.standard_normal((N, P, D), dtype=np.float32))).to(dtype).cuda()
    qd, wd = _cuda(rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D))
    tb = search.TokenBank(bank, wd)
    tw, qn = search.prepare_queries(qd, tb.weights)
    nl = ops.cosine_token_topk_chunks(N, P, Q, D, k)
    code = ops.bank_dtype_code(dtype, "test")
    st = torch.cuda.current_stream().cuda_stream
    for combine in tsr.COMBINES:
        stats = {}
        a = search.cosine_topk_tokens(qd, tb, k, combine)
        b = search.cosine_topk_tokens(qd, tb, k, combine, top_t=None, stats=stats)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and "top_t" not in stats
        assert torch.equal(search.cosine_token_scores(qd, tb, combine), search.cosine_token_scores(qd, tb, combine, top_t=None))
        c = ops.COMBINE_CODES[combine]
        want = torch.full((Q, N), 7.0, device="cuda")
        got = want.clone()
        ops.cosine_token_scores(tw, qn, bank, tb.norms, c, 1e-6, want)
        ops.check(lib().skyemb_cosine_token_scores_top(tw.data_ptr(), qn.data_ptr(), bank.data_ptr(), code, tb.norms.data_ptr(), Q, N, P, D,
                                                       c, 0, 1e-6, got.data_ptr(), st), "skyemb_cosine_token_scores_top")
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        ps, pi = torch.full((Q, nl, k), 7.0, device="cuda"), torch.full((Q, nl, k), 7, device="cuda", dtype=torch.int64)
        ps2, pi2 = ps.clone(), pi.clone()
        ops.cosine_token_topk(tw, qn, bank, tb.norms, k, c, 1e-6, 5, nl, ps, pi)
        ops.check(lib().skyemb_cosine_token_topk_top(tw.data_ptr(), qn.data_ptr(), bank.data_ptr(), code, tb.norms.data_ptr(), Q, N, P, D, k,
                                                     c, 0, 1e-6, 5, nl, None, ps2.data_ptr(), pi2.data_ptr(), st),
                  "skyemb_cosine_token_topk_top")
        assert torch.equal(ps2.view(torch.int32), ps.view(torch.int32)) and torch.equal(pi2, pi)


def test_top_t_out_of_range_raises_before_any_launch():
    from sky_embeddings_amd import search
    q = torch.randn(2, 64, device="cuda")
    tb = search.TokenBank(torch.randn(50, 4, 64, device="cuda"))
    for t in (0, -1, 5, 17):
        with pytest.raises(ValueError, match="top_t"):
            search.cosine_topk_tokens(q, tb, 5, top_t=t)
        with pytest.raises(ValueError, match="top_t"):
            search.cosine_token_scores(q, tb, "mean", top_t=t)
    with pytest.raises(ValueError, match="top_t"):
        search.cosine_topk_tokens(q, torch.randn(50, 64, 64, device="cuda"), 5, top_t=17)


@pytest.mark.parametrize("combine", ("mean", "min"))
def test_token_bank_search_with_top_t_equals_the_streaming_driver(combine):
    """cosine_topk_tokens(top_t=3) over build_embedding_bank(pool='tokens'), standardised as similarity_search.py --bank does
    (--bank --n_top_sims 3), picks the images mae_simsearch(..., n_top_sims=3) picks, in the same order.  min scores are
    bit-equal (the same fma chain, then a selection).  mean: the token scores are bit-equal and both sides round three adds and
    one division once each, in different orders, so the scores agree within 4 ulp of the largest score."""
    from sky_embeddings_amd import search
    from sky_embeddings_amd.utils.eval_fns import build_embedding_bank
    from sky_embeddings_amd.utils.similarity import determine_target_features, mae_simsearch
    from tests.test_token_search_gpu import _TinyEncoder
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(8)
    N, B, k, t = 96, 16, 12, 3
    x = torch.randn(N, 5, 16, 16, generator=g)
    rd = torch.stack((torch.arange(N, dtype=torch.float32), torch.zeros(N)), dim=1)       # column 0 carries the image index
    loader = [(x[i:i + B], torch.zeros(B), rd[i:i + B]) for i in range(0, N, B)]
    model = _TinyEncoder().to(dev)
    with torch.no_grad():
        target_latent = model.forward_features(torch.randn(7, 5, 16, 16, generator=g).to(dev))[0]
    imgs, _lat, brd, bsc = mae_simsearch(model, target_latent, loader, dev, metric='cosine', combine=combine, use_weights=True,
                                         max_pool=False, cls_token=False, nested_batches=False, n_save=k, verbose=0, n_top_sims=t)
    bank = build_embedding_bank(model, loader, dev, pool='tokens')
    first = bank[:B]
    mu, sd = first.mean(dim=(0, 1)), first.std(dim=(0, 1), unbiased=True)
    tl = (target_latent[:, 1:] - mu) / (sd + 1e-8)
    search.standardise_(bank.view(-1, 64), mu, sd)
    avg, w = determine_target_features(tl)
    s, i = search.cosine_topk_tokens(avg.reshape(1, -1), bank, k, combine=combine, weights=w, top_t=t)
    assert np.array_equal(i[0].cpu().numpy(), brd[:, 0].cpu().numpy().astype(np.int64))
    assert torch.equal(imgs.cpu(), x[i[0].cpu()])
    got, ref = s[0].cpu().numpy(), bsc.cpu().numpy()
    worst, ulp = np.abs(got - ref).max(), np.spacing(np.abs(ref).max())
    print(combine, "max |delta| vs mae_simsearch =", worst, "= %.2f ulp of the largest score" % (worst / ulp))
    if combine == "mean":
        assert worst < 4 * ulp
    else:
        assert np.array_equal(got, ref)
