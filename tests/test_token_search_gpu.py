"""GPU: the patch-token bank search (search.cosine_token_scores / cosine_topk_tokens, csrc/topk_tokens.hip) against the CPU
restatement tests/token_search_reference.py, bit for bit (np.array_equal on scores and on indices)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import similarity_oracle as so
from tests import token_search_reference as tsr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PS, DS, QS = (1, 4, 16, 64, 256), (64, 128, 768, 1024), (1, 3, 16)


def _weights(rng, D):
    w = rng.random(D, dtype=np.float32) + 0.1
    return w / w.sum()


def _cuda(*arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", PS)
def test_token_scores_bit_exact(P, D, Q):
    """N both at and off whole 16-row tiles and whole waves (P = 4: N * P = 4012 is not a multiple of 16)."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(1000 * P + D + Q)
    for N in ({1: 3001, 4: 1003, 16: 259, 64: 67, 256: 19}[P], {1: 2048, 4: 512, 16: 128, 64: 32, 256: 8}[P]):
        bank = rng.standard_normal((N, P, D), dtype=np.float32)
        bank[N // 3, P // 2, 5] = np.nan                    # a NaN token
        bank[N // 2, 0] = 0.0                               # an all-zero token
        q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
        s = tsr.token_scores(q, bank, w)
        bd, qd, wd = _cuda(bank, q, w)
        tb = search.TokenBank(bd, wd)
        for combine in tsr.COMBINES:
            got = search.cosine_token_scores(qd, tb, combine).cpu().numpy()
            assert np.array_equal(got, tsr.combine_scores(s, combine)), (P, D, Q, N, combine)


def _planted_bank(rng, N, P, D, q0, w):
    """Random tokens with one NaN token and exact duplicate images among the best of query 0 (min combine): at the end, in the
    middle and near the start of the bank -- inside and outside a strided sample."""
    bank = rng.standard_normal((N, P, D), dtype=np.float32)
    bank[11, P // 2, 3] = np.nan
    best = np.argsort(-tsr.combined_scores(q0, bank, "min", w)[0])[:3]
    bank[N - 1] = bank[best[0]]
    bank[N // 2 + 1] = bank[best[1]]
    bank[7] = bank[best[2]]
    return bank


def _ks(Q, P, D, N):
    from sky_embeddings_amd import ops
    ks = [k for k in (10, 100, 300) if ops.cosine_token_applicable(Q, P, D, k)]
    assert 10 in ks and 100 in ks and (300 in ks or Q == 16)       # 16 x 300 list entries per wave exceed the LDS formula
    assert all(k <= N for k in ks)
    return ks


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", PS)
def test_token_topk_bit_exact(P, D, Q):
    """Tens of thousands of rows; most waves see fewer than k finite images (P = 256: a handful of images per wave)."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(77 * P + D + Q)
    N = {1: 24001, 4: 6003, 16: 1501, 64: 379, 256: 301}[P]
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    bank = _planted_bank(rng, N, P, D, q[:1], w)
    s = tsr.token_scores(q, bank, w)
    bd, qd, wd = _cuda(bank, q, w)
    tb = search.TokenBank(bd, wd)
    for combine in tsr.COMBINES:
        sc = tsr.combine_scores(s, combine)
        for k in _ks(Q, P, D, N):
            ref_s, ref_i = tsr.topk_of_scores(sc, k)
            for prune in (True, False):
                got_s, got_i = search.cosine_topk_tokens(qd, tb, k, combine, prune=prune)
                assert np.array_equal(got_i.cpu().numpy(), ref_i), (P, D, Q, combine, k, prune)
                assert np.array_equal(got_s.cpu().numpy(), ref_s), (P, D, Q, combine, k, prune)


@pytest.mark.parametrize("P,D,Q,N,k", [(1, 64, 3, 21000, 10), (4, 128, 16, 20600, 10), (16, 64, 1, 20500, 10), (64, 64, 2, 2600, 1),
                                       (4, 64, 1, 615000, 300)])
def test_token_topk_with_the_pruning_floor(P, D, Q, N, k):
    """Banks of at least 8 x 256 x k images: the floor from the image sample is used, lies strictly below the true k-th best
    combined score, and leaves the result unchanged."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(N + P)
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    bank = _planted_bank(rng, N, P, D, q[:1], w)
    s = tsr.token_scores(q, bank, w)
    bd, qd, wd = _cuda(bank, q, w)
    tb = search.TokenBank(bd, wd)
    tw, qn = search.prepare_queries(qd, tb.weights)
    for combine in tsr.COMBINES:
        ref_s, ref_i = tsr.topk_of_scores(tsr.combine_scores(s, combine), k)
        floor = search.token_pruning_floor(tw, qn, tb, k, combine)
        assert floor is not None and bool((floor.cpu().numpy() < ref_s[:, k - 1]).all()), (combine, floor, ref_s[:, k - 1])
        for prune in (True, False):
            stats = {}
            got_s, got_i = search.cosine_topk_tokens(qd, tb, k, combine, prune=prune, stats=stats)
            assert stats == dict(path="tokens", groups=1, pruned=prune)
            assert np.array_equal(got_i.cpu().numpy(), ref_i), (combine, prune)
            assert np.array_equal(got_s.cpu().numpy(), ref_s), (combine, prune)


def test_more_than_16_queries_run_in_groups():
    from sky_embeddings_amd import search
    rng = np.random.default_rng(20)
    Q, N, P, D, k = 20, 1501, 16, 128, 10
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    bank = _planted_bank(rng, N, P, D, q[:1], w)
    bd, qd, wd = _cuda(bank, q, w)
    for combine in tsr.COMBINES:
        ref_s, ref_i = tsr.topk_tokens(q, bank, k, combine, w)
        stats = {}
        got_s, got_i = search.cosine_topk_tokens(qd, bd, k, combine, weights=wd, stats=stats)
        assert stats["groups"] == 2
        assert np.array_equal(got_i.cpu().numpy(), ref_i) and np.array_equal(got_s.cpu().numpy(), ref_s), combine
        assert np.array_equal(search.cosine_token_scores(qd, bd, combine, weights=wd).cpu().numpy(),
                              tsr.combined_scores(q, bank, combine, w))


def test_fewer_than_k_finite_images_end_in_terminators():
    """35 of 40 images hold a NaN token: min and mean return the 5 finite images, then (-inf, -1); max ignores the NaN tokens."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(9)
    N, P, D, k = 40, 4, 64, 10
    bank = rng.standard_normal((N, P, D), dtype=np.float32)
    bank[5:, 1, 0] = np.nan
    q = rng.standard_normal((2, D), dtype=np.float32)
    bd, qd = _cuda(bank, q)
    for combine in tsr.COMBINES:
        ref_s, ref_i = tsr.topk_tokens(q, bank, k, combine)
        got_s, got_i = search.cosine_topk_tokens(qd, bd, k, combine)
        assert np.array_equal(got_i.cpu().numpy(), ref_i) and np.array_equal(got_s.cpu().numpy(), ref_s), combine
        if combine != "max":
            assert sorted(ref_i[0, :5].tolist()) == [0, 1, 2, 3, 4] and (ref_i[:, 5:] == -1).all()


@pytest.mark.parametrize("T,P,N", [(65, 16, 128), (65, 64, 64)])
def test_reference_goldens_on_the_gpu(T, P, N):
    """D = 96 zero-padded to 128 in bank, query and weights: a zero column adds fma(0, 0, acc) and changes no bit, so the results
    equal the unpadded CPU restatement bit for bit and sit within 5e-7 of the reference's combined scores."""
    from sky_embeddings_amd import search
    z = np.load(os.path.join(GOLDEN, "similarity.npz"))
    key = f"sim/{T}_{P}_{N}"
    tgt, tst = torch.from_numpy(z[key + "/target"]), z[key + "/test"]
    avg, w = so.determine_target_features(tgt)
    avg, w = avg.numpy(), w.numpy()

    def pad(a):
        return np.ascontiguousarray(np.concatenate((a, np.zeros(a.shape[:-1] + (32,), np.float32)), axis=-1))
    for uw in (1, 0):
        weights = w if uw else np.ones(96, np.float32)
        bd, qd, wd = _cuda(pad(tst), pad(avg[None]), pad(weights))
        tb = search.TokenBank(bd, wd)
        for combine in tsr.COMBINES:
            want = tsr.combined_scores(avg[None], tst, combine, weights)
            got = search.cosine_token_scores(qd, tb, combine).cpu().numpy()
            assert np.array_equal(got, want), (key, combine, uw)
            ref = z[f"{key}/cosine_{combine}_{uw}"]
            err = np.abs(got[0] - ref).max()
            print(key, combine, uw, "max |delta| vs golden =", err)
            assert err < 5e-7, (key, combine, uw, err)
            got_s, got_i = search.cosine_topk_tokens(qd, tb, 10, combine)
            ref_s, ref_i = tsr.topk_of_scores(want, 10)
            assert np.array_equal(got_i.cpu().numpy(), ref_i) and np.array_equal(got_s.cpu().numpy(), ref_s)


def test_sharded_token_bank_merge_equals_single_bank():
    """Two 'ranks' in one process: per-shard top-k (global image indices via idx_offset) + k-way merge == whole bank."""
    from sky_embeddings_amd import ops, search
    rng = np.random.default_rng(3)
    Q, N, P, D, k = 5, 3000, 16, 128, 12
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = rng.standard_normal((N, P, D), dtype=np.float32)
    x[2500] = x[100]
    qd = torch.from_numpy(q).cuda()
    for combine in tsr.COMBINES:
        whole_s, whole_i = search.cosine_topk_tokens(qd, torch.from_numpy(x).cuda(), k, combine)
        parts = []
        for lo, hi in ((0, 1500), (1500, 3000)):
            tb = search.TokenBank(torch.from_numpy(x[lo:hi]).cuda(), None, idx_offset=lo)
            parts.append(search.cosine_topk_tokens(qd, tb, k, combine))
        gs = torch.stack([p[0] for p in parts], dim=1).contiguous()
        gi = torch.stack([p[1] for p in parts], dim=1).contiguous()
        out_s, out_i = torch.empty(Q, k, device="cuda"), torch.empty(Q, k, device="cuda", dtype=torch.int64)
        ops.topk_merge(gs, gi, Q, 2, k, out_s, out_i)
        assert torch.equal(out_i, whole_i) and torch.equal(out_s, whole_s)
        ref_s, ref_i = tsr.topk_tokens(q, x, k, combine)
        assert np.array_equal(out_i.cpu().numpy(), ref_i) and np.array_equal(out_s.cpu().numpy(), ref_s)


class _TinyEncoder(torch.nn.Module):
    """One linear layer over 4 x 4 pixel blocks: [B, 5, 16, 16] -> a cls row (mean of the patch rows) + 16 patch tokens of
    width 64.  Deterministic, so two passes over the loader give the same tokens."""
    num_extra_tokens = 1

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(4)
        self.W = torch.nn.Parameter(torch.randn(80, 64, generator=g) * 0.2, requires_grad=False)

    def forward_features(self, x, ra_dec=None, mask_ratio=0, mask=None, reshape_out=False):
        B, C, H, Wd = x.shape
        p = x.reshape(B, C, H // 4, 4, Wd // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // 4) * (Wd // 4), C * 16)
        tok = p @ self.W
        return torch.cat((tok.mean(dim=1, keepdim=True), tok), dim=1), None, None


@pytest.mark.parametrize("combine", tsr.COMBINES)
def test_token_bank_search_equals_the_streaming_driver(combine):
    """cosine_topk_tokens over build_embedding_bank(pool='tokens'), standardised as similarity_search.py --bank does, picks the
    images mae_simsearch(max_pool=False, cls_token=False) picks, in the same order; min / max scores bit-equal (the same fma
    chain, then an exact reduction), mean within 5e-7 (torch.mean's summation order is not the kernel's).  Random inputs: no
    exact ties (mae_simsearch orders ties by arrival)."""
    from sky_embeddings_amd import search
    from sky_embeddings_amd.utils.eval_fns import build_embedding_bank
    from sky_embeddings_amd.utils.similarity import determine_target_features, mae_simsearch
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(8)
    N, B, k = 96, 16, 12
    x = torch.randn(N, 5, 16, 16, generator=g)
    rd = torch.stack((torch.arange(N, dtype=torch.float32), torch.zeros(N)), dim=1)       # column 0 carries the image index
    loader = [(x[i:i + B], torch.zeros(B), rd[i:i + B]) for i in range(0, N, B)]
    model = _TinyEncoder().to(dev)
    with torch.no_grad():
        target_latent = model.forward_features(torch.randn(7, 5, 16, 16, generator=g).to(dev))[0]
    imgs, _lat, brd, bsc = mae_simsearch(model, target_latent, loader, dev, metric='cosine', combine=combine, use_weights=True,
                                         max_pool=False, cls_token=False, nested_batches=False, n_save=k, verbose=0)
    bank = build_embedding_bank(model, loader, dev, pool='tokens')
    assert bank.shape == (N, 16, 64) and bank.dtype == torch.float32 and bank.is_contiguous()
    first = bank[:B]
    mu, sd = first.mean(dim=(0, 1)), first.std(dim=(0, 1), unbiased=True)
    tl = (target_latent[:, 1:] - mu) / (sd + 1e-8)
    search.standardise_(bank.view(-1, 64), mu, sd)
    avg, w = determine_target_features(tl)
    s, i = search.cosine_topk_tokens(avg.reshape(1, -1), bank, k, combine=combine, weights=w)
    assert np.array_equal(i[0].cpu().numpy(), brd[:, 0].cpu().numpy().astype(np.int64))
    assert torch.equal(imgs.cpu(), x[i[0].cpu()])
    got, ref = s[0].cpu().numpy(), bsc.cpu().numpy()
    print(combine, "max |delta| vs mae_simsearch =", np.abs(got - ref).max())
    if combine == "mean":
        assert np.abs(got - ref).max() < 5e-7
    else:
        assert np.array_equal(got, ref)


def test_refused_shapes_raise_before_any_launch():
    from sky_embeddings_amd import search
    q64, q96 = torch.randn(2, 64, device="cuda"), torch.randn(2, 96, device="cuda")
    with pytest.raises(ValueError, match="16 % P == 0"):
        search.cosine_topk_tokens(q64, torch.randn(50, 9, 64, device="cuda"), 5)
    with pytest.raises(ValueError, match="D % 64 == 0"):
        search.cosine_topk_tokens(q96, torch.randn(50, 16, 96, device="cuda"), 5)
    with pytest.raises(ValueError, match="D % 64 == 0"):
        search.cosine_token_scores(q96, torch.randn(50, 16, 96, device="cuda"), "min")
    bank = torch.randn(50, 16, 64, device="cuda")
    with pytest.raises(ValueError, match="combine"):
        search.cosine_topk_tokens(q64, bank, 5, combine="median")
    with pytest.raises(ValueError, match="combine"):
        search.cosine_token_scores(q64, bank, "median")
    for k in (0, 51):
        with pytest.raises(ValueError):
            search.cosine_topk_tokens(q64, bank, k)
    with pytest.raises(ValueError, match="163840"):
        search.cosine_topk_tokens(torch.randn(16, 64, device="cuda"), torch.randn(400, 16, 64, device="cuda"), 400)
    s, i = search.cosine_topk_tokens(torch.empty(0, 64, device="cuda"), bank, 5)                # no queries: no launch
    assert s.shape == (0, 5) and i.shape == (0, 5) and i.dtype == torch.int64
    s, i = search.cosine_topk_tokens(q64, bank, 50)                                            # k == N: every image
    assert torch.isfinite(s).all() and sorted(i[0].tolist()) == list(range(50))


def test_prefiltered_search_refuses_a_q_times_n_beyond_its_32_bit_counters_before_any_launch():
    """Stage 1 of the two-stage search counts work items and k-steps in 32 bits: ceil(N / 2048) * ceil(Q / 256) * (D / 32) must stay
    below 2^31 (include/skyemb.h, "Addressing limits").  Past that the call returns 1 with the limit in its text and launches
    nothing -- every pointer here is one small buffer and the workspace is declared empty, so a launch could not go unnoticed; a
    shape inside the limit gets past this check and is stopped by the next one, the workspace size."""
    from sky_embeddings_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(1024, device="cuda")
    p, N, D, k = buf.data_ptr(), 2 ** 31 - 256, 768, 100
    args = lambda Q: (p, p, Q, p, p, p, p, N, D, k, 1e-6, 0, None, p, 0, p, p, p, None)
    for call in (L.skyemb_cosine_topk_prefiltered,
                 lambda *a: L.skyemb_cosine_topk_prefiltered_lp(*a[:3], a[5], a[4], None, *a[6:])):   # (tw, qn, Q, bank16, xn, tail, rowp, ...)
        assert call(*args(600_000)) == 1
        text = L.skyemb_last_error().decode()
        assert "Q x N too large" in text and "below 2^31" in text and "Q=600000" in text, text
        assert call(*args(33)) == 1
        assert "workspace too small" in L.skyemb_last_error().decode()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0
