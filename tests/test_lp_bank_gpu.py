"""GPU: half-precision resident banks (fp16 / bf16) for the patch-token search.  A 16-bit bank IS the fp32 bank its elements
widen to, so everything is compared bit for bit (np.array_equal) with the CPU restatement tests/token_search_reference.py run on
``bank16.to(torch.float32)``; the 16-bit bank is always made on the CPU by ``torch.from_numpy(x).to(dtype)``."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import similarity_oracle as so
from tests import token_search_reference as tsr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = (torch.float16, torch.bfloat16)
IDS = ("f16", "bf16")


def _weights(rng, D):
    w = rng.random(D, dtype=np.float32) + 0.1
    return w / w.sum()


def _round(x, dtype):
    """-> (the 16-bit bank, rounded on the CPU by torch; its exact fp32 widening as a NumPy array)."""
    b16 = torch.from_numpy(x).to(dtype)
    return b16, b16.to(torch.float32).numpy()


def _scaled_bank(rng, N, P, D, dtype):
    """Rounding acts at different exponents (every 7th image x 1e-3, every 11th x 50); one NaN token, one all-zero token, one
    element that is an fp16 subnormal and, for fp16, one that rounds to inf.  -> (fp32 array, (image, token) of the inf or None)"""
    x = rng.standard_normal((N, P, D), dtype=np.float32)
    x[::7] *= np.float32(1e-3)
    x[::11] *= np.float32(50)
    x[N // 3, P // 2, 5] = np.nan
    x[N // 2, 0] = 0.0
    x[1, 0, 9] = 3e-6
    inf_at = None
    if dtype == torch.float16:
        inf_at = (N // 5, P - 1)
        x[inf_at[0], inf_at[1], 2] = 7e4
    return x, inf_at


@pytest.mark.parametrize("Q", (1, 3, 16))
@pytest.mark.parametrize("D", (64, 192, 768, 1024))
@pytest.mark.parametrize("P", (1, 4, 16, 64))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lp_token_scores_bit_exact(dtype, P, D, Q):
    """D = 64: one 64-element register set; D = 192: an odd number of sets, no multiple of 128.  N off and on whole 16-row
    tiles."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(1000 * P + D + Q)
    for N in ({1: 3001, 4: 1003, 16: 259, 64: 67}[P], {1: 2048, 4: 512, 16: 128, 64: 32}[P]):
        x, inf_at = _scaled_bank(rng, N, P, D, dtype)
        b16, wide = _round(x, dtype)
        assert wide[1, 0, 9] != 0 and abs(wide[1, 0, 9]) < 2.0 ** -14 if dtype == torch.float16 else True
        q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
        s = tsr.token_scores(q, wide, w)
        tb = search.TokenBank(b16.cuda(), torch.from_numpy(w).cuda())
        assert tb.dtype == dtype and tb.norms.dtype == torch.float32
        qd = torch.from_numpy(q).cuda()
        if inf_at is not None:
            assert np.isinf(wide[inf_at[0], inf_at[1], 2]) and np.isneginf(s[:, inf_at[0], inf_at[1]]).all()
        for combine in tsr.COMBINES:
            got = search.cosine_token_scores(qd, tb, combine).cpu().numpy()
            assert np.array_equal(got, tsr.combine_scores(s, combine)), (dtype, P, D, Q, N, combine)
            if inf_at is not None and combine == "min":
                assert np.isneginf(got[:, inf_at[0]]).all()


def _bank_with_duplicates(rng, N, P, D, dtype, q0, w):
    """A 16-bit bank with one NaN token and exact duplicates of the three best images of query 0 (min combine, scored on the
    widened bank) at the end, in the middle and near the start.  -> (16-bit CPU tensor, its fp32 widening)"""
    x = rng.standard_normal((N, P, D), dtype=np.float32)
    x[11, P // 2, 3] = np.nan
    b16, wide = _round(x, dtype)
    best = np.argsort(-tsr.combined_scores(q0, wide, "min", w)[0])[:3]
    for dst, src in ((N - 1, best[0]), (N // 2 + 1, best[1]), (7, best[2])):
        b16[dst] = b16[int(src)]
    return b16, b16.to(torch.float32).numpy()


@pytest.mark.parametrize("Q", (1, 16))
@pytest.mark.parametrize("D", (64, 768))
@pytest.mark.parametrize("P", (1, 16, 64))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lp_token_topk_bit_exact(dtype, P, D, Q):
    from sky_embeddings_amd import ops, search
    rng = np.random.default_rng(77 * P + D + Q)
    N = {1: 24001, 16: 1501, 64: 379}[P]
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    b16, wide = _bank_with_duplicates(rng, N, P, D, dtype, q[:1], w)
    s = tsr.token_scores(q, wide, w)
    tb = search.TokenBank(b16.cuda(), torch.from_numpy(w).cuda())
    qd = torch.from_numpy(q).cuda()
    ks = [k for k in (10, 100, 300) if ops.cosine_token_applicable(Q, P, D, k)]
    assert 10 in ks and 100 in ks and (300 in ks or Q == 16) and all(k <= N for k in ks)
    for combine in tsr.COMBINES:
        sc = tsr.combine_scores(s, combine)
        for k in ks:
            ref_s, ref_i = tsr.topk_of_scores(sc, k)
            for prune in (True, False):
                got_s, got_i = search.cosine_topk_tokens(qd, tb, k, combine, prune=prune)
                assert np.array_equal(got_i.cpu().numpy(), ref_i), (dtype, P, D, Q, combine, k, prune)
                assert np.array_equal(got_s.cpu().numpy(), ref_s), (dtype, P, D, Q, combine, k, prune)


@pytest.mark.parametrize("P,D,Q,N,k", [(4, 128, 16, 20600, 10), (1, 64, 3, 21000, 10)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lp_token_topk_with_the_pruning_floor(dtype, P, D, Q, N, k):
    """The floor comes from a 16-bit sample through the `_lp` scores call, lies strictly below the true k-th best and leaves the
    result unchanged."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(N + P)
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    b16, wide = _bank_with_duplicates(rng, N, P, D, dtype, q[:1], w)
    s = tsr.token_scores(q, wide, w)
    tb = search.TokenBank(b16.cuda(), torch.from_numpy(w).cuda())
    qd = torch.from_numpy(q).cuda()
    tw, qn = search.prepare_queries(qd, tb.weights)
    assert tb.sample(256 * k)[0].dtype == dtype
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


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_weighted_norms_lp_equal_the_fp32_norms_of_the_widened_rows(dtype):
    from sky_embeddings_amd import ops
    rng = np.random.default_rng(4)
    for (N, D) in ((5, 64), (1000, 192), (4099, 768)):
        x = rng.standard_normal((N, D), dtype=np.float32)
        x[::7] *= np.float32(1e-3)
        x[::11] *= np.float32(50)
        b16 = torch.from_numpy(x).to(dtype)
        xd, wided = b16.cuda(), b16.to(torch.float32).cuda()
        for wd in (torch.from_numpy(_weights(rng, D)).cuda(), None):
            got, want = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
            ops.weighted_norms_lp(xd, wd, got)
            ops.weighted_norms(wided, wd, want)
            assert torch.equal(got, want), (dtype, N, D, wd is None)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_standardise_to_is_the_oracle_value_rounded_once(dtype):
    from sky_embeddings_amd import search
    z = np.load(os.path.join(GOLDEN, "similarity.npz"))
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((777, 192), dtype=np.float32) * np.float32(3)).astype(np.float32)
    mu, sd = rng.standard_normal(192, dtype=np.float32), rng.random(192, dtype=np.float32) + np.float32(0.5)
    x[5, 7] = np.nan
    x[9, 3] = 3e5                        # (3e5 - mu) / sd overflows fp16
    sd[11] = 0.0                         # division by 1e-8
    x[3, 11] = mu[11]                    # ... of an exact zero
    for xin, m, s in ((z["std/in"].reshape(-1, 96), z["std/mu"], z["std/sd"]), (x, mu, sd)):
        want = torch.from_numpy(so.standardise_np(xin, m, s)).to(dtype).to(torch.float32).numpy()
        got = search.standardise_to(torch.from_numpy(xin).cuda(), torch.from_numpy(m).cuda(), torch.from_numpy(s).cuda(), dtype)
        assert got.dtype == dtype and got.shape == xin.shape
        assert np.array_equal(got.to(torch.float32).cpu().numpy(), want, equal_nan=True), dtype
    assert np.isnan(want[5, 7]) and want[3, 11] == 0
    if dtype == torch.float16:
        assert np.isinf(want[9, 3]) and np.isinf(want[:, 11]).sum() > 700


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lp_more_than_16_queries_and_two_dimensional_banks(dtype):
    from sky_embeddings_amd import search
    rng = np.random.default_rng(20)
    Q, N, P, D, k = 20, 1501, 16, 128, 10
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    b16, wide = _bank_with_duplicates(rng, N, P, D, dtype, q[:1], w)
    bd, qd, wd = b16.cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(w).cuda()
    for combine in tsr.COMBINES:
        ref_s, ref_i = tsr.topk_tokens(q, wide, k, combine, w)
        stats = {}
        got_s, got_i = search.cosine_topk_tokens(qd, bd, k, combine, weights=wd, stats=stats)
        assert stats["groups"] == 2 and stats["path"] == "tokens"
        assert np.array_equal(got_i.cpu().numpy(), ref_i) and np.array_equal(got_s.cpu().numpy(), ref_s), combine
        assert np.array_equal(search.cosine_token_scores(qd, bd, combine, weights=wd).cpu().numpy(),
                              tsr.combined_scores(q, wide, combine, w))
    # a 2-D 16-bit tensor given to cosine_topk: a token bank with P = 1
    Q, N, D, k = 2, 5000, 128, 10
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    x = rng.standard_normal((N, D), dtype=np.float32)
    x[4000] = x[17]
    b16, wide = _round(x, dtype)
    qd, wd = torch.from_numpy(q).cuda(), torch.from_numpy(w).cuda()
    ref_s, ref_i = tsr.topk_tokens(q, wide[:, None, :], k, "min", w)
    stats = {}
    got_s, got_i = search.cosine_topk(qd, b16.cuda(), k, weights=wd, stats=stats)
    assert stats["path"] == "tokens" and stats["groups"] == 1
    assert np.array_equal(got_i.cpu().numpy(), ref_i) and np.array_equal(got_s.cpu().numpy(), ref_s)
    stats = {}
    search.cosine_topk(qd, torch.from_numpy(x).cuda(), k, weights=wd, stats=stats)
    assert stats == dict(path="exact", redone=0)                 # an fp32 2-D bank takes the path it always took


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


def test_build_embedding_bank_in_fp16_batch_by_batch():
    """The 16-bit bank equals the fp32 bank built with defaults, standardised with the same first-batch statistics by the CPU
    oracle and rounded by torch.  Searching it returns every image whose fp32 score clears the (k+1)-th best by more than twice
    the rounding bound 2u / (1 - u) + 1e-6 (u = 2^-11): rounding can move two scores towards each other by the bound each."""
    from sky_embeddings_amd import search
    from sky_embeddings_amd.utils.eval_fns import build_embedding_bank
    from sky_embeddings_amd.utils.similarity import determine_target_features
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(8)
    N, B, k = 96, 16, 12
    x = torch.randn(N, 5, 16, 16, generator=g)
    loader = [(x[i:i + B], torch.zeros(B), torch.zeros(B, 2)) for i in range(0, N, B)]
    model = _TinyEncoder().to(dev)
    bank32 = build_embedding_bank(model, loader, dev, pool='tokens')
    assert bank32.dtype == torch.float32 and bank32.shape == (N, 16, 64)
    bank16, mu, sd = build_embedding_bank(model, loader, dev, pool='tokens', bank_dtype=torch.float16,
                                          standardise_with_first_batch=True)
    assert bank16.dtype == torch.float16 and bank16.shape == (N, 16, 64) and bank16.is_contiguous()
    first = bank32[:B]
    assert torch.equal(mu, first.mean(dim=(0, 1))) and torch.equal(sd, first.std(dim=(0, 1), unbiased=True))
    std32 = so.standardise_np(bank32.cpu().numpy().reshape(-1, 64), mu.cpu().numpy(), sd.cpu().numpy())
    want = torch.from_numpy(std32).to(torch.float16).view(N, 16, 64)
    assert torch.equal(bank16.cpu(), want)
    # the same images as the fp32 bank wherever the fp32 scores are further apart than the bound
    with torch.no_grad():
        target = model.forward_features(torch.randn(7, 5, 16, 16, generator=g).to(dev))[0][:, 1:]
    avg, w = determine_target_features((target - mu) / (sd + 1e-8))
    bound = 2 * 2.0 ** -11 / (1 - 2.0 ** -11) + 1e-6
    fp32 = torch.from_numpy(std32).view(N, 16, 64).cuda()
    for combine in tsr.COMBINES:
        s32 = search.cosine_token_scores(avg.reshape(1, -1), fp32, combine, weights=w)[0].cpu().numpy()
        _, i32 = search.cosine_topk_tokens(avg.reshape(1, -1), fp32, k, combine=combine, weights=w)
        _, i16 = search.cosine_topk_tokens(avg.reshape(1, -1), bank16, k, combine=combine, weights=w)
        kth1 = np.sort(s32)[::-1][k]
        must = set(np.nonzero(s32 > kth1 + 2 * bound)[0].tolist())
        got = set(i16[0].cpu().tolist())
        print(combine, "fp16 top-k == fp32 top-k:", bool(torch.equal(i16, i32)), "| images that must be found:", len(must))
        assert must <= got, (combine, sorted(must - got))
