"""GPU: the patch-token bank search restricted to a selection of images (``select=`` of search.cosine_topk_tokens /
cosine_token_scores / cosine_topk, the SEL kernels of csrc/topk_tokens.hip) against the CPU restatement on the compacted bank
(tests/token_select_reference.py), bit for bit: np.array_equal on scores and on indices, everywhere.

Shapes are the smallest at which each mechanism can break: N in {37, 531, 4099} (N % 32 != 0: the mask's tail word; a ragged
last tile; 4099 images at P >= 4: more than one workgroup and a short last wave range), P on both sides of the 16-row tile."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import token_search_reference as tsr
from tests import token_select_reference as tsel

PS, NS, QS, KS = (1, 2, 4, 8, 16, 32, 64), (37, 531, 4099), (1, 5, 16), (1, 7, 100)
LP = (torch.float16, torch.bfloat16)


def _weights(rng, D):
    w = rng.random(D, dtype=np.float32) + 0.1
    return w / w.sum()


def _cuda(*arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


def _top_ts(P):
    return [t for t in (None, 1, 3, 16) if t is None or t <= min(P, 16)]


def _masks(N, seed):
    """name -> bool [N]."""
    rng = np.random.default_rng(seed)
    i = np.arange(N)
    m = {"ones": np.ones(N, bool), "zeros": np.zeros(N, bool), "bernoulli_0.5": rng.random(N) < 0.5, "bernoulli_0.05": rng.random(N) < 0.05,
         "runs_64": (i // 64) % 2 == 0, "alternating": i % 2 == 0, "alternating_odd": i % 2 == 1}
    for at in (0, 31, 32, N - 1):
        m[f"one_at_{at}"] = i == at
    return m


def _equal(got, ref, tag):
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(gi, ref[1]), tag
    assert np.array_equal(gs, ref[0]), tag


def test_pack_select_writes_the_documented_words():
    """skyemb_pack_select against the NumPy bit layout, the padding bits zeroed in a buffer that held ones, host and device flags."""
    from sky_embeddings_amd import ops, search
    for N in (1, 31, 32, 33, 37, 64, 255, 256, 257, 531, 4099):
        flags = np.random.default_rng(N).random(N) < 0.5
        flags[[0, N - 1]] = True
        want = tsel.pack_words(flags)
        words = torch.full(((N + 31) // 32 + 2,), -1, dtype=torch.int32, device="cuda")
        ops.pack_select(torch.from_numpy(flags).cuda().view(torch.uint8), words)
        got = words.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:-2], want) and (got[-2:] == 0xFFFFFFFF).all(), N          # nothing past ceil(N / 32) words
        for f in (torch.from_numpy(flags), torch.from_numpy(flags).cuda()):
            sel = search.Selection(f)
            assert sel.N == N and sel.count == int(flags.sum()) and sel.words.is_cuda
            assert np.array_equal(sel.words.cpu().numpy().view(np.uint32), want)
            assert np.array_equal(sel.indices().cpu().numpy(), np.nonzero(flags)[0])


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("P", PS)
def test_select_masks_bit_exact(P, N):
    """Every mask x every combine x every Q on an fp32 bank, D = 64; k, top_t and prune rotate through their values over the 99
    searches of a case (k = 100 where the bank has 100 images, else N: k exceeds the selected count for the sparse masks).  The bank's token
    scores are computed once for 16 queries: a query's result does not depend on the others.

    What the counter n reaches in one case (n = 9 m + 3 c + i for mask m of 11, combine c of 3, query count QS[i]): every
    (mask, combine, Q) once; k = KS[(i + c + m) % 3], so each of the 27 (Q, k, combine) triples occurs under three or four masks;
    top_t = tts[(3 m + c) % len(tts)] (max: 1 wherever that is not None), so with four values every (combine, top_t) pair occurs
    and each mask sees three of them; prune alternates in pairs of searches, so every (mask, combine) runs with and without it.
    A case takes about half a second on the MI355X (the 99 references are lexsorts of at most 16 x 4099 scores)."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(1000 * P + N)
    D = 64
    bank = rng.standard_normal((N, P, D), dtype=np.float32)
    bank[N // 3, P // 2, 5] = np.nan                             # a NaN token in an image that most masks select
    bank[N - 1] = bank[0]                                        # equal images at both ends
    q, w = rng.standard_normal((16, D), dtype=np.float32), _weights(rng, D)
    s = tsr.token_scores(q, bank, w)
    bd, qd, wd = _cuda(bank, q, w)
    tb = search.TokenBank(bd, wd, idx_offset=7)
    tts, n = _top_ts(P), 0
    for name, flags in _masks(N, P + N).items():
        sel = search.Selection(torch.from_numpy(flags))
        assert sel.count == int(flags.sum())
        for combine, Q in [(c, Q) for c in tsr.COMBINES for Q in QS]:
            k, t, prune = min(KS[(n + n // 3 + n // 9) % 3], N), tts[(n // 3) % len(tts)], bool((n // 2) % 2)     # every (Q, k) pair occurs
            n += 1
            if combine == "max" and t is not None:
                t = 1                                            # max is d[0] for every t
            tag = (P, N, name, combine, Q, k, t, prune)
            ref = tsel.topk_of_token_scores_select(s[:Q], k, combine, flags, t, idx_offset=7)
            stats = {}
            got = search.cosine_topk_tokens(qd[:Q], tb, k, combine, prune=prune, stats=stats, top_t=t, select=sel)
            assert stats["selected"] == sel.count and stats["path"] == "tokens"
            _equal(got, ref, tag)
            sc = search.cosine_token_scores(qd[:Q], tb, combine, top_t=t, select=sel).cpu().numpy()
            assert np.array_equal(sc, tsel.scores_of_token_scores_select(s[:Q], combine, flags, t)), tag
            if name == "ones":                                   # the select=None result, bit for bit
                plain = search.cosine_topk_tokens(qd[:Q], tb, k, combine, prune=prune, top_t=t)
                assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), tag
                assert np.array_equal(sc, search.cosine_token_scores(qd[:Q], tb, combine, top_t=t).cpu().numpy()), tag
            if name == "zeros":
                assert bool((got[1] == -1).all()) and bool(torch.isneginf(got[0]).all()) and np.isneginf(sc).all(), tag
            if name.startswith("one_at"):
                at = int(name.split("_")[-1])
                if not (at == N // 3 and combine != "max"):      # the NaN image scores -inf under min and mean
                    assert bool((got[1][:, 0] == at + 7).all()), tag
                assert bool((got[1][:, 1:] == -1).all()), tag


@pytest.mark.parametrize("dtype", (torch.float32,) + LP)
@pytest.mark.parametrize("P", (4, 16, 32))
def test_poisoned_deselected_images_change_nothing(P, dtype):
    """Deselected images filled with NaN and +-6e4 (finite in fp16): every output equals the restatement on the compacted bank
    -- which holds none of them -- and the outputs of the clean bank.  A NaN token in a SELECTED image behaves as ever: -inf under
    min and mean, ignored by max."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(50 * P + LP.index(dtype) if dtype in LP else P)
    N, D, Q, k = 531, 64, 5, 100
    clean = torch.from_numpy(rng.standard_normal((N, P, D), dtype=np.float32)).to(dtype)
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    qd, wd = _cuda(q, w)
    for name in ("bernoulli_0.5", "alternating", "runs_64"):
        flags = _masks(N, P)[name]
        keep = np.nonzero(flags)[0]
        bank = clean.clone()
        bank[int(keep[3]), P // 2, 7] = float("nan")             # a selected image with one NaN token
        bad = bank.clone()
        off = torch.from_numpy(~flags)
        bad[off] = float("nan")
        bad[off, 0::2, 1::3] = 6e4
        bad[off, 1::2, 0::3] = -6e4
        s = tsr.token_scores(q, bank.to(torch.float32).numpy(), w)
        tb_clean, tb_bad = search.TokenBank(bank.cuda(), wd), search.TokenBank(bad.cuda(), wd)
        sel = search.Selection(torch.from_numpy(flags))
        for combine in tsr.COMBINES:
            for t in (None, 3):
                if combine == "max" and t is not None:
                    continue
                ref = tsel.topk_of_token_scores_select(s, k, combine, flags, t)
                if t is None:
                    assert np.isneginf(tsel.scores_of_token_scores_select(s, combine, flags)[:, keep[3]]).all() == (combine != "max")
                got = search.cosine_topk_tokens(qd, tb_bad, k, combine, top_t=t, select=sel)
                _equal(got, ref, (P, dtype, name, combine, t))
                got_clean = search.cosine_topk_tokens(qd, tb_clean, k, combine, top_t=t, select=sel)
                assert torch.equal(got[0], got_clean[0]) and torch.equal(got[1], got_clean[1])
                sc = search.cosine_token_scores(qd, tb_bad, combine, top_t=t, select=sel)
                assert np.array_equal(sc.cpu().numpy(), tsel.scores_of_token_scores_select(s, combine, flags, t))
                assert torch.equal(sc, search.cosine_token_scores(qd, tb_clean, combine, top_t=t, select=sel))


@pytest.mark.parametrize("dtype", (torch.float32,) + LP)
def test_wide_rows_and_the_library_s_own_search_of_the_compacted_bank(dtype):
    """D = 128.  The restatement straight from the compacted BANK (tsel.topk_tokens_select), and the library's plain search over
    ``bank[flags].contiguous()`` with the indices mapped back by hand: the same lists."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(128)
    N, P, D, Q, k = 531, 16, 128, 5, 100
    bank = torch.from_numpy(rng.standard_normal((N, P, D), dtype=np.float32)).to(dtype)
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    qd, wd = _cuda(q, w)
    flags = _masks(N, 3)["bernoulli_0.5"]
    where = torch.from_numpy(np.nonzero(flags)[0]).cuda()
    bd = bank.cuda()
    tb = search.TokenBank(bd, wd, idx_offset=1000)
    compact = search.TokenBank(bd[torch.from_numpy(flags).cuda()].contiguous(), wd)
    for combine, t in (("min", None), ("mean", None), ("max", None), ("min", 3), ("mean", 16)):
        got = search.cosine_topk_tokens(qd, tb, k, combine, top_t=t, select=torch.from_numpy(flags))
        _equal(got, tsel.topk_tokens_select(q, bank.to(torch.float32).numpy(), k, combine, flags, t, w, idx_offset=1000), (dtype, combine, t))
        cs, ci = search.cosine_topk_tokens(qd, compact, k, combine, top_t=t)
        assert torch.equal(got[0], cs) and torch.equal(got[1], torch.where(ci >= 0, where[ci.clamp(min=0)] + 1000, ci))


def test_ties_across_deselected_images():
    """Duplicated images on both sides of a deselected duplicate, inside one tile (P = 4) and across tiles (P = 16)."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(9)
    for P in (4, 16):
        N, D = 531, 64
        bank = rng.standard_normal((N, P, D), dtype=np.float32)
        dup = (1, 2, 3, 40, 41, 300, N - 1)
        for j in dup[1:]:
            bank[j] = bank[1]
        q, w = bank[1].mean(axis=0, keepdims=True), _weights(rng, D)
        flags = np.ones(N, bool)
        flags[[2, 41, 5, 299]] = False
        bd, qd, wd = _cuda(bank, q, w)
        for combine in tsr.COMBINES:
            ref = tsel.topk_tokens_select(q, bank, 10, combine, flags, weights=w)
            got = search.cosine_topk_tokens(qd, search.TokenBank(bd, wd), 10, combine, select=torch.from_numpy(flags).cuda())
            _equal(got, ref, (P, combine))
            gi = got[1][0].cpu().tolist()
            kept = [j for j in dup if flags[j]]
            first = gi.index(kept[0])
            assert gi[first:first + len(kept)] == kept and 2 not in gi and 41 not in gi, (P, combine, gi)


def test_more_than_16_queries_share_one_selection():
    """Q = 20: two groups through the Python API, one Selection; per query the result of a Q = 1 call."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(20)
    Q, N, P, D, k = 20, 531, 16, 64, 7
    bank, q, w = rng.standard_normal((N, P, D), dtype=np.float32), rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    flags = _masks(N, 20)["bernoulli_0.5"]
    s = tsr.token_scores(q, bank, w)
    bd, qd, wd = _cuda(bank, q, w)
    tb, sel = search.TokenBank(bd, wd), search.Selection(torch.from_numpy(flags))
    for combine, t in (("min", None), ("mean", 3)):
        stats = {}
        got = search.cosine_topk_tokens(qd, tb, k, combine, stats=stats, top_t=t, select=sel)
        assert stats["groups"] == 2 and stats["selected"] == sel.count
        _equal(got, tsel.topk_of_token_scores_select(s, k, combine, flags, t), (combine, t))
        sc = search.cosine_token_scores(qd, tb, combine, top_t=t, select=sel)
        assert np.array_equal(sc.cpu().numpy(), tsel.scores_of_token_scores_select(s, combine, flags, t))
        for j in (0, 15, 16, 19):
            one = search.cosine_topk_tokens(qd[j:j + 1], tb, k, combine, top_t=t, select=sel)
            assert torch.equal(one[0][0], got[0][j]) and torch.equal(one[1][0], got[1][j])


def _floor_case(P, D, Q, N, k, flags, seed):
    """Random tokens; every DESELECTED image is the query repeated (token score 1 under every weighting), so a floor taken from
    a sample of the whole bank would lie above every selected score."""
    rng = np.random.default_rng(seed)
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    bank = rng.standard_normal((N, P, D), dtype=np.float32)
    bank[~flags] = q[0]
    return bank, q, w


# The size rule (a floor exists from 8 x 256 x k = 20480 selected images on) leaves room for 100 and 20 deselected images at the
# two shapes of test_token_topk_top_t_with_the_pruning_floor; a selection of about 90 % with a floor needs a larger bank, the
# third and fourth case.
@pytest.mark.parametrize("P,D,Q,N,k,n_off", [(4, 64, 1, 20600, 10, 100), (16, 64, 1, 20500, 10, 20), (4, 64, 1, 23000, 10, 2300),
                                             (16, 64, 1, 23000, 10, 2300)])
def test_selection_with_the_pruning_floor(P, D, Q, N, k, n_off):
    """The floor comes from selected images only: it exists, lies strictly below the k-th best SELECTED score, prune=True and
    prune=False give the restatement's lists, and stats['pruned'] says so."""
    from sky_embeddings_amd import search
    flags = np.ones(N, bool)
    flags[np.random.default_rng(N).choice(N, n_off, replace=False)] = False
    bank, q, w = _floor_case(P, D, Q, N, k, flags, N + P)
    s = tsr.token_scores(q, bank, w)
    bd, qd, wd = _cuda(bank, q, w)
    tb, sel = search.TokenBank(bd, wd), search.Selection(torch.from_numpy(flags))
    tw, qn = search.prepare_queries(qd, tb.weights)
    for combine, t in (("min", None), ("mean", None), ("min", 2)):
        ref = tsel.topk_of_token_scores_select(s, k, combine, flags, t)
        assert ref[0][0, 0] < 0.99                                # no deselected image (score 1) is in the reference
        floor = search.token_pruning_floor(tw, qn, tb, k, combine, top_t=t, select=sel)
        assert floor is not None and bool((floor.cpu().numpy() < ref[0][:, k - 1]).all()), (combine, t, floor, ref[0][:, k - 1])
        assert tb._sample is None                                 # the selected sample is not kept
        for prune in (True, False):
            stats = {}
            got = search.cosine_topk_tokens(qd, tb, k, combine, prune=prune, stats=stats, top_t=t, select=sel)
            assert stats["pruned"] is prune and stats["selected"] == N - n_off
            _equal(got, ref, (combine, t, prune))


def test_the_selected_sample_lives_with_the_selection():
    """Selection.sample: strided over the selected images, gathered once per (bank, weights, size) and again after set_weights
    -- the norms changed -- or for another bank; the bank's own sample stays untouched."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(5)
    N, P, D = 300, 4, 64
    flags = rng.random(N) < 0.5
    bd, w1, w2 = _cuda(rng.standard_normal((N, P, D), dtype=np.float32), _weights(rng, D), _weights(rng, D))
    tb, sel = search.TokenBank(bd, w1), search.Selection(torch.from_numpy(flags))
    st, sn = sel.sample(tb, 20)
    where = np.nonzero(flags)[0][np.arange(20) * (int(flags.sum()) // 20)]
    assert torch.equal(st, bd[torch.from_numpy(where).cuda()]) and torch.equal(sn, tb.norms.view(N, P)[torch.from_numpy(where).cuda()].view(-1))
    assert sel.sample(tb, 20)[0] is st and tb._sample is None
    assert sel.sample(tb, 10)[0].shape[0] == 10
    st = sel.sample(tb, 20)[0]
    tb.set_weights(w2)
    st2, sn2 = sel.sample(tb, 20)
    assert st2 is not st and torch.equal(sn2, tb.norms.view(N, P)[torch.from_numpy(where).cuda()].view(-1)) and not torch.equal(sn2, sn)
    other = search.TokenBank(bd.clone(), w2)
    assert sel.sample(other, 20)[0] is not st2


@pytest.mark.parametrize("P,D,Q,N,k", [(4, 64, 1, 20600, 10), (16, 64, 1, 20500, 10)])
def test_small_selection_has_no_floor(P, D, Q, N, k):
    """5 % selected: fewer than 8 x the sample, so no floor (the whole bank alone would have one) and the results are right."""
    from sky_embeddings_amd import search
    flags = np.random.default_rng(N).random(N) < 0.05
    bank, q, w = _floor_case(P, D, Q, N, k, flags, N + P + 1)
    s = tsr.token_scores(q, bank, w)
    bd, qd, wd = _cuda(bank, q, w)
    tb, sel = search.TokenBank(bd, wd), search.Selection(torch.from_numpy(flags))
    tw, qn = search.prepare_queries(qd, tb.weights)
    assert search.token_pruning_floor(tw, qn, tb, k, "min") is not None
    assert search.token_pruning_floor(tw, qn, tb, k, "min", select=sel) is None
    for combine in ("min", "mean"):
        stats = {}
        got = search.cosine_topk_tokens(qd, tb, k, combine, stats=stats, select=sel)
        assert stats["pruned"] is False and stats["selected"] == int(flags.sum())
        _equal(got, tsel.topk_of_token_scores_select(s, k, combine, flags), combine)


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16))
def test_cosine_topk_select_on_flat_banks(dtype):
    """cosine_topk(select=) on a flat [N, D] bank: the token search with P = 1; equals cosine_topk on the compacted bank (indices
    mapped back) and the restatement.  Q = 20: groups of 16.  A PreparedBank with select is refused, naming the route."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(4)
    N, D, k = 4099, 64, 100
    bank = torch.from_numpy(rng.standard_normal((N, D), dtype=np.float32)).to(dtype)
    q, w = rng.standard_normal((20, D), dtype=np.float32), _weights(rng, D)
    qd, wd = _cuda(q, w)
    bd = bank.cuda()
    for name in ("bernoulli_0.5", "bernoulli_0.05", "runs_64"):
        flags = _masks(N, 4)[name]
        fd = torch.from_numpy(flags).cuda()
        where = torch.nonzero(fd).squeeze(1)
        for Q in (1, 20):
            stats = {}
            got = search.cosine_topk(qd[:Q], bd, k, weights=wd, stats=stats, select=fd)
            assert stats["path"] == "tokens" and stats["selected"] == int(flags.sum())
            _equal(got, tsel.topk_tokens_select(q[:Q], bank.to(torch.float32).numpy()[:, None], k, "min", flags, weights=w), (dtype, name, Q))
            kc = min(k, int(flags.sum()))
            cs, ci = search.cosine_topk(qd[:Q], bd[fd].contiguous(), kc, weights=wd)
            assert torch.equal(got[0][:, :kc], cs) and torch.equal(got[1][:, :kc], where[ci])
            assert bool((got[1][:, kc:] == -1).all())
    if dtype == torch.float32:
        with pytest.raises(ValueError, match="cosine_topk_tokens"):
            search.cosine_topk(qd[:1], search.PreparedBank(bd, wd), k, select=fd)


def test_sel_entry_points_with_a_null_selection_are_the_top_calls():
    """select == NULL through the `_sel` entry points: the `_top` call's outputs, list for list, for the three bank types."""
    from sky_embeddings_amd import ops, search
    from sky_embeddings_amd._lib import lib
    rng = np.random.default_rng(21)
    Q, N, P, D, k = 3, 531, 16, 64, 7
    st = torch.cuda.current_stream().cuda_stream
    for dtype in (torch.float32,) + LP:
        bank = torch.from_numpy(rng.standard_normal((N, P, D), dtype=np.float32)).to(dtype).cuda()
        qd, wd = _cuda(rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D))
        tb = search.TokenBank(bank, wd)
        tw, qn = search.prepare_queries(qd, tb.weights)
        nl, code = ops.cosine_token_topk_chunks(N, P, Q, D, k), ops.bank_dtype_code(dtype, "test")
        for c, t in ((0, 0), (1, 3), (2, 0)):
            want = torch.full((Q, N), 7.0, device="cuda")
            got = want.clone()
            ops.cosine_token_scores(tw, qn, bank, tb.norms, c, 1e-6, want, t)
            ops.check(lib().skyemb_cosine_token_scores_sel(tw.data_ptr(), qn.data_ptr(), bank.data_ptr(), code, tb.norms.data_ptr(), Q, N, P, D,
                                                           c, t, 1e-6, got.data_ptr(), None, st), "skyemb_cosine_token_scores_sel")
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
            ps, pi = torch.full((Q, nl, k), 7.0, device="cuda"), torch.full((Q, nl, k), 7, device="cuda", dtype=torch.int64)
            ps2, pi2 = ps.clone(), pi.clone()
            ops.cosine_token_topk(tw, qn, bank, tb.norms, k, c, 1e-6, 5, nl, ps, pi, None, t)
            ops.check(lib().skyemb_cosine_token_topk_sel(tw.data_ptr(), qn.data_ptr(), bank.data_ptr(), code, tb.norms.data_ptr(), Q, N, P, D, k,
                                                         c, t, 1e-6, 5, nl, None, ps2.data_ptr(), pi2.data_ptr(), None, st),
                      "skyemb_cosine_token_topk_sel")
            assert torch.equal(ps2.view(torch.int32), ps.view(torch.int32)) and torch.equal(pi2, pi)


def test_bad_selections_raise_before_any_launch():
    """A wrong-length mask on a bank whose shape the kernel takes, a wrong dtype and two dimensions: ValueError, outputs never
    allocated; a misaligned word pointer is the library's refusal."""
    from sky_embeddings_amd import ops, search
    q = torch.randn(2, 64, device="cuda")
    tb = search.TokenBank(torch.randn(50, 4, 64, device="cuda"))
    search.cosine_topk_tokens(q, tb, 5, select=torch.ones(50, dtype=torch.bool, device="cuda"))      # the shape is accepted
    for n in (49, 51, 0):
        for bad in (torch.ones(n, dtype=torch.bool, device="cuda"), search.Selection(torch.ones(n, dtype=torch.bool))):
            with pytest.raises(ValueError, match="select describes"):
                search.cosine_topk_tokens(q, tb, 5, select=bad)
            with pytest.raises(ValueError, match="select describes"):
                search.cosine_token_scores(q, tb, select=bad)
            with pytest.raises(ValueError, match="select describes"):
                search.cosine_topk(q, tb.bank[:, 0].contiguous(), 5, select=bad)
    for bad in (torch.ones(50, dtype=torch.uint8, device="cuda"), torch.ones(50, 1, dtype=torch.bool, device="cuda")):
        with pytest.raises(ValueError, match="Selection"):
            search.cosine_topk_tokens(q, tb, 5, select=bad)
    tw, qn = search.prepare_queries(q, None)
    words = torch.zeros(9, dtype=torch.int8, device="cuda")[1:]                                      # odd address
    with pytest.raises(RuntimeError, match="select must be 4-byte aligned"):
        ops.cosine_token_scores(tw, qn, tb.bank, tb.norms, 0, 1e-6, torch.empty(2, 50, device="cuda"), 0, words)
