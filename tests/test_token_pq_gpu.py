"""GPU: per-query feature weights in the patch-token bank search (``weights`` [Q, D] of search.cosine_topk_tokens /
cosine_token_scores / cosine_topk / distance_topk_tokens / distance_token_scores; the PQW kernels of csrc/topk_tokens.hip and the
PQC kernels of csrc/distance_tokens.hip) against the CPU restatements, bit for bit: np.array_equal on scores and on indices.
Cosine: tests/token_pq_reference.py.  Distance: the existing single-weight call is the yardstick (and it equals
tests/token_distance_reference.py).

On the parent commit a [Q, D] ``weights`` never reaches a kernel as such: the cosine calls hand it to skyemb_weighted_norms as
if it were [D] (every query and every bank norm then takes ROW 0 -- silently wrong for every other query), the distance calls
fail in ``prepare_distance_weights`` (reshape of Q D values to D).  The bit-for-bit, independence and distance tests below
therefore fail there.

Shapes are the smallest at which each mechanism can break: D = 64 (one register set), 192 (nchunk % 8 != 0: the loop's odd tail)
and 768 (the product width); P on both sides of the 16-row tile and across two tiles; Q = 1, 5, 16 (zero rows of both operand
images; a partly filled lane group; full); banks of 2 000 to 5 000 images whose row count is no multiple of a wave's range."""
import configparser
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import token_distance_reference as tdr
from tests import token_pq_reference as pq

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
# P -> (images, ((D, Q), ...)): every D and every Q with every P; Q D rows is what the CPU restatement pays for
SHAPES = {1: (5003, ((64, 1), (192, 5), (768, 16))),
          4: (2003, ((64, 16), (192, 1), (768, 5))),
          16: (2001, ((64, 16), (192, 5), (768, 1))),
          32: (2001, ((64, 16), (192, 5), (768, 1)))}
CASES = [(dt, P, D, Q) for dt in DTYPES for P, (_, dq) in SHAPES.items() for D, Q in dq]
KS = (1, 100)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _weights(rng, Q, D):
    """Q different positive weight rows of very different scales per feature (inverse variances look like this)."""
    return (rng.random((Q, D), dtype=np.float32) + np.float32(0.05)) * np.exp(rng.standard_normal((Q, D))).astype(np.float32)


def _bank(rng, N, P, D, dtype=torch.float32):
    """(the bank as the device holds it, its exactly widened fp32 image as NumPy)."""
    b = torch.from_numpy(rng.standard_normal((N, P, D), dtype=np.float32)).to(dtype)
    return b, b.to(torch.float32).numpy()


def _equal(got, ref, tag):
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(gi, ref[1]), tag
    assert np.array_equal(gs, ref[0]), tag


@pytest.mark.parametrize("dtype,P,D,Q", CASES, ids=[f"{str(dt)[6:]}-P{P}-D{D}-Q{Q}" for dt, P, D, Q in CASES])
def test_cosine_per_query_weights_bit_exact(dtype, P, D, Q):
    """Scores of every image and the top-k for k = 1 and 100, every combine, on one bank per case; the restatement's token scores
    are computed once.  A NaN token and equal images at both ends are planted."""
    from sky_embeddings_amd import search
    N = SHAPES[P][0]
    rng = np.random.default_rng(1000 * P + D + Q)
    bank_t, bank = _bank(rng, N, P, D, dtype)
    bank_t[N // 3, P // 2, 5] = float("nan")
    bank_t[N - 1] = bank_t[0]
    bank = bank_t.to(torch.float32).numpy()
    q, W = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, Q, D)
    bd, (qd, Wd) = bank_t.cuda(), _cuda(q, W)
    s = pq.token_scores_pq(q, bank, W)
    for combine in pq.COMBINES:
        sc = search.cosine_token_scores(qd, bd, combine, weights=Wd).cpu().numpy()
        assert np.array_equal(sc, pq.combine(s, combine)), (combine,)
        for k in KS:
            stats = {}
            got = search.cosine_topk_tokens(qd, bd, k, combine, weights=Wd, stats=stats)
            assert stats["path"] == "tokens" and stats["per_query_weights"] is True and stats["group"] == 16
            _equal(got, pq.topk_of_token_scores(s, k, combine), (combine, k))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_rows_of_the_weight_image_do_not_leak(dtype):
    """Q = 16 with 16 different weight rows: row q of the result is the Q = 1 call with query q and its row alone, bit for bit
    (a Q = 1 call has 15 zero rows in both operand images)."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(21)
    N, P, D, k = 2003, 4, 192, 100
    bank_t, _ = _bank(rng, N, P, D, dtype)
    qd, Wd = _cuda(rng.standard_normal((16, D), dtype=np.float32), _weights(rng, 16, D))
    bd = bank_t.cuda()
    for combine in ("min", "mean"):
        all_s, all_i = search.cosine_topk_tokens(qd, bd, k, combine, weights=Wd)
        all_sc = search.cosine_token_scores(qd, bd, combine, weights=Wd)
        for i in range(16):
            one_s, one_i = search.cosine_topk_tokens(qd[i:i + 1], bd, k, combine, weights=Wd[i:i + 1])
            assert torch.equal(one_i[0], all_i[i]) and torch.equal(one_s[0], all_s[i]), (combine, i)
            assert torch.equal(search.cosine_token_scores(qd[i:i + 1], bd, combine, weights=Wd[i:i + 1])[0], all_sc[i]), (combine, i)


def test_one_hot_weight_blocks_search_their_own_features():
    """Weight rows that are 1 on disjoint feature blocks and 0 elsewhere: a zero weight adds an exact zero to both chains, so
    each query's result is the restatement's on the bank restricted to its block, bit for bit."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(22)
    N, P, D, k = 2003, 4, 192, 100
    _, bank = _bank(rng, N, P, D)
    q = rng.standard_normal((3, D), dtype=np.float32)
    W = np.zeros((3, D), np.float32)
    for i in range(3):
        W[i, 64 * i:64 * i + 64] = 1
    bd, qd, Wd = _cuda(bank, q, W)
    for combine in pq.COMBINES:
        got = search.cosine_topk_tokens(qd, bd, k, combine, weights=Wd)
        for i in range(3):
            blk = slice(64 * i, 64 * i + 64)
            ref = pq.topk_tokens_pq(q[i:i + 1, blk], bank[:, :, blk], k, combine, np.ones((1, 64), np.float32))
            _equal((got[0][i:i + 1], got[1][i:i + 1]), ref, (combine, i))
        assert len({tuple(r) for r in got[1].cpu().numpy().tolist()}) == 3          # three different answers


def test_composes_with_top_t_selection_pruning_and_idx_offset():
    """top_t = 3 (min, mean) over a random half of a TokenBank with idx_offset = 7, whose own weights must go unused; k = 1 has a
    pruning floor (2 500 selected images >= 8 x 256 k), and prune=False must give the same bits."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(23)
    N, P, D, Q = 5003, 4, 64, 5
    _, bank = _bank(rng, N, P, D)
    q, W = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, Q, D)
    flags = rng.random(N) < 0.5
    bd, qd, Wd = _cuda(bank, q, W)
    own = torch.from_numpy(rng.random(D, dtype=np.float32) + 0.1).cuda()
    tb = search.TokenBank(bd, own, idx_offset=7)
    norms = tb.norms.clone()
    sel = search.Selection(torch.from_numpy(flags))
    s = pq.token_scores_pq(q, bank, W)
    for combine in ("min", "mean"):
        for k in KS:
            ref = pq.topk_of_token_scores(s, k, combine, 3, flags, idx_offset=7)
            stats = {}
            got = search.cosine_topk_tokens(qd, tb, k, combine, weights=Wd, top_t=3, select=sel, stats=stats)
            assert stats["pruned"] == (k == 1) and stats["top_t"] == 3 and stats["selected"] == sel.count
            _equal(got, ref, (combine, k))
            plain = search.cosine_topk_tokens(qd, tb, k, combine, weights=Wd, top_t=3, select=sel, prune=False)
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), (combine, k)
        sc = search.cosine_token_scores(qd, tb, combine, weights=Wd, top_t=3, select=sel).cpu().numpy()
        from tests import token_select_reference as tsel
        assert np.array_equal(sc, tsel.scores_of_token_scores_select(s, combine, flags, 3)), combine
    assert tb.weights is own or torch.equal(tb.weights, own)
    assert torch.equal(tb.norms, norms)
    # the floor itself: scored by the kernel with per-query weights, a lower bound of the k-th best selected score
    tw, qn = search.prepare_queries_pq(qd, Wd)
    floor = search.token_pruning_floor(tw, qn, bd, 1, "min", top_t=3, select=sel, weights=Wd)
    best = pq.topk_of_token_scores(s, 1, "min", 3, flags)[0][:, 0]
    assert floor is not None and bool((floor.cpu().numpy() < best).all())


def test_special_values():
    from sky_embeddings_amd import search
    rng = np.random.default_rng(24)
    N, P, D, Q, k = 2003, 4, 64, 5, 100
    _, bank = _bank(rng, N, P, D)
    q, W = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, Q, D)
    bd, qd, Wd = _cuda(bank, q, W)
    base = search.cosine_topk_tokens(qd, bd, k, "mean", weights=Wd)
    # an all-zero weight row: every score is 0 / eps = 0, the k lowest image indices in order
    W0 = Wd.clone()
    W0[2] = 0
    s0, i0 = search.cosine_topk_tokens(qd, bd, k, "mean", weights=W0)
    assert bool((s0[2] == 0).all()) and i0[2].tolist() == list(range(k))
    assert bool((search.cosine_token_scores(qd, bd, "mean", weights=W0)[2] == 0).all())
    keep = [0, 1, 3, 4]
    assert torch.equal(s0[keep], base[0][keep]) and torch.equal(i0[keep], base[1][keep])
    # a NaN in one query's weights: that query returns only (-inf, -1), every other query's bits are unchanged
    Wn = Wd.clone()
    Wn[2, 17] = float("nan")
    sn, inn = search.cosine_topk_tokens(qd, bd, k, "mean", weights=Wn)
    assert bool(torch.isneginf(sn[2]).all()) and bool((inn[2] == -1).all())
    assert torch.equal(sn[keep], base[0][keep]) and torch.equal(inn[keep], base[1][keep])
    # a negative sum under the root: NaN norm, NaN score, -inf
    Wm = Wd.clone()
    Wm[2] = -Wm[2]
    sm, im = search.cosine_topk_tokens(qd, bd, k, "max", weights=Wm)
    assert bool(torch.isneginf(sm[2]).all()) and bool((im[2] == -1).all())
    # a NaN token in a deselected image changes nothing
    flags = rng.random(N) < 0.5
    flags[11] = False
    sel = search.Selection(torch.from_numpy(flags))
    clean = search.cosine_topk_tokens(qd, bd, k, "mean", weights=Wd, select=sel)
    dirty_bank = bd.clone()
    dirty_bank[11, 1, 3] = float("nan")
    dirty = search.cosine_topk_tokens(qd, dirty_bank, k, "mean", weights=Wd, select=sel)
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])
    _equal(clean, pq.topk_tokens_pq(q, bank, k, "mean", W, flags=flags), "select")


@pytest.mark.parametrize("Q,D,k,g", ((17, 64, 100, 16), (4, 1024, 300, 3)))
def test_more_queries_than_one_pass_holds(Q, D, k, g):
    """Groups of g = the largest count with 128 D + 32 g k <= 163840: 16 at D = 64, and 3 at (D = 1024, k = 300), where
    131072 + 9600 g <= 163840 holds up to g = 3.  Weights are sliced along with the queries."""
    from sky_embeddings_amd import search
    assert max(x for x in range(1, 17) if 128 * D + 32 * x * k <= 163840) == g
    rng = np.random.default_rng(25 + Q)
    N, P = 2001, 1
    _, bank = _bank(rng, N, P, D)
    q, W = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, Q, D)
    bd, qd, Wd = _cuda(bank, q, W)
    stats = {}
    got = search.cosine_topk_tokens(qd, bd, k, "min", weights=Wd, stats=stats)
    assert stats["group"] == g and stats["groups"] == -(-Q // g)
    s = pq.token_scores_pq(q, bank, W)
    _equal(got, pq.topk_of_token_scores(s, k, "min"), (Q, D, k))
    assert np.array_equal(search.cosine_token_scores(qd, bd, "min", weights=Wd).cpu().numpy(), pq.combine(s, "min"))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("P", (4, 16, 32))
@pytest.mark.parametrize("metric", tdr.METRICS)
def test_distance_per_query_weights_are_the_single_weight_calls(metric, P, dtype):
    """The [Q, D] call equals Q single-weight calls (the existing entry point, weights=row) bit for bit, and each of those equals
    tests/token_distance_reference.py.  top_t, a selection and the scores call ride along."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(26 + P)
    N, D, Q, k = 531, 192, 5, 100
    bank_t, bank = _bank(rng, N, P, D, dtype)
    q, W = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, Q, D)
    flags = rng.random(N) < 0.5
    bd, (qd, Wd) = bank_t.cuda(), _cuda(q, W)
    sel = search.Selection(torch.from_numpy(flags))
    for combine, t, fl, s_ in (("mean", None, None, None), ("min", None, flags, sel), ("max", 3, None, None), ("mean", 3, flags, sel)):
        stats = {}
        got = search.distance_topk_tokens(qd, bd, k, metric, combine, weights=Wd, top_t=t, select=s_, stats=stats)
        assert stats["per_query_weights"] is True and stats["group"] == 16
        sc = search.distance_token_scores(qd, bd, metric, combine, weights=Wd, top_t=t, select=s_)
        for i in range(Q):
            one = search.distance_topk_tokens(qd[i:i + 1], bd, k, metric, combine, weights=Wd[i], top_t=t, select=s_)
            assert torch.equal(one[1][0], got[1][i]) and torch.equal(one[0][0], got[0][i]), (combine, t, i)
            assert torch.equal(search.distance_token_scores(qd[i:i + 1], bd, metric, combine, weights=Wd[i], top_t=t, select=s_)[0], sc[i])
            c = search.prepare_distance_weights(Wd[i], D, torch.device("cuda")).cpu().numpy()
            _equal(one, tdr.distance_topk_tokens(c, q[i:i + 1], bank, k, metric, combine, t, fl), (combine, t, i))


def test_flat_bank_with_per_query_weights_is_the_token_search_with_one_token_per_row():
    from sky_embeddings_amd import search
    rng = np.random.default_rng(27)
    N, D, Q, k = 3001, 192, 5, 100
    bank = rng.standard_normal((N, D), dtype=np.float32)
    q, W = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, Q, D)
    bd, qd, Wd = _cuda(bank, q, W)
    stats = {}
    got = search.cosine_topk(qd, bd, k, weights=Wd, stats=stats)
    assert stats["path"] == "tokens" and stats["per_query_weights"] is True
    tok = search.cosine_topk_tokens(qd, bd.unsqueeze(1), k, "min", weights=Wd)
    assert torch.equal(got[0], tok[0]) and torch.equal(got[1], tok[1])
    _equal(got, pq.topk_tokens_pq(q, bank[:, None], k, "min", W), "flat")
    with pytest.raises(ValueError, match="PreparedBank"):
        search.cosine_topk(qd, search.PreparedBank(bd), k, weights=Wd)


def test_refusals_come_before_any_launch():
    """Argument checks that return before hipLaunchKernelGGL: the LDS rule, a misaligned w / c, a wrong weight shape."""
    from sky_embeddings_amd import _lib, ops, search
    L = _lib.lib()
    assert L.skyemb_cosine_token_pq_applicable(16, 4, 768, 100) == 1
    assert L.skyemb_cosine_token_pq_applicable(16, 4, 768, 300) == 0
    text = L.skyemb_last_error().decode()
    assert "D=768" in text and "Q=16" in text and "k=300" in text and "128 D + 32 Q k" in text
    rng = np.random.default_rng(28)
    N, P, D, Q, k = 2003, 4, 64, 5, 10
    bd, qd, Wd = _cuda(rng.standard_normal((N, P, D), dtype=np.float32), rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, Q, D))
    tw, qn = search.prepare_queries_pq(qd, Wd)
    off = torch.empty(Q * D + 1, device="cuda")[1:].view(Q, D)              # 4 bytes past a 16-byte boundary
    off.copy_(Wd)
    assert off.data_ptr() % 16 == 4
    out = torch.full((Q, N), 7.0, device="cuda")
    with pytest.raises(_lib.SkyembError, match="w must be 16-byte aligned"):
        ops.cosine_token_scores_pq(tw, qn, bd, off, _lib.COMBINE_MIN, 1e-6, out)
    nl = ops.cosine_token_topk_chunks(N, P, Q, D, k)
    ps, pi = torch.full((Q, nl, k), 7.0, device="cuda"), torch.full((Q, nl, k), 7, device="cuda", dtype=torch.int64)
    with pytest.raises(_lib.SkyembError, match="w must be 16-byte aligned"):
        ops.cosine_token_topk_pq(tw, qn, bd, off, k, _lib.COMBINE_MIN, 1e-6, 0, nl, ps, pi)
    with pytest.raises(_lib.SkyembError, match="c and t must be 16-byte aligned"):
        ops.distance_token_scores_pq(off, qd, bd, _lib.METRIC_MAE, _lib.COMBINE_MEAN, out)
    with pytest.raises(_lib.SkyembError, match="128 D"):
        ops.cosine_token_topk_pq(tw, qn, bd, Wd, 513, _lib.COMBINE_MIN, 1e-6, 0, nl, ps, pi)
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((ps == 7).all()) and bool((pi == 7).all())         # nothing ran
    calls = (lambda w: search.cosine_topk_tokens(qd, bd, k, weights=w), lambda w: search.cosine_token_scores(qd, bd, weights=w),
             lambda w: search.distance_topk_tokens(qd, bd, k, weights=w), lambda w: search.distance_token_scores(qd, bd, weights=w),
             lambda w: search.cosine_topk(qd, bd[:, 0].contiguous(), k, weights=w, select=torch.ones(N, dtype=torch.bool)))
    for bad in (Wd[:4], Wd[:, :32], Wd[None], torch.ones(D + 64, device="cuda")):     # leading dimension, D, rank, D of a vector
        for call in calls:
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(tuple(bad.shape)) in str(e.value) and f"({Q}, {D})" in str(e.value)
    with pytest.raises(ValueError, match="128 D"):                           # no group size fits (k > 512): the library's text
        search.cosine_topk_tokens(torch.zeros(2, 1024, device="cuda"), torch.zeros(600, 1, 1024, device="cuda"), 513,
                                  weights=torch.ones(2, 1024, device="cuda"))


def _run_cli(work, dd, targets, name, *extra):
    out = subprocess.run([sys.executable, str(work / "similarity_search.py"), "mim_t", "-tgt_fn", "targets.h5", "-tst_fn", "test.h5", "-tgt_i",
                          targets, "-aug", "False", "-snr", "[-1e30,1e30]", "-bs", "16", "-ns", "21", "-dd", str(dd), "--bank", "-mp",
                          "False", "-ct", "False", *extra],
                         cwd=str(work), env=dict(os.environ, PYTHONPATH=str(work)), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return dict(np.load(str(work / "results" / f"mim_t_targets_simsearch_results_{name}.npz")))


def test_cli_per_target_rows_are_the_single_target_runs(tmp_path):
    """similarity_search.py --bank --per-target with two targets over 64 synthetic test images and a tiny ViT, each run a fresh
    child process: the npz has the leading target axis and row t is the --bank run with -tgt_i [t] alone -- the same images in
    the same order, scores within the shared-versus-per-query bound of tests/token_pq_reference.py (that run scores with the
    bank norms of ONE weight vector).  -ns is 21 and the first 20 are compared, so the cut lies inside the saved scores: the
    single-target scores must be further apart than twice the bound at every position, or the orders could differ legitimately
    (asserted, on those saved scores, before anything is compared)."""
    from sky_embeddings_amd import hdf5_lite
    from sky_embeddings_amd.utils.mim_vit import build_model as build_mae
    dd = tmp_path / "data"
    dd.mkdir()
    hdf5_lite.make_synthetic_cutouts(str(dd / "targets.h5"), n=8, seed=5)
    hdf5_lite.make_synthetic_cutouts(str(dd / "test.h5"), n=64, seed=6)
    work = tmp_path / "work"
    (work / "configs").mkdir(parents=True)
    (work / "models").mkdir()
    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(ROOT, "configs", "mim_1.ini"))
    cfg["TRAINING"]["compute_dtype"] = "f32"
    with open(work / "configs" / "mim_t.ini", "w") as fh:
        cfg.write(fh)
    torch.manual_seed(20262)
    mae, _, _ = build_mae(cfg, str(tmp_path / "none.pth.tar"), torch.device("cuda"))
    torch.save({"batch_iters": 1, "losses": {}, "model": {k: v.cpu() for k, v in mae.module.state_dict().items()}}, str(work / "models" / "mim_t.pth.tar"))
    Dw = int(cfg["ARCHITECTURE"]["embed_dim"])
    del mae
    for name in ("similarity_search.py", "utils", "sky_embeddings_amd"):
        os.symlink(os.path.join(ROOT, name), work / name)
    both = _run_cli(work, dd, "[2,5]", "per_target", "--per-target")
    assert both["test_scores"].shape == (2, 21) and both["test_ra_decs"].shape[:2] == (2, 21)
    assert both["test_images"].shape[:2] == (2, 21) and both["test_features"].shape[:2] == (2, 21)
    assert both["target_images"].shape[0] == 2
    assert not (work / "results" / "mim_t_targets_simsearch_results_f.npz").exists()         # the plain output file is not written
    tol = pq.shared_bound(Dw, "min")
    for t, target in enumerate((2, 5)):
        one = _run_cli(work, dd, f"[{target}]", "f")
        assert one["test_scores"].shape == (21,)
        gaps = -np.diff(one["test_scores"].astype(np.float64))
        print("target", target, "smallest gap", gaps.min(), "bound", tol, "max |delta|", np.abs(one["test_scores"] - both["test_scores"][t]).max())
        assert (gaps > 2 * tol).all(), (target, gaps.min())                   # no tie at any position, the cut included
        assert (np.abs(one["test_scores"][:20].astype(np.float64) - both["test_scores"][t, :20]) <= tol).all(), target
        assert np.array_equal(one["test_ra_decs"][:20], both["test_ra_decs"][t, :20], equal_nan=True), target
        assert np.array_equal(one["test_images"][:20], both["test_images"][t, :20], equal_nan=True), target
    assert not np.array_equal(both["test_ra_decs"][0], both["test_ra_decs"][1])            # two targets, two answers
