"""GPU: the weighted MSE / MAE patch-token search (search.distance_topk_tokens / distance_token_scores, kernels in
csrc/distance_tokens.hip) against the CPU restatement (tests/token_distance_reference.py), bit for bit: np.array_equal on
distances and on indices, everywhere except the two tests that compare with torch's own arithmetic (the reference goldens and
the streamed CLI path), which use the bound derived in the restatement's docstring.

Shapes are the smallest at which each mechanism can break: N in {37, 531, 4099} (the mask's tail word; a ragged last tile; more
than one workgroup and a short last wave range), P on both sides of the 16-row tile and across tiles, D = 64 (one float4 step per
lane) and 192 (three: an odd number of steps per four-load block)."""
import configparser
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import token_distance_reference as tdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS, NS, QS, KS = (1, 4, 16, 32), (37, 531, 4099), (1, 5, 16), (1, 7, 100)
LP = (torch.float16, torch.bfloat16)


def _weights(rng, D):
    return rng.random(D, dtype=np.float32) + 0.1


def _cuda(*arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


def _c(wd, D):
    """The library's own c = fp32(w / sum(w)) (torch on the device), read back: the restatement starts from the same bits."""
    from sky_embeddings_amd import search
    return search.prepare_distance_weights(wd, D, torch.device("cuda")).cpu().numpy()


def _top_ts(P):
    return [t for t in (None, 1, 3, 16) if t is None or t <= min(P, 16)]


def _masks(N, seed):
    """name -> bool [N], or None for a search without a selection."""
    rng = np.random.default_rng(seed)
    i = np.arange(N)
    m = {"none": None, "ones": np.ones(N, bool), "zeros": np.zeros(N, bool), "bernoulli_0.5": rng.random(N) < 0.5,
         "bernoulli_0.05": rng.random(N) < 0.05}
    for at in (0, 31, 32, N - 1):
        m[f"one_at_{at}"] = i == at
    return m


def _equal(got, ref, tag):
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(gi, ref[1]), tag
    assert np.array_equal(gs, ref[0]), tag


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("P", PS)
def test_distance_search_bit_exact(P, N):
    """Every mask x every combine x every Q on an fp32 bank; the metric, k, top_t and prune rotate through their values over the 81
    searches of a case (n = 9 m + 3 c + i for mask m, combine c, query count QS[i]: metric = n % 2; k = KS[(i + c + m) % 3], so
    every (Q, k, combine) occurs; top_t walks its values once per three searches; prune alternates in pairs).  D = 64 or 192 by
    case.  The token distances of the whole bank are computed once per metric for 16 queries.  A NaN token, a +inf token
    distance and equal images at both ends are planted."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(2000 * P + N)
    D = (64, 192)[(PS.index(P) + NS.index(N)) % 2]
    bank = rng.standard_normal((N, P, D), dtype=np.float32)
    bank[N // 3, P // 2, 5] = np.nan                             # a NaN token in an image that most masks select
    bank[N // 2, 0, 70 % D] = np.inf                             # a +inf token distance
    bank[N - 1] = bank[0]                                        # equal images at both ends
    q, w = rng.standard_normal((16, D), dtype=np.float32), _weights(rng, D)
    bd, qd, wd = _cuda(bank, q, w)
    c = _c(wd, D)
    a = {m: tdr.token_distances(c, q, bank, m) for m in tdr.METRICS}
    tb = search.TokenBank(bd, wd, idx_offset=7)
    tts, n = _top_ts(P), 0
    for name, flags in _masks(N, P + N).items():
        sel = None if flags is None else search.Selection(torch.from_numpy(flags))
        for combine, Q in [(cb, Q) for cb in tdr.COMBINES for Q in QS]:
            metric = tdr.METRICS[n % 2]
            k, t, prune = min(KS[(n + n // 3 + n // 9) % 3], N), tts[(n // 3) % len(tts)], bool((n // 2) % 2)
            n += 1
            tag = (P, N, D, name, metric, combine, Q, k, t, prune)
            ref = tdr.topk_of_token_distances(a[metric][:Q], k, combine, t, flags, idx_offset=7)
            stats = {}
            got = search.distance_topk_tokens(qd[:Q], tb, k, metric, combine, prune=prune, stats=stats, top_t=t, select=sel)
            assert stats["path"] == "tokens" and stats["metric"] == metric and (sel is None or stats["selected"] == sel.count)
            _equal(got, ref, tag)
            sc = search.distance_token_scores(qd[:Q], tb, metric, combine, top_t=t, select=sel).cpu().numpy()
            assert np.array_equal(sc, tdr.scores_of_token_distances(a[metric][:Q], combine, t, flags)), tag
            if name == "ones":                                   # the select=None result, bit for bit
                plain = search.distance_topk_tokens(qd[:Q], tb, k, metric, combine, prune=prune, top_t=t)
                assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), tag
            if name == "zeros":
                assert bool((got[1] == -1).all()) and bool(torch.isposinf(got[0]).all()) and np.isposinf(sc).all(), tag
            if name == "bernoulli_0.05" and k > int(flags.sum()):       # k above the selected count: the (+inf, -1) tail
                cnt = int(np.isfinite(ref[0][0]).sum())
                assert cnt <= int(flags.sum()) < k and bool((got[1][:, cnt:] == -1).all()) and bool(torch.isposinf(got[0][:, cnt:]).all()), tag
            if name.startswith("one_at"):
                assert bool((got[1][:, 1:] == -1).all()), tag


@pytest.mark.parametrize("dtype", LP)
@pytest.mark.parametrize("P", (4, 32))
def test_16_bit_bank_is_the_fp32_call_on_the_widened_bank(P, dtype):
    from sky_embeddings_amd import search
    rng = np.random.default_rng(300 + P)
    N, D, Q, k = 531, 192, 5, 100
    bank16 = torch.from_numpy(rng.standard_normal((N, P, D), dtype=np.float32)).to(dtype)
    bank16[7, P // 2, 3] = float("nan")
    wide = bank16.to(torch.float32)
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    qd, wd = _cuda(q, w)
    c = _c(wd, D)
    flags = _masks(N, 5)["bernoulli_0.5"]
    b16, b32 = bank16.cuda(), wide.cuda()
    for metric in tdr.METRICS:
        a = tdr.token_distances(c, q, wide.numpy(), metric)
        for combine, t, fl in (("min", None, None), ("mean", None, flags), ("max", 3, None), ("mean", 3, flags)):
            sel = None if fl is None else torch.from_numpy(fl)
            got = search.distance_topk_tokens(qd, b16, k, metric, combine, weights=wd, top_t=t, select=sel)
            _equal(got, tdr.topk_of_token_distances(a, k, combine, t, fl), (P, dtype, metric, combine, t))
            g32 = search.distance_topk_tokens(qd, b32, k, metric, combine, weights=wd, top_t=t, select=sel)
            assert torch.equal(got[0], g32[0]) and torch.equal(got[1], g32[1])
            sc = search.distance_token_scores(qd, b16, metric, combine, weights=wd, top_t=t, select=sel)
            assert torch.equal(sc, search.distance_token_scores(qd, b32, metric, combine, weights=wd, top_t=t, select=sel))
            assert np.array_equal(sc.cpu().numpy(), tdr.scores_of_token_distances(a, combine, t, fl))


def test_17_queries_run_as_two_groups_and_without_weights():
    """Q = 17 through the Python API, weights=None (w = 1): per query the result of a Q = 1 call."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(17)
    Q, N, P, D, k = 17, 531, 16, 64, 7
    bank, q = rng.standard_normal((N, P, D), dtype=np.float32), rng.standard_normal((Q, D), dtype=np.float32)
    bd, qd = _cuda(bank, q)
    c = _c(None, D)
    assert np.array_equal(c, tdr.prepare_c(None, D))
    for metric, combine, t in (("MAE", "mean", None), ("MSE", "max", 3)):
        a = tdr.token_distances(c, q, bank, metric)
        stats = {}
        got = search.distance_topk_tokens(qd, bd, k, metric, combine, stats=stats, top_t=t)
        assert stats["groups"] == 2 and stats["pruned"] is False
        _equal(got, tdr.topk_of_token_distances(a, k, combine, t), (metric, combine, t))
        assert np.array_equal(search.distance_token_scores(qd, bd, metric, combine, top_t=t).cpu().numpy(), tdr.combine_distances(a, combine, t))
        for j in (0, 15, 16):
            one = search.distance_topk_tokens(qd[j:j + 1], bd, k, metric, combine, top_t=t)
            assert torch.equal(one[0][0], got[0][j]) and torch.equal(one[1][0], got[1][j])


def test_exact_ties_go_to_the_lower_index():
    """Duplicated images inside one tile (P = 4) and across tiles (P = 16), some of them deselected.  The duplicates are tokens
    close to the query (0.1 sigma around it, every other token is a sigma and more away), so under every metric and combine they
    are the best images and their run opens the list."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(9)
    for P in (4, 16):
        N, D = 531, 64
        bank = rng.standard_normal((N, P, D), dtype=np.float32)
        dup = (1, 2, 3, 40, 41, 300, N - 1)
        q, w = rng.standard_normal((1, D), dtype=np.float32), _weights(rng, D)
        bank[1] = q + np.float32(0.1) * rng.standard_normal((P, D), dtype=np.float32)
        for j in dup[1:]:
            bank[j] = bank[1]
        flags = np.ones(N, bool)
        flags[[2, 41, 5, 299]] = False
        bd, qd, wd = _cuda(bank, q, w)
        c = _c(wd, D)
        for metric in tdr.METRICS:
            for combine in tdr.COMBINES:
                for fl in (None, flags):
                    ref = tdr.distance_topk_tokens(c, q, bank, 10, metric, combine, None, fl)
                    got = search.distance_topk_tokens(qd, bd, 10, metric, combine, weights=wd, select=None if fl is None else torch.from_numpy(fl))
                    _equal(got, ref, (P, metric, combine))
                    gi = got[1][0].cpu().tolist()
                    kept = [j for j in dup if fl is None or fl[j]]
                    assert gi[:len(kept)] == kept, (P, metric, combine, gi)


@pytest.mark.parametrize("P", (4, 16, 32))
def test_nan_and_inf_in_selected_and_in_deselected_images(P):
    """Deselected images filled with NaN and +-inf change nothing; in selected images a NaN / +inf token follows the documented
    rule: ignored by min, +inf under max and mean, and under top_t once fewer than top_t finite tokens are left."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(60 + P)
    N, D, Q, k = 531, 64, 5, 100
    clean = rng.standard_normal((N, P, D), dtype=np.float32)
    q, w = rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    qd, wd = _cuda(q, w)
    c = _c(wd, D)
    flags = _masks(N, P)["bernoulli_0.5"]
    keep = np.nonzero(flags)[0]
    bank = clean.copy()
    bank[keep[3], P // 2, 7] = np.nan                            # one NaN token
    bank[keep[5], 0, 9] = np.inf                                 # one +inf token distance
    bank[keep[8], : P - 1] = np.nan                              # one finite token left
    bad = bank.copy()
    bad[~flags] = np.nan
    bad[~flags, 0::2, 1::3] = np.inf
    bad[~flags, 1::2, 0::3] = -np.inf
    sel = search.Selection(torch.from_numpy(flags))
    b_ok, b_bad = _cuda(bank, bad)
    for metric in tdr.METRICS:
        a = tdr.token_distances(c, q, bank, metric)
        for combine in tdr.COMBINES:
            for t in (None, 3):
                ref = tdr.topk_of_token_distances(a, k, combine, t, flags)
                sref = tdr.scores_of_token_distances(a, combine, t, flags)
                assert np.isposinf(sref[:, keep[8]]).all() == (combine != "min")
                if t is None:
                    assert np.isposinf(sref[:, keep[3]]).all() == (combine != "min") and np.isposinf(sref[:, keep[5]]).all() == (combine != "min")
                got = search.distance_topk_tokens(qd, b_bad, k, metric, combine, weights=wd, top_t=t, select=sel)
                _equal(got, ref, (P, metric, combine, t))
                ok = search.distance_topk_tokens(qd, b_ok, k, metric, combine, weights=wd, top_t=t, select=sel)
                assert torch.equal(got[0], ok[0]) and torch.equal(got[1], ok[1])
                sc = search.distance_token_scores(qd, b_bad, metric, combine, weights=wd, top_t=t, select=sel)
                assert np.array_equal(sc.cpu().numpy(), sref)
                assert torch.equal(sc, search.distance_token_scores(qd, b_ok, metric, combine, weights=wd, top_t=t, select=sel))


# The floor exists from 8 x 256 x k images on: k = 1 gives 2048, so N = 2100 engages it for the whole bank and, with 40 images
# deselected, for the selection; N = 2047 is one image short of the rule.
@pytest.mark.parametrize("P,D", [(4, 64), (16, 192)])
def test_pruning_floor_engages_and_changes_nothing(P, D):
    from sky_embeddings_amd import search
    rng = np.random.default_rng(80 + P)
    N, Q, k = 2100, 5, 1
    bank, q, w = rng.standard_normal((N, P, D), dtype=np.float32), rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    flags = np.ones(N, bool)
    flags[rng.choice(N, 40, replace=False)] = False
    bank[~flags] = q[0] + np.float32(1e-3)                       # next to query 0: a floor from the whole bank would shut every selected image out
    bd, qd, wd = _cuda(bank, q, w)
    c = _c(wd, D)
    tb, sel = search.TokenBank(bd, wd), search.Selection(torch.from_numpy(flags))
    for metric, combine, t in (("MAE", "mean", None), ("MSE", "min", None), ("MAE", "max", 2)):
        a = tdr.token_distances(c, q, bank, metric)
        for fl, s in ((None, None), (flags, sel)):
            ref = tdr.topk_of_token_distances(a, k, combine, t, fl)
            floor = search.distance_pruning_floor(torch.from_numpy(c).cuda(), qd, tb, k, metric, combine, top_t=t, select=s)
            assert floor is not None and bool((floor.cpu().numpy() < -ref[0][:, k - 1]).all())      # key space, strictly below the k-th best key
            for prune in (True, False):
                for b in (tb, bd):                               # a TokenBank's kept sample and a plain tensor's gathered one
                    stats = {}
                    got = search.distance_topk_tokens(qd, b, k, metric, combine, weights=wd, prune=prune, stats=stats, top_t=t, select=s)
                    assert stats["pruned"] is prune
                    _equal(got, ref, (P, metric, combine, t, prune))
    stats = {}
    search.distance_topk_tokens(qd, bd[:2047].contiguous(), k, stats=stats)
    assert stats["pruned"] is False


def test_idx_offset_shards_merge_to_the_whole_bank_result():
    """Two shards with idx_offset, their key-space lists merged by skyemb_topk_merge as the sharded path does, then negated."""
    from sky_embeddings_amd import ops, search
    rng = np.random.default_rng(11)
    N, P, D, Q, k = 531, 4, 64, 5, 100
    bank, q, w = rng.standard_normal((N, P, D), dtype=np.float32), rng.standard_normal((Q, D), dtype=np.float32), _weights(rng, D)
    bank[400] = bank[100]                                        # a tie across the shards
    bd, qd, wd = _cuda(bank, q, w)
    cut = 301
    flags = _masks(N, 11)["bernoulli_0.5"]
    for metric, combine, fl in (("MAE", "mean", None), ("MSE", "min", flags)):
        whole = search.distance_topk_tokens(qd, bd, k, metric, combine, weights=wd, select=None if fl is None else torch.from_numpy(fl))
        parts = []
        for lo, hi in ((0, cut), (cut, N)):
            tb = search.TokenBank(bd[lo:hi].contiguous(), wd, idx_offset=lo)
            parts.append(search.distance_topk_tokens(qd, tb, k, metric, combine, select=None if fl is None else torch.from_numpy(fl[lo:hi])))
        gs = torch.stack([-p[0] for p in parts], dim=1).contiguous()
        gi = torch.stack([p[1] for p in parts], dim=1).contiguous()
        out_s, out_i = torch.empty(Q, k, device="cuda"), torch.empty(Q, k, device="cuda", dtype=torch.int64)
        ops.topk_merge(gs, gi, Q, 2, k, out_s, out_i)
        assert torch.equal(-out_s, whole[0]) and torch.equal(out_i, whole[1])
        _equal(whole, tdr.distance_topk_tokens(_c(wd, D), q, bank, k, metric, combine, None, fl), (metric, combine))


def test_library_lists_are_in_key_space_with_one_terminator():
    """The raw topk call: every list is keys (= -distance) descending, images ascending among equal keys, ended by ONE (-inf, -1);
    the raw scores call writes distances into every slot of a buffer that held a marker."""
    from sky_embeddings_amd import ops, search
    rng = np.random.default_rng(12)
    Q, N, P, D, k = 3, 531, 16, 64, 7
    bank, q = rng.standard_normal((N, P, D), dtype=np.float32), rng.standard_normal((Q, D), dtype=np.float32)
    bd, qd = _cuda(bank, q)
    cd = search.prepare_distance_weights(None, D, bd.device)
    nl = ops.cosine_token_topk_chunks(N, P, Q, D, k)
    ps, pi = torch.full((Q, nl, k), 7.0, device="cuda"), torch.full((Q, nl, k), 7, device="cuda", dtype=torch.int64)
    ops.distance_token_topk(cd, qd, bd, ops.METRIC_CODES["MAE"], ops.COMBINE_CODES["mean"], k, 1000, nl, ps, pi)
    ps, pi = ps.cpu().numpy(), pi.cpu().numpy()
    want = tdr.combine_distances(tdr.token_distances(cd.cpu().numpy(), q, bank, "MAE"), "mean")
    seen = np.zeros((Q, N), bool)
    for qi in range(Q):
        for l in range(nl):
            term = np.nonzero(pi[qi, l] == -1)[0]
            n_in = int(term[0]) if len(term) else k
            s, i = ps[qi, l, :n_in], pi[qi, l, :n_in] - 1000
            assert (np.diff(s) <= 0).all() and np.array_equal(-s, want[qi, i])
            if n_in < k:
                assert pi[qi, l, n_in] == -1 and np.isneginf(ps[qi, l, n_in]) and (pi[qi, l, n_in + 1:] == 7).all()
            seen[qi, i] = True
    assert seen.any(axis=1).all()
    sc = torch.full((Q, N), 7.0, device="cuda")
    ops.distance_token_scores(cd, qd, bd, ops.METRIC_CODES["MAE"], ops.COMBINE_CODES["mean"], sc)
    assert np.array_equal(sc.cpu().numpy(), want)


def test_reference_goldens_on_the_gpu():
    """compute_similarity's own results (tests/golden/similarity_distance.npz) within the CPU test's bound."""
    from sky_embeddings_amd import search
    from tests.test_token_distance_cpu import D, golden_cases, golden_tolerance
    z = np.load(os.path.join(ROOT, "tests", "golden", "similarity_distance.npz"))
    n = 0
    for key, P, bank, avg, cs, want in golden_cases():
        bd, qd, wd = _cuda(bank, avg[None], z[key + "/w"])
        for (metric, combine, uw, t), gold in want.items():
            got = search.distance_token_scores(qd, bd, metric, combine, weights=wd if uw else None, top_t=t)[0].cpu().numpy()
            tol = golden_tolerance(combine, P if t is None else t)
            assert (np.abs(got.astype(np.float64) - gold) <= tol * gold).all(), (key, metric, combine, uw, t)
            n += 1
    assert n == 120 and D == 64


def _run_cli(work, dd, *extra):
    out = subprocess.run([sys.executable, str(work / "similarity_search.py"), "mim_t", "-tgt_fn", "targets.h5", "-tst_fn", "test.h5", "-tgt_i",
                          "[0,1,2,3]", "-aug", "False", "-snr", "[-1e30,1e30]", "-bs", "16", "-ns", "20", "-dd", str(dd), *extra],
                         cwd=str(work), env=dict(os.environ, PYTHONPATH=str(work)), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    z = np.load(str(work / "results" / "mim_t_targets_simsearch_results_f.npz"))
    return z["test_scores"], z["test_images"]


def test_cli_bank_distance_metrics_agree_with_the_streamed_path(tmp_path):
    """similarity_search.py --bank -m MAE (token bank, -c mean) against the same command without --bank (torch glue on streamed
    batches), each in a fresh child process: the saved distances agree position by position within the derived bound -- the
    contract's (tdr.distance_bound: D / 16 + 8 + P roundings for the mean over P tokens) plus the same allowance for torch's
    unspecified summation order as the golden test takes, D * 2^-24 for a token distance and P * 2^-24 for its mean -- and the
    saved images agree except where neighbouring distances are closer than that.  -m MSE --bank -mp True runs the pooled mode as
    a one-token bank and returns ascending distances."""
    from sky_embeddings_amd import hdf5_lite
    from sky_embeddings_amd.utils.mim_vit import build_model as build_mae
    dd = tmp_path / "data"
    dd.mkdir()
    hdf5_lite.make_synthetic_cutouts(str(dd / "targets.h5"), n=8, seed=5)
    hdf5_lite.make_synthetic_cutouts(str(dd / "test.h5"), n=48, seed=6)
    work = tmp_path / "work"
    (work / "configs").mkdir(parents=True)
    (work / "models").mkdir()
    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(ROOT, "configs", "mim_1.ini"))
    cfg["TRAINING"]["compute_dtype"] = "f32"
    with open(work / "configs" / "mim_t.ini", "w") as fh:
        cfg.write(fh)
    torch.manual_seed(20261)
    mae, _, _ = build_mae(cfg, str(tmp_path / "none.pth.tar"), torch.device("cuda"))
    torch.save({"batch_iters": 1, "losses": {}, "model": {k: v.cpu() for k, v in mae.module.state_dict().items()}}, str(work / "models" / "mim_t.pth.tar"))
    Dw, P = int(cfg["ARCHITECTURE"]["embed_dim"]), mae.module.patch_embed.num_patches
    del mae
    for name in ("similarity_search.py", "utils", "sky_embeddings_amd"):
        os.symlink(os.path.join(ROOT, name), work / name)
    common = ("-m", "MAE", "-mp", "False", "-ct", "False", "-c", "mean")
    bank_s, bank_x = _run_cli(work, dd, "--bank", *common)
    flow_s, flow_x = _run_cli(work, dd, *common)
    assert bank_s.shape == flow_s.shape == (20,) and (np.diff(bank_s) >= 0).all() and (bank_s > 0).all()
    tol = tdr.distance_bound(Dw, "mean", P) + (Dw + P) * tdr.U
    assert (np.abs(bank_s.astype(np.float64) - flow_s) <= tol * flow_s).all(), (bank_s, flow_s, tol)
    for j in range(20):
        if not np.array_equal(np.nan_to_num(bank_x[j]), np.nan_to_num(flow_x[j])):
            near = [abs(float(flow_s[j]) - float(flow_s[i])) <= 2 * tol * flow_s[j] for i in (j - 1, j + 1) if 0 <= i < 20]
            assert any(near), j
    mse_s, _ = _run_cli(work, dd, "--bank", "-m", "MSE", "-mp", "True")
    assert mse_s.shape == (20,) and (np.diff(mse_s) >= 0).all() and np.isfinite(mse_s).all() and (mse_s > 0).all()
