"""CPU: the weighted MSE / MAE patch-token search's restatement (tests/token_distance_reference.py) against the reference goldens
(tests/golden/similarity_distance.npz, written by the reference's compute_similarity), its documented rules, and every refusal of
the library and of the Python layer -- none of which needs a GPU."""
import os

import numpy as np
import pytest
import torch

from tests import token_distance_reference as tdr
from sky_embeddings_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "similarity_distance.npz")
CASES = ((40, 1, 200), (33, 4, 64), (33, 16, 48))
D = 64


def golden_cases():
    """(key, P, bank, avg, c by use_weights, {(metric, combine, uw, t): golden}) per case, t None for 'all'."""
    z = np.load(GOLDEN)
    for (T, P, N) in CASES:
        key = f"dist/{T}_{P}_{N}"
        want = {}
        for name in z.files:
            if name.startswith(key + "/M"):
                metric, combine, uw, t = name[len(key) + 1:].split("_")
                want[(metric, combine, int(uw), None if t == "tall" else int(t[1:]))] = z[name]
        yield key, P, z[key + "/test"], z[key + "/avg"], {1: tdr.prepare_c(z[key + "/w"], D), 0: tdr.prepare_c(None, D)}, want


def golden_tolerance(combine, count):
    """Relative: the contract's derived bound against the exact formula (tdr.distance_bound), plus the same for torch's result,
    whose summation order is unspecified: D * 2^-24 is the allowance for that (any order of D non-negative terms, its own roundings
    of a term included, stays within it at D = 64)."""
    return tdr.distance_bound(D, combine, count) + D * tdr.U


def test_restatement_matches_every_golden_array():
    n = 0
    for key, P, bank, avg, cs, want in golden_cases():
        assert bank.shape[2] == D and bank.dtype == np.float32
        for metric in tdr.METRICS:
            for uw in (1, 0):
                a = tdr.token_distances(cs[uw], avg[None], bank, metric)
                exact = tdr.exact_token_distances(cs[uw], avg[None], bank, metric)
                # the bound as derived, against the fp64 formula from the same inputs
                assert (np.abs(a - exact) <= tdr.distance_bound(D) * exact).all(), (key, metric, uw)
                for (m, combine, u, t), gold in want.items():
                    if m != metric or u != uw:
                        continue
                    got = tdr.combine_distances(a, combine, t)[0]
                    tol = golden_tolerance(combine, P if t is None else t)
                    assert got.shape == gold.shape and (np.abs(got.astype(np.float64) - gold) <= tol * gold).all(), (key, m, combine, u, t)
                    n += 1
    assert n == 120


def test_golden_file_is_data_of_the_documented_shape():
    z = np.load(GOLDEN)
    assert len(z.files) == 129 and os.path.getsize(GOLDEN) < 512 * 1024
    for (T, P, N) in CASES:
        assert z[f"dist/{T}_{P}_{N}/test"].shape == (N, P, D) and z[f"dist/{T}_{P}_{N}/MAE_mean_1_tall"].shape == (N,)


def test_planted_nan_and_inf_follow_the_documented_rule():
    rng = np.random.default_rng(1)
    N, P = 12, 4
    bank = rng.standard_normal((N, P, D), dtype=np.float32)
    bank[3, 1, 5] = np.nan                                       # one NaN token
    bank[5, 2, 9] = np.inf                                       # one +inf token distance
    bank[7] = np.nan                                             # no finite token at all
    bank[9, :3, 0] = np.nan                                      # one finite token left
    q, c = rng.standard_normal((2, D), dtype=np.float32), tdr.prepare_c(rng.random(D, dtype=np.float32) + 0.1, D)
    for metric in tdr.METRICS:
        a = tdr.token_distances(c, q, bank, metric)
        assert np.isnan(a[:, 3, 1]).all() and np.isposinf(a[:, 5, 2]).all()
        clean = np.where(np.isnan(a), np.inf, a)
        mn = tdr.combine_distances(a, "min")
        assert np.array_equal(mn[:, [3, 5, 9]], clean.min(axis=2)[:, [3, 5, 9]]) and np.isfinite(mn[:, [3, 5, 9]]).all()   # ignored by min
        assert np.isposinf(mn[:, 7]).all()
        for combine in ("max", "mean"):
            assert np.isposinf(tdr.combine_distances(a, combine)[:, [3, 5, 7, 9]]).all()                 # +inf under max and mean
        for combine in tdr.COMBINES:                             # top_t = 3: images 3 and 5 have three finite tokens, 9 has one
            s = tdr.combine_distances(a, combine, 3)
            assert np.isfinite(s[:, [3, 5]]).all() and np.isposinf(s[:, 7]).all()
            assert np.isfinite(s[:, 9]).all() == (combine == "min")
            ds, di = tdr.topk_of_distances(s, N)
            assert 7 not in di and (9 in di[0]) == (combine == "min")                                    # +inf images are never returned
            n_ok = int(np.isfinite(s[0]).sum())
            assert (di[:, n_ok:] == -1).all() and np.isposinf(ds[:, n_ok:]).all() and (np.diff(ds[:, :n_ok]) >= 0).all()


def test_top_t_equal_to_p_differs_from_the_plain_mean_by_order_only():
    rng = np.random.default_rng(2)
    for P in (4, 16):
        bank, q = rng.standard_normal((50, P, D), dtype=np.float32), rng.standard_normal((3, D), dtype=np.float32)
        a = tdr.token_distances(tdr.prepare_c(None, D), q, bank, "MAE")
        plain, top = tdr.combine_distances(a, "mean"), tdr.combine_distances(a, "mean", P)
        exact = a.astype(np.float64).mean(axis=2)
        for got in (plain, top):                                 # both are the same sum: P - 1 roundings and one division
            assert (np.abs(got - exact) <= tdr.gamma(P) * exact).all()
        assert not np.array_equal(plain, top)                    # ... in another order
        for combine in ("min", "max"):                           # while min and max at top_t == P are the plain ones, bit for bit
            assert np.array_equal(tdr.combine_distances(a, combine), tdr.combine_distances(a, combine, P))


def test_restatement_order_is_the_documented_one():
    """One row by hand: 16 partials over (d >> 2) & 15, ascending d, the folds 8, 4, 2, 1, one division."""
    rng = np.random.default_rng(3)
    Dw = 128
    x, t = rng.standard_normal(Dw, dtype=np.float32), rng.standard_normal(Dw, dtype=np.float32)
    c = tdr.prepare_c(rng.random(Dw, dtype=np.float32) + 0.1, Dw)
    for metric in tdr.METRICS:
        p = [np.float32(0)] * 16
        for d in range(Dw):
            diff = np.float32(x[d] - t[d])
            v = np.float32(abs(diff)) if metric == "MAE" else np.float32(diff * diff)
            p[(d >> 2) & 15] = np.float32(p[(d >> 2) & 15] + np.float32(c[d] * v))
        for f in (8, 4, 2, 1):
            p = [np.float32(p[j] + p[j ^ f]) for j in range(16)]
        assert len(set(float(v) for v in p)) == 1
        assert tdr.token_distances(c, t[None], x[None, None], metric)[0, 0, 0] == np.float32(p[0] / np.float32(Dw))


def test_selection_is_the_compacted_bank():
    rng = np.random.default_rng(4)
    N, P = 37, 4
    bank, q, c = rng.standard_normal((N, P, D), dtype=np.float32), rng.standard_normal((2, D), dtype=np.float32), tdr.prepare_c(None, D)
    flags = rng.random(N) < 0.5
    a = tdr.token_distances(c, q, bank, "MSE")
    for combine, t in (("min", None), ("mean", 3), ("max", 2)):
        s1 = tdr.topk_of_token_distances(a, 30, combine, t, flags, idx_offset=5)
        s2 = tdr.distance_topk_tokens(c, q, bank, 30, "MSE", combine, t, flags, idx_offset=5)
        assert np.array_equal(s1[0], s2[0]) and np.array_equal(s1[1], s2[1])
        assert set(s1[1][0][s1[1][0] >= 0] - 5) == set(np.nonzero(flags)[0])
        sc = tdr.scores_of_token_distances(a, combine, t, flags)
        assert np.isposinf(sc[:, ~flags]).all() and np.isfinite(sc[:, flags]).all()


def test_entry_points_are_exported_and_refuse_bad_calls_before_any_launch():
    """The library loads without a GPU; argument validation comes before any device work."""
    L = _lib.lib()
    assert L.skyemb_version() == _lib.ABI_VERSION == 111
    for name in ("skyemb_distance_token_scores", "skyemb_distance_token_topk"):
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    assert (_lib.METRIC_MSE, _lib.METRIC_MAE) == (1, 2)
    buf = np.zeros(256, np.float32).ctypes.data           # a host address: no call below may get as far as reading it

    def err(rc):
        assert rc != 0
        return L.skyemb_last_error()

    def topk(dt=_lib.F32, P=4, Dw=64, metric=2, combine=1, top_t=2, bank=buf, sel=buf, c=buf, t=buf, nl=None, k=5, Q=1):
        if nl is None:
            nl = L.skyemb_cosine_token_topk_chunks(10, P, Q, Dw, k)       # 0 for a shape that is refused anyway
        return L.skyemb_distance_token_topk(c, t, bank, dt, Q, 10, P, Dw, metric, combine, top_t, k, 0, nl, None, buf, buf, sel, None)

    def scores(dt=_lib.F32, P=4, Dw=64, metric=2, combine=1, top_t=2, bank=buf, sel=buf, c=buf, t=buf, Q=1):
        return L.skyemb_distance_token_scores(c, t, bank, dt, Q, 10, P, Dw, metric, combine, top_t, buf, sel, None)

    for call, who in ((topk, b"skyemb_distance_token_topk"), (scores, b"skyemb_distance_token_scores")):
        for dt in (_lib.F32, _lib.F16, _lib.BF16):
            for top_t, P in ((-1, 4), (17, 4), (5, 4), (17, 64)):
                assert f"top_t={top_t} P={P}".encode() in err(call(dt=dt, P=P, top_t=top_t))
            for metric in (0, 3, -1):
                msg = err(call(dt=dt, metric=metric))
                assert b"metric must be" in msg and who in msg, msg
            assert b"unknown combine" in err(call(dt=dt, combine=7))
            msg = err(call(dt=dt, P=9))
            assert b"16 % P == 0" in msg and who in msg, msg
            assert b"D % 64 == 0" in err(call(dt=dt, Dw=96)) and b"Q <= 16" in err(call(dt=dt, Q=17))
            assert b"bad arguments" in err(call(dt=dt, bank=None)) and b"bad arguments" in err(call(dt=dt, c=None))
            for off in (1, 2, 3):
                assert b"select must be 4-byte aligned" in err(call(dt=dt, sel=buf + off))
            for what in ("bank", "c", "t"):
                assert b"16-byte aligned" in err(call(dt=dt, **{what: buf + 4}))
        for dt in (3, 7, -1):
            msg = err(call(dt=dt))
            assert b"bank_dtype must be" in msg and str(dt).encode() in msg, msg
    assert b"nlists must come from" in err(topk(nl=3))
    assert b"k <= 512" in err(topk(k=513))


def test_python_layer_raises_before_any_device_work():
    from sky_embeddings_amd import ops, search
    assert ops.METRIC_CODES == {"MSE": _lib.METRIC_MSE, "MAE": _lib.METRIC_MAE}
    bank, q = torch.zeros(8, 4, 64), torch.zeros(1, 64)
    both = (lambda **kw: search.distance_topk_tokens(q, bank, kw.pop("k", 2), **kw), lambda **kw: (kw.pop("k", 0), search.distance_token_scores(q, bank, **kw)))
    for call in both:
        for metric in ("cosine", "mae", None):
            with pytest.raises(ValueError, match="metric = "):
                call(metric=metric)
        with pytest.raises(ValueError, match="combine = "):
            call(combine="median")
        for top_t in (0, 5, 17, 1.5, True):
            with pytest.raises(ValueError, match="top_t = "):
                call(top_t=top_t)
        for bad in (torch.ones(7, dtype=torch.bool), torch.ones(9, dtype=torch.bool)):
            with pytest.raises(ValueError, match="select describes"):
                call(select=bad)
    for k in (0, -1, 9):
        with pytest.raises(ValueError, match="k = "):
            search.distance_topk_tokens(q, bank, k)
    with pytest.raises(ValueError, match="k <= 512"):
        search.distance_topk_tokens(q, torch.zeros(600, 4, 64), 513)
    with pytest.raises(ValueError, match="D % 64 == 0"):
        search.distance_token_scores(torch.zeros(1, 96), torch.zeros(8, 4, 96))
    with pytest.raises(ValueError, match="16 % P == 0"):
        search.distance_topk_tokens(q, torch.zeros(8, 3, 64), 2)
    with pytest.raises(ValueError, match="bank dtype"):
        search.distance_topk_tokens(q, torch.zeros(8, 4, 64, dtype=torch.float64), 2)


def test_cli_takes_the_distance_metrics_with_bank(monkeypatch):
    """--bank no longer refuses -m MSE / MAE; an unknown metric name exits with a message before anything is loaded."""
    import similarity_search
    monkeypatch.setattr("sys.argv", ["similarity_search.py", "m", "--bank", "-m", "L1"])
    with pytest.raises(SystemExit) as e:
        similarity_search.main()
    assert "L1" in str(e.value) and "MAE" in str(e.value)
