"""CPU: the restatement of the patch-token search with per-query feature weights (tests/token_pq_reference.py) -- its fma chain
pinned to the C oracle, its two derived bounds, the reference goldens with one target -- and the argument validation of the
Python layer and of the `_pq` entry points that needs no device."""
import os

import numpy as np
import pytest
import torch

from oracle import similarity_oracle as so
from tests import token_pq_reference as pq
from tests import token_search_reference as tsr
from tests import token_topt_reference as ttr
from sky_embeddings_amd import _lib, ops, search

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = ((3, 40, 4, 64), (2, 9, 16, 192), (1, 7, 1, 768))            # (Q, N, P, D)


def _data(Q, N, P, D, seed):
    rng = np.random.default_rng(seed)
    q, bank = rng.standard_normal((Q, D), dtype=np.float32), rng.standard_normal((N, P, D), dtype=np.float32)
    W = (rng.random((Q, D), dtype=np.float32) + np.float32(0.05)) * np.exp(rng.standard_normal((Q, D))).astype(np.float32)
    return q, bank, W


def test_the_restated_fma_chain_is_the_oracles_bit_for_bit():
    """``chain`` / ``fma32`` rebuild oracle.similarity_oracle.cosine_scores_np (C fmaf) exactly, bank norm included; fma32 also
    rounds once where a product-then-sum in fp32 or in fp64 would round twice."""
    for n, (Q, N, P, D) in enumerate(SHAPES):
        q, bank, W = _data(Q, N, P, D, 40 + n)
        assert np.array_equal(pq.token_scores_shared(q, bank, W[0]), tsr.token_scores(q, bank, W[0]))
    f = np.float32
    # 1 + 2^-24 + 2^-60: fp64 rounds the sum to the fp32 midpoint 1 + 2^-24, which then ties to even (1); one rounding gives 1 + 2^-23
    assert pq.fma32(f(2.0 ** -30), f(2.0 ** -30), f(1) + f(0)) == f(1)
    a, b, c = f(1 + 2.0 ** -12), f(1 + 2.0 ** -12), f(2.0 ** -60)
    exact_up = pq.fma32(a, b, c)                                  # (1 + 2^-11 + 2^-24) + 2^-60: just above the midpoint
    assert exact_up == np.nextafter(f(1 + 2.0 ** -11), f(2)) and f(np.float64(a) * np.float64(b) + np.float64(c)) == f(1 + 2.0 ** -11)


def test_restatement_is_within_its_bound_of_fp64():
    for n, (Q, N, P, D) in enumerate(SHAPES):
        q, bank, W = _data(Q, N, P, D, 50 + n)
        s, e = pq.token_scores_pq(q, bank, W), pq.exact_token_scores_pq(q, bank, W)
        err = float(np.abs(s - e).max())
        print((Q, N, P, D), "max |fp32 - fp64| =", err, "bound", pq.score_bound(D))
        assert 0 < err <= pq.score_bound(D)
        for combine in pq.COMBINES:
            want = {"min": e.min(axis=2), "max": e.max(axis=2), "mean": e.mean(axis=2)}[combine]
            assert np.abs(pq.combine(s, combine) - want).max() <= pq.score_bound(D, combine, P)
            if P >= 3:
                d = -np.sort(-e, axis=2)[:, :, :3]
                want = {"min": d[:, :, 2], "max": d[:, :, 0], "mean": d.mean(axis=2)}[combine]
                assert np.abs(pq.combine(s, combine, 3) - want).max() <= pq.score_bound(D, combine, 3)


def test_identical_rows_are_within_the_second_bound_of_the_shared_weights_search():
    differ = 0
    for n, (Q, N, P, D) in enumerate(SHAPES):
        q, bank, W = _data(Q, N, P, D, 60 + n)
        w = W[0]
        s, ref = pq.token_scores_pq(q, bank, np.broadcast_to(w, q.shape)), tsr.token_scores(q, bank, w)
        err = float(np.abs(s - ref).max())
        print((Q, N, P, D), "max |per-query - shared| =", err, "bound", pq.shared_bound(D))
        assert err <= pq.shared_bound(D)
        differ += int((s != ref).sum())
        for combine in pq.COMBINES:
            assert np.abs(pq.combine(s, combine) - tsr.combine_scores(ref, combine)).max() <= pq.shared_bound(D, combine, P)
    assert differ > 0                                             # the two norm chains are not the same bits: the docs say so


GOLDEN_CASES = ((130, 1, 512), (65, 16, 128), (65, 64, 64))


def test_one_target_returns_the_goldens_images():
    """Q = 1 with the target's own weights as the one row: the ten best images of every combined-score array of similarity.npz
    and similarity_topt.npz, in the golden's order (no case is left out: none has a near-tie that flips)."""
    z, zt = np.load(os.path.join(GOLDEN, "similarity.npz")), np.load(os.path.join(GOLDEN, "similarity_topt.npz"))
    n = 0
    for (T, P, N) in GOLDEN_CASES:
        key = f"sim/{T}_{P}_{N}"
        tgt, tst = torch.from_numpy(z[key + "/target"]), z[key + "/test"]
        avg, w = so.determine_target_features(tgt)
        for uw in (1, 0):
            W = w.numpy()[None] if uw else np.ones((1, tst.shape[2]), np.float32)
            s = pq.token_scores_pq(avg[None].numpy(), tst, W)
            for combine in pq.COMBINES:
                for t in (None, 1, 2, 3, 4, 8, 16):
                    name = f"{key}/cosine_{combine}_{uw}" + ("" if t is None else f"_t{t}")
                    if t is not None and name not in zt.files:
                        continue
                    ref = (z if t is None else zt)[name]
                    got = pq.combine(s, combine, t)[0]
                    # the golden is torch's fp32 evaluation in an order of its own: each side is within score_bound of fp64
                    count = P if t is None else t
                    assert np.abs(got - ref).max() <= 2 * pq.score_bound(tst.shape[2], combine, count), name
                    _, idx = tsr.topk_of_scores(got[None], 10)
                    assert np.array_equal(idx[0], np.argsort(-ref, kind="stable")[:10]), name
                    n += 1
    assert n == 18 + 72


def test_pq_predicate_follows_its_stated_limits():
    """skyemb_cosine_token_pq_applicable: skyemb_cosine_token_applicable's limits with 128 D in place of 64 D; a refusal leaves
    the refused shape as the error text."""
    def want(Q, P, D, k):
        return (1 <= Q <= 16 and D >= 64 and D % 64 == 0 and D <= 1024 and 1 <= P <= 4096 and (16 % P == 0 or P % 16 == 0)
                and 1 <= k <= 512 and 128 * D + 32 * Q * k <= 163840)
    L = _lib.lib()
    n = 0
    for Q in (0, 1, 3, 6, 7, 16, 17):
        for P in (0, 1, 3, 4, 16, 24, 32, 4096, 4112):
            for D in (0, 32, 64, 96, 768, 1024, 1088):
                for k in (0, 1, 100, 127, 128, 129, 300, 512, 513):
                    assert bool(L.skyemb_cosine_token_pq_applicable(Q, P, D, k)) == want(Q, P, D, k), (Q, P, D, k)
                    if not want(Q, P, D, k):
                        text = L.skyemb_last_error().decode()
                        assert f"(Q={Q} P={P} D={D} k={k})" in text and "128 D + 32 Q k <= 163840" in text
                    n += 1
    assert n > 3000
    # the issue's examples: D = 768, k = 300 -> six queries per pass; D = 1024 -> three
    assert search._pq_group("t", 16, 768, 300) == 6 and search._pq_group("t", 16, 1024, 300) == 3
    assert search._pq_group("t", 4, 768, 100) == 16
    with pytest.raises(ValueError, match="128 D"):
        search._pq_group("t", 16, 768, 513)
    # the existing predicate and the list count are untouched
    assert ops.cosine_token_applicable(7, 16, 768, 300) and not L.skyemb_cosine_token_pq_applicable(7, 16, 768, 300)
    assert ops.cosine_token_topk_chunks(100000, 16, 16, 768, 100) > 0


def test_python_layer_refuses_wrong_weight_shapes_without_a_device():
    Q, N, P, D = 5, 40, 4, 64
    q, bank = torch.zeros(Q, D), torch.zeros(N, P, D)
    assert search._weights_arg(None, Q, D, "t") is None and search._weights_arg(torch.ones(D), Q, D, "t") is None
    W = torch.ones(Q, D)
    assert search._weights_arg(W, Q, D, "t") is W
    calls = (lambda w: search.cosine_topk_tokens(q, bank, 3, weights=w), lambda w: search.cosine_token_scores(q, bank, weights=w),
             lambda w: search.distance_topk_tokens(q, bank, 3, weights=w), lambda w: search.distance_token_scores(q, bank, weights=w))
    for bad in (torch.ones(Q - 1, D), torch.ones(Q, D // 2), torch.ones(1, Q, D), torch.ones(D + 64), torch.ones(())):
        for call in calls:
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(tuple(bad.shape)) in str(e.value) and f"({Q}, {D})" in str(e.value) and f"({D},)" in str(e.value)
    with pytest.raises(ValueError, match="PreparedBank"):
        search.cosine_topk(q, object(), 3, weights=W)


def test_cli_per_target_needs_bank_and_two_latents_per_target(monkeypatch):
    import similarity_search
    parser = similarity_search.parseArguments()
    assert parser.parse_args(["m"]).per_target is False and parser.parse_args(["m", "--bank", "--per-target"]).per_target is True
    monkeypatch.setattr("sys.argv", ["similarity_search.py", "m", "--per-target"])
    with pytest.raises(SystemExit) as e:
        similarity_search.main()
    assert "--per-target" in str(e.value) and "--bank" in str(e.value)
    # per target: determine_target_features over that target's latents alone; all targets pooled without the flag
    tl = torch.randn(3 * 5, 4, 8)
    q, w = similarity_search.target_queries(tl, 3, True)
    for t in range(3):
        avg_t, w_t = similarity_search.determine_target_features(tl[5 * t:5 * t + 5])
        assert torch.equal(q[t], avg_t) and torch.equal(w[t], w_t)
    q1, w1 = similarity_search.target_queries(tl, 3, False)
    avg, wa = similarity_search.determine_target_features(tl)
    assert q1.shape == (1, 8) and torch.equal(q1[0], avg) and torch.equal(w1, wa)
    with pytest.raises(SystemExit) as e:                              # -aug False with a pooled mode: one vector per target
        similarity_search.target_queries(torch.randn(3, 1, 8), 3, True)
    assert "no variance" in str(e.value) and "\n" not in str(e.value)


def test_pq_bindings_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.skyemb_version() == _lib.ABI_VERSION == 111                      # additive: the version did not move
    names = ("skyemb_cosine_token_pq_applicable", "skyemb_cosine_token_scores_pq", "skyemb_cosine_token_topk_pq",
             "skyemb_distance_token_scores_pq", "skyemb_distance_token_topk_pq")
    for name in names:
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    buf = np.zeros(4096, np.float32)
    b = buf.ctypes.data + (-buf.ctypes.data) % 16
    rc = L.skyemb_cosine_token_scores_pq(None, None, None, 1, None, 1, 10, 4, 64, 0, 0, 1e-6, None, None, None)
    assert rc != 0 and b"bad arguments" in L.skyemb_last_error()
    rc = L.skyemb_cosine_token_scores_pq(b, b, b, 7, b, 1, 10, 4, 64, 0, 0, 1e-6, b, None, None)
    assert rc != 0 and b"bank_dtype" in L.skyemb_last_error()
    rc = L.skyemb_cosine_token_scores_pq(b, b, b, 1, b + 4, 1, 10, 4, 64, 0, 0, 1e-6, b, None, None)
    assert rc != 0 and b"skyemb_cosine_token_scores_pq: w must be 16-byte aligned" in L.skyemb_last_error()
    rc = L.skyemb_cosine_token_topk_pq(b, b, b, 1, b, 16, 1000, 16, 768, 300, 0, 0, 1e-6, 0, 4, None, b, b, None, None)
    assert rc != 0 and b"128 D + 32 Q k <= 163840 bytes of LDS (Q=16 P=16 D=768 k=300)" in L.skyemb_last_error()
    rc = L.skyemb_cosine_token_topk_pq(b, b, b, 1, b, 2, 1000, 16, 64, 5, 0, 17, 1e-6, 0, 4, None, b, b, None, None)
    assert rc != 0 and b"top_t" in L.skyemb_last_error()
    rc = L.skyemb_cosine_token_topk_pq(b, b, b, 1, b, 2, 1000, 16, 64, 5, 0, 0, 1e-6, 0, 3, None, b, b, None, None)
    assert rc != 0 and b"nlists" in L.skyemb_last_error()
    rc = L.skyemb_cosine_token_scores_pq(b, b, b, 1, b, 1, 10, 4, 64, 0, 0, 1e-6, b, b + 2, None)
    assert rc != 0 and b"select must be 4-byte aligned" in L.skyemb_last_error()
    rc = L.skyemb_distance_token_scores_pq(b + 4, b, b, 1, 1, 10, 4, 64, 2, 1, 0, b, None, None)
    assert rc != 0 and b"skyemb_distance_token_scores_pq: bank, c and t must be 16-byte aligned" in L.skyemb_last_error()
    rc = L.skyemb_distance_token_topk_pq(b, b, b, 1, 16, 1000, 16, 1024, 2, 1, 0, 100, 0, 4, None, b, b, None, None)
    assert rc != 0 and b"skyemb_distance_token_topk_pq" in L.skyemb_last_error() and b"128 D" in L.skyemb_last_error()
    rc = L.skyemb_distance_token_topk_pq(b, b, b, 1, 2, 1000, 16, 64, 3, 1, 0, 5, 0, 4, None, b, b, None, None)
    assert rc != 0 and b"metric" in L.skyemb_last_error()
