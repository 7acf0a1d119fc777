"""CPU: the restatement of the patch-token search (tests/token_search_reference.py) against the goldens captured from the
reference's compute_similarity, its tie / NaN / zero-token rules, and the library's host-side predicate and bindings."""
import os

import numpy as np
import torch

from oracle import similarity_oracle as so
from tests import token_search_reference as tsr
from sky_embeddings_amd import _lib, ops
from sky_embeddings_amd.ops import COMBINE_CODES          # the token search bindings: this module needs them

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ((130, 1, 512), (65, 16, 128), (65, 64, 64))


def test_restatement_matches_the_reference_goldens():
    """max |delta| < 5e-7 (the bound test_c_topk_oracle_against_reference_formula uses for P = 1) on all 18 combined-score arrays,
    and the same ten best images in the same order."""
    z = np.load(os.path.join(GOLDEN, "similarity.npz"))
    for (T, P, N) in CASES:
        key = f"sim/{T}_{P}_{N}"
        tgt, tst = torch.from_numpy(z[key + "/target"]), z[key + "/test"]
        avg, w = so.determine_target_features(tgt)
        for uw in (1, 0):
            weights = w.numpy() if uw else None
            s = tsr.token_scores(avg[None].numpy(), tst, weights)
            assert s.shape == (1, N, P)
            for combine in tsr.COMBINES:
                ref = z[f"{key}/cosine_{combine}_{uw}"]
                got = tsr.combine_scores(s, combine)[0]
                err = np.abs(got - ref).max()
                print(key, combine, uw, "max |delta| =", err)
                assert err < 5e-7, (key, combine, uw, err)
                _, idx = tsr.topk_of_scores(got[None], 10)
                assert np.array_equal(idx[0], np.argsort(-ref, kind="stable")[:10]), (key, combine, uw)


def test_ties_resolve_to_the_lower_image_index():
    rng = np.random.default_rng(5)
    bank = rng.standard_normal((12, 4, 64), dtype=np.float32)
    bank[9] = bank[2]
    bank[5] = bank[2]
    q = bank[2].mean(axis=0, keepdims=True)
    for combine in tsr.COMBINES:
        s, i = tsr.topk_tokens(q, bank, 12, combine)
        pos = [int(np.where(i[0] == j)[0][0]) for j in (2, 5, 9)]
        assert pos[1] == pos[0] + 1 and pos[2] == pos[0] + 2, (combine, i[0])
        assert s[0][pos[0]] == s[0][pos[1]] == s[0][pos[2]]


def test_nan_and_zero_tokens():
    """A NaN token scores -inf: min and mean of its image are -inf (the image is never returned), max ignores it.  An all-zero
    token scores 0 / eps = 0 exactly and takes part like any other score."""
    rng = np.random.default_rng(6)
    bank = rng.standard_normal((6, 4, 64), dtype=np.float32)
    bank[1, 2, 7] = np.nan
    bank[3, 0] = 0.0
    q = rng.standard_normal((2, 64), dtype=np.float32)
    s = tsr.token_scores(q, bank)
    assert np.isneginf(s[:, 1, 2]).all() and (s[:, 3, 0] == 0).all()
    for combine in ("min", "mean"):
        c = tsr.combine_scores(s, combine)
        assert np.isneginf(c[:, 1]).all() and np.isfinite(np.delete(c, 1, axis=1)).all()
        ts, ti = tsr.topk_of_scores(c, 6)
        assert (ti[:, 5] == -1).all() and np.isneginf(ts[:, 5]).all() and not (ti == 1).any()
    c = tsr.combine_scores(s, "max")
    assert np.array_equal(c[:, 1], np.delete(s[:, 1], 2, axis=1).max(axis=1))
    assert np.array_equal(tsr.combine_scores(s, "min")[:, 3], np.minimum(s[:, 3, 1:].min(axis=1), np.float32(0)))
    # mean: sequential fp32 sum in token order, then one division
    want = ((((np.float32(0) + s[:, 0, 0]) + s[:, 0, 1]) + s[:, 0, 2]) + s[:, 0, 3]) / np.float32(4)
    assert np.array_equal(tsr.combine_scores(s, "mean")[:, 0], want)


def test_applicable_predicate_follows_its_stated_limits():
    """skyemb_cosine_token_applicable(Q, P, D, k): Q <= 16; D % 64 == 0, D <= 1024; 1 <= P <= 4096 with 16 % P == 0 or
    P % 16 == 0; 1 <= k <= 512; 64 D + 32 Q k <= 163840.  Pure host code: no GPU needed."""
    def want(Q, P, D, k):
        return (1 <= Q <= 16 and D >= 64 and D % 64 == 0 and D <= 1024 and 1 <= P <= 4096 and (16 % P == 0 or P % 16 == 0)
                and 1 <= k <= 512 and 64 * D + 32 * Q * k <= 163840)
    n = 0
    for Q in (0, 1, 3, 16, 17):
        for P in (0, 1, 2, 3, 4, 8, 9, 16, 24, 32, 48, 64, 256, 4096, 4112, 8192):
            for D in (0, 32, 64, 96, 128, 768, 1024, 1088):
                for k in (0, 1, 10, 100, 192, 193, 224, 225, 300, 512, 513):
                    assert ops.cosine_token_applicable(Q, P, D, k) == want(Q, P, D, k), (Q, P, D, k)
                    n += 1
    assert n > 5000
    # the default n_save of similarity_search.py with one target vector, ViT-B and ViT-L widths
    assert ops.cosine_token_applicable(1, 16, 768, 300) and ops.cosine_token_applicable(1, 16, 1024, 300)
    assert ops.cosine_token_applicable(1, 256, 1024, 300)
    # list counts exist exactly where the predicate holds
    assert ops.cosine_token_topk_chunks(100000, 16, 1, 768, 300) > 0
    assert ops.cosine_token_topk_chunks(100000, 9, 1, 768, 300) == 0


def test_new_bindings_load_and_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.skyemb_version() == _lib.ABI_VERSION == 111
    assert (_lib.COMBINE_MIN, _lib.COMBINE_MEAN, _lib.COMBINE_MAX) == (0, 1, 2)
    assert COMBINE_CODES == {"min": 0, "mean": 1, "max": 2} and tuple(COMBINE_CODES) == tsr.COMBINES
    for name in ("skyemb_cosine_token_applicable", "skyemb_cosine_token_topk_chunks", "skyemb_cosine_token_scores",
                 "skyemb_cosine_token_topk"):
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    # argument validation happens before any device work, so it is safe without a GPU
    rc = L.skyemb_cosine_token_topk(None, None, None, None, 1, 10, 16, 64, 5, 0, 1e-6, 0, 1, None, None, None, None)
    assert rc != 0 and b"bad arguments" in L.skyemb_last_error()
    buf = (np.zeros(64, np.float32)).ctypes.data
    rc = L.skyemb_cosine_token_topk(buf, buf, buf, buf, 1, 10, 9, 64, 5, 0, 1e-6, 0, 1, None, buf, buf, None)
    assert rc != 0 and b"16 % P == 0" in L.skyemb_last_error()
    rc = L.skyemb_cosine_token_scores(buf, buf, buf, buf, 1, 10, 16, 96, 0, 1e-6, buf, None)
    assert rc != 0 and b"D % 64 == 0" in L.skyemb_last_error()
    rc = L.skyemb_cosine_token_scores(buf, buf, buf, buf, 1, 10, 16, 64, 7, 1e-6, buf, None)
    assert rc != 0 and b"unknown combine" in L.skyemb_last_error()
