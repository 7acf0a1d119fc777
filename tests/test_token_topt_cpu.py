"""CPU: the restatement of the top-t patch combine (tests/token_topt_reference.py) against the goldens captured from the
reference's compute_similarity(n_top_sims=t), its identities, NaN / -inf and tie rules, and the refusals of the two `_top` entry
points before any device work."""
import itertools
import os

import numpy as np
import torch

from oracle import similarity_oracle as so
from tests import token_search_reference as tsr
from tests import token_topt_reference as ttr
from sky_embeddings_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ((65, 16, 128), (65, 64, 64))
TS = (1, 2, 3, 4, 8, 16)
NINF = np.float32(-np.inf)


def test_restatement_matches_the_reference_goldens():
    """max |delta| < 5e-7 (the bound tests/test_token_search_cpu.py uses) on all 72 arrays of similarity_topt.npz, and the same ten
    best images in the same order."""
    z = np.load(os.path.join(GOLDEN, "similarity.npz"))
    zt = np.load(os.path.join(GOLDEN, "similarity_topt.npz"))
    n, worst = 0, 0.0
    for (T, P, N) in CASES:
        key = f"sim/{T}_{P}_{N}"
        tgt, tst = torch.from_numpy(z[key + "/target"]), z[key + "/test"]
        avg, w = so.determine_target_features(tgt)
        for uw in (1, 0):
            s = tsr.token_scores(avg[None].numpy(), tst, w.numpy() if uw else None)
            for t in TS:
                for combine in ttr.COMBINES:
                    ref = zt[f"{key}/cosine_{combine}_{uw}_t{t}"]
                    got = ttr.combine_top(s, combine, t)[0]
                    err = float(np.abs(got - ref).max())
                    print(key, combine, uw, t, "max |delta| =", err)
                    assert err < 5e-7, (key, combine, uw, t, err)
                    _, idx = tsr.topk_of_scores(got[None], 10)
                    assert np.array_equal(idx[0], np.argsort(-ref, kind="stable")[:10]), (key, combine, uw, t)
                    n, worst = n + 1, max(worst, err)
    print("largest |delta| over", n, "arrays =", worst)
    assert n == 72 == len(zt.files)


def test_identities_with_the_plain_combines():
    rng = np.random.default_rng(11)
    for P in (2, 4, 16, 48):
        bank = rng.standard_normal((9, P, 64), dtype=np.float32)
        bank[3, P // 2, 1] = np.nan
        s = tsr.token_scores(rng.standard_normal((3, 64), dtype=np.float32), bank)
        if P <= 16:
            assert np.array_equal(ttr.combine_top(s, "min", P), tsr.combine_scores(s, "min"))       # t == P: the plain min
        for t in range(1, min(P, 16) + 1):
            assert np.array_equal(ttr.combine_top(s, "max", t), tsr.combine_scores(s, "max"))       # any t: the plain max
        assert np.array_equal(ttr.combine_top(s, "mean", 1), tsr.combine_scores(s, "max"))          # (0 + d[0]) / 1
        assert np.array_equal(ttr.combine_top(s, "min", 1), tsr.combine_scores(s, "max"))


def test_mean_at_t_equal_p_sums_in_descending_order():
    """mean with top_t == P is not the plain mean.  Token scores 0.1, 0.7, 0.2, 0.4 (as fp32): the plain mean sums them in token
    order, the top-t mean as 0.7, 0.4, 0.2, 0.1; the two fp32 sums differ in the last bit."""
    f = np.float32
    s = np.array([[[f(0.1), f(0.7), f(0.2), f(0.4)]]], np.float32)
    want_plain = ((((f(0) + f(0.1)) + f(0.7)) + f(0.2)) + f(0.4)) / f(4)
    want_top = ((((f(0) + f(0.7)) + f(0.4)) + f(0.2)) + f(0.1)) / f(4)
    plain, top = tsr.combine_scores(s, "mean")[0, 0], ttr.combine_top(s, "mean", 4)[0, 0]
    assert plain == want_plain and top == want_top
    assert plain != top and np.nextafter(min(plain, top), f(1)) == max(plain, top)           # neighbours: one ulp apart
    # the top-t mean does not depend on the token order
    for perm in itertools.permutations(range(4)):
        assert ttr.combine_top(s[:, :, list(perm)], "mean", 4)[0, 0] == want_top


def test_images_short_of_finite_tokens_score_minus_inf():
    """Exactly t - 1 finite tokens: -inf under min and mean, absent from the top-k; exactly t finite tokens: finite.  max ignores
    the -inf tokens."""
    rng = np.random.default_rng(12)
    P, t = 8, 3
    bank = rng.standard_normal((6, P, 64), dtype=np.float32)
    bank[1, t - 1:, 0] = np.nan                                  # image 1: t - 1 = 2 finite tokens
    bank[4, t:, 0] = np.nan                                      # image 4: t = 3 finite tokens
    q = rng.standard_normal((2, 64), dtype=np.float32)
    s = tsr.token_scores(q, bank)
    assert np.isfinite(s[:, 1]).sum(axis=1).tolist() == [t - 1] * 2 and np.isfinite(s[:, 4]).sum(axis=1).tolist() == [t] * 2
    for combine in ("min", "mean"):
        c = ttr.combine_top(s, combine, t)
        assert np.isneginf(c[:, 1]).all() and np.isfinite(np.delete(c, 1, axis=1)).all()
        ts, ti = ttr.topk_tokens_top(q, bank, 6, combine, t)
        assert not (ti == 1).any() and (ti[:, 5] == -1).all() and np.isneginf(ts[:, 5]).all() and (ti[:, :5] >= 0).all()
        assert (np.sort(ti[:, :5], axis=1) == [0, 2, 3, 4, 5]).all()
    assert np.array_equal(ttr.combine_top(s, "min", t)[:, 4], s[:, 4, :t].min(axis=1))
    c = ttr.combine_top(s, "max", t)
    assert np.isfinite(c).all() and np.array_equal(c[:, 1], s[:, 1, :t - 1].max(axis=1))
    # +inf and -inf tokens in one sum: NaN, which ranks as -inf
    s2 = np.array([[[np.inf, NINF, 1.0, 2.0]]], np.float32)
    assert np.isneginf(ttr.combine_top(s2, "mean", 4)[0, 0]) and ttr.combine_top(s2, "mean", 3)[0, 0] == np.inf


def test_ties():
    """Duplicated token rows inside one image: the score is that of any ordering of them.  Duplicate images resolve to the
    lower index."""
    rng = np.random.default_rng(13)
    bank = rng.standard_normal((12, 4, 64), dtype=np.float32)
    bank[2, 3] = bank[2, 0]                                      # two equal tokens in image 2
    bank[9] = bank[2]
    bank[5] = bank[2][[3, 1, 0, 2]]                              # the same tokens in another order
    q = bank[2].mean(axis=0, keepdims=True)
    for combine in ttr.COMBINES:
        for t in (1, 2, 3, 4):
            c = ttr.combined_scores_top(q, bank, combine, t)
            for perm in itertools.permutations(range(4)):
                b2 = bank.copy()
                b2[2] = bank[2][list(perm)]
                assert ttr.combined_scores_top(q, b2, combine, t)[0, 2] == c[0, 2], (combine, t, perm)
            s, i = ttr.topk_tokens_top(q, bank, 12, combine, t)
            pos = [int(np.where(i[0] == j)[0][0]) for j in (2, 5, 9)]
            assert pos[1] == pos[0] + 1 and pos[2] == pos[0] + 2, (combine, t, i[0])
            assert s[0][pos[0]] == s[0][pos[1]] == s[0][pos[2]]


def test_top_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument validation happens before any device work, so this is safe without a GPU.  bank_dtype takes the three bank types
    (SKYEMB_BF16 = 0, SKYEMB_F32 = 1, SKYEMB_F16 = 2); every other code is refused."""
    L = _lib.lib()
    assert L.skyemb_version() == _lib.ABI_VERSION == 111
    for name in ("skyemb_cosine_token_scores_top", "skyemb_cosine_token_topk_top"):
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    buf = np.zeros(256, np.float32).ctypes.data           # a host address: no call below may get as far as reading it

    def err(rc):
        assert rc != 0
        return L.skyemb_last_error()

    def topk(dt=_lib.F32, P=4, D=64, combine=0, top_t=2, bank=buf):
        return L.skyemb_cosine_token_topk_top(buf, buf, bank, dt, buf, 1, 10, P, D, 5, combine, top_t, 1e-6, 0, 1, None, buf, buf, None)

    def scores(dt=_lib.F32, P=4, D=64, combine=0, top_t=2, bank=buf):
        return L.skyemb_cosine_token_scores_top(buf, buf, bank, dt, buf, 1, 10, P, D, combine, top_t, 1e-6, buf, None)

    for dt in (_lib.F32, _lib.F16, _lib.BF16):
        for call in (topk, scores):
            for top_t, P in ((-1, 4), (17, 4), (5, 4), (17, 16), (17, 64), (3, 2)):
                msg = err(call(dt=dt, P=P, top_t=top_t))
                assert b"top_t" in msg and f"top_t={top_t} P={P}".encode() in msg, msg
            assert b"unknown combine" in err(call(dt=dt, combine=7))
            assert b"unknown combine" in err(call(dt=dt, combine=-1, top_t=0))
            assert b"16 % P == 0" in err(call(dt=dt, P=9)) and b"D % 64 == 0" in err(call(dt=dt, D=96))
            assert b"bad arguments" in err(call(dt=dt, bank=None))
    for dt in (3, 7, -1):                                  # no bank element type
        for call in (topk, scores):
            for rc in (call(dt=dt), call(dt=dt, bank=None), call(dt=dt, top_t=0)):
                msg = err(rc)
                assert b"bank_dtype must be" in msg and str(dt).encode() in msg, msg
    # top_t = 0 is the plain call: NULL pointers reach the plain call's text
    plain = err(L.skyemb_cosine_token_topk(None, None, None, None, 1, 10, 16, 64, 5, 0, 1e-6, 0, 1, None, None, None, None))
    assert b"bad arguments" in plain
    for dt in (_lib.F32, _lib.F16, _lib.BF16):
        top = err(L.skyemb_cosine_token_topk_top(None, None, None, dt, None, 1, 10, 16, 64, 5, 0, 0, 1e-6, 0, 1, None, None, None, None))
        assert top.replace(b"skyemb_cosine_token_topk_top", b"skyemb_cosine_token_topk") == plain
        msg = err(L.skyemb_cosine_token_scores_top(None, None, None, dt, None, 1, 10, 16, 64, 0, 0, 1e-6, None, None))
        assert b"bad arguments" in msg


def test_python_layer_refuses_top_t_out_of_range_and_the_cli_takes_the_flag():
    import pytest
    import similarity_search
    from sky_embeddings_amd import search
    bank = torch.zeros(8, 4, 64)
    for call in (lambda t: search.cosine_topk_tokens(torch.zeros(1, 64), bank, 2, top_t=t),
                 lambda t: search.cosine_token_scores(torch.zeros(1, 64), bank, top_t=t)):
        for t in (0, -1, 5, 17, 2.5, True):
            with pytest.raises(ValueError, match="top_t"):
                call(t)
    with pytest.raises(ValueError, match="top_t"):
        search.cosine_topk_tokens(torch.zeros(1, 64), torch.zeros(8, 64, 64), 2, top_t=17)
    parser = similarity_search.parseArguments()
    assert parser.parse_args(["m"]).n_top_sims is None
    assert parser.parse_args(["m", "-nts", "3"]).n_top_sims == 3 and parser.parse_args(["m", "--n_top_sims", "4"]).n_top_sims == 4
