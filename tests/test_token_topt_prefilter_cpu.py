"""CPU: the candidate rule of the two-stage token search under ``top_t`` (tests/token_topt_prefilter_reference.py) -- the count of
passing rows against a brute-force count, the kernel's bit-sliced fold restated lane by lane, the count rule as a necessary
condition of the contract's top-t score --, the route decision, the mapping of t = 1, t = P and 'max' onto the plain folds, and the
new C entries."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from sky_embeddings_amd import _lib, ops, search
from tests import token_topt_prefilter_reference as pr
from tests import token_topt_reference as ttr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN, MAX, MEAN = (ops.COMBINE_CODES[c] for c in ("min", "max", "mean"))
NEW = ("skyemb_token_topt_prefilter_applicable", "skyemb_cosine_topk_tokens_prefiltered_top", "skyemb_cosine_topk_tokens_prefiltered_top_sel")


def _patterns(P, t, rng):
    """Pass bits boolean [8 blocks, 64 rows] of one strip: per image random, all, none and exactly t - 1, t, t + 1 rows."""
    out = []
    n_img = 64 // P
    for kind in ("random", "sparse", "dense", "all", "none", t - 1, t, t + 1):
        b = np.zeros((8, n_img, P), dtype=bool)
        if kind == "random":
            b = rng.random((8, n_img, P)) < 0.5
        elif kind == "sparse":
            b = rng.random((8, n_img, P)) < (t - 0.5) / P
        elif kind == "dense":
            b = rng.random((8, n_img, P)) < min(1.0, (t + 0.5) / P)
        elif kind == "all":
            b[:] = True
        elif kind != "none":
            if not 0 <= kind <= P:
                continue
            for i in range(8):
                for g in range(n_img):
                    b[i, g, rng.permutation(P)[:kind]] = True
        out.append((kind, b.reshape(8, 64)))
    return out


@pytest.mark.parametrize("P", pr.PS)
def test_count_fold_equals_the_brute_force_count(P):
    """Every P and every t in 1 .. min(P, 16): the fold as the kernel writes it (bit planes, row shifts, nibble steps, the plane-wise
    comparison) leaves exactly the images with at least t passing rows, at the bit and lane of their first row, and nothing else."""
    rng = np.random.default_rng(P)
    lgp = P.bit_length() - 1
    for t in range(1, min(P, pr.MAX_TOP_T) + 1):
        for kind, bits in _patterns(P, t, rng):
            words = pr.strip_words(bits)
            got = pr.count_fold_lanes(words, lgp, t)
            want = pr.count_candidates(bits, P, t)                        # [8, 64 / P]
            assert np.array_equal(pr.strip_images(got, lgp), want), (P, t, kind)
            # nothing but the images' first rows is set: the append walk below the fold reads every bit
            back = np.zeros((8, 64), dtype=bool)
            back[:, ::P] = want
            assert np.array_equal(got, pr.strip_words(back)), (P, t, kind)
        # t = P is the AND fold, t = 1 the OR fold: the plain folds the library keeps for them
        bits = rng.random((8, 64)) < 0.7
        r = bits.reshape(8, -1, P)
        assert np.array_equal(pr.count_candidates(bits, P, P if P <= 16 else 16), r.sum(axis=2) >= min(P, 16))
        assert np.array_equal(pr.count_candidates(bits, P, 1), r.any(axis=2))
        if P <= 16:
            assert np.array_equal(pr.count_candidates(bits, P, P), r.all(axis=2))


def test_the_count_is_a_necessary_condition_of_the_top_t_score():
    """d[t-1] >= tau implies at least t token scores >= tau, for every (P, t): the exact-score side of the argument (a NaN score is
    -inf and never counts).  With U_i >= e_i row by row the count of passing rows can only be larger."""
    rng = np.random.default_rng(3)
    for P, t in pr.all_pairs():
        s = rng.standard_normal((3, 40, P)).astype(np.float32)
        s[0, :5, 0] = -np.inf
        s[1, 7] = -np.inf
        d = ttr.combine_top(s, "min", t)
        for tau in (-0.5, 0.0, 0.7):
            reach = d >= np.float32(tau)
            count = (s >= np.float32(tau)).sum(axis=2)
            assert np.array_equal(reach, count >= t), (P, t, tau)


def test_image_sandwich_counts_rows():
    mi = np.array([[1, 1, 0, 0, 1, 0, 0, 0]], dtype=bool)                  # two images of P = 4
    mo = np.array([[0, 0, 1, 0, 0, 1, 1, 1]], dtype=bool)
    for t, (want_in, want_out) in {1: ([1, 1], [0, 0]), 2: ([1, 0], [0, 1]), 3: ([0, 0], [0, 1]), 4: ([0, 0], [1, 1])}.items():
        a, b = pr.image_sandwich_top(mi, mo, 4, t)
        assert a[0].tolist() == [bool(v) for v in want_in] and b[0].tolist() == [bool(v) for v in want_out], t


@pytest.mark.parametrize("P,t", pr.PAIRS)
def test_planted_cases_are_in_their_classes(P, t):
    """The inputs of the GPU file's stage-1 test: one slice, a tail tile with padding rows, and for q* every planted image decided
    by its count of high tokens (asserted inside planted_case)."""
    c = pr.planted_case(P, t, "fp16" if (P + t) % 2 else "bf16", bool(t % 2))
    assert (c["N"] * P) % 256 != 0 and 2048 < c["N"] * P < 2048 + 256 and c["k"] in (1, 100, 256) and c["k"] <= c["N"]
    mi, mo = pr.image_classes(c, c["thr0"])
    planted = c["highs"] >= 0
    assert (mi[pr.QSTAR] | mo[pr.QSTAR])[planted].all()                     # no planted image is a don't-care
    # the defect the sandwich must catch: a fold that ANDs or ORs where it should count
    if 1 < t < P:
        rows_in, _ = pr.sr.sandwich(c["thr0"], c["score"], c["hw"], c["rows"])
        r = rows_in.reshape(c["Q"], c["N"], P)
        assert (r.all(axis=2) != (r.sum(axis=2) >= t))[pr.QSTAR].any() and (r.any(axis=2) != (r.sum(axis=2) >= t))[pr.QSTAR].any()


def _request(**kw):
    tb = search.TokenBank.__new__(search.TokenBank)               # no device: the decision reads the flags only
    tb._resident, tb.dtype = True, torch.float16
    base = dict(who="cosine_topk_tokens", Q=300, N=4096, P=16, D=128, k=10, combine=MIN, metric=None, metric_name=None, top_t=4,
                per_query=False, step=16, idx_offset=0, tokens=None, bank=tb, weights=None, select=None)
    base.update(kw)
    return search.TokenRequest(**base)


def _selection(count):
    sel = search.Selection.__new__(search.Selection)
    sel.count = count
    return sel


def test_route_decision_under_top_t(monkeypatch):
    """'min' and 'max' with top_t take the two-stage route, alone and under a Selection; 'mean' with top_t keeps the grouped route
    with a reason that names it.  (On the commit before this route every request with top_t was refused.)"""
    monkeypatch.setattr(search, "TOKEN_TOPT_PREFILTER_MIN_Q_SMALL", 17)
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 17)
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    refusal = search._token_prefilter_refusal
    for P, t in pr.all_pairs():
        for combine in (MIN, MAX):
            assert refusal(_request(P=P, N=4096 * 16 // P, top_t=t, combine=combine)) is None, (P, t, combine)
    assert refusal(_request(select=_selection(4096))) is None
    assert refusal(_request(select=_selection(4096), combine=MAX)) is None
    assert refusal(_request(select=_selection(128))) is None            # 128 x 16 = 2048 rows
    why = refusal(_request(select=_selection(127)))
    assert isinstance(why, str) and "selected images" in why
    assert refusal(_request(combine=MEAN)) == "top_t under combine 'mean'"
    assert refusal(_request(combine=MEAN, select=_selection(4096))) == "top_t under combine 'mean'"
    for field, (v, word) in dict(per_query=(True, "per-query weights"), P=(48, "divide 64"), D=(144, "D % 32"), k=(257, "k <= 256"),
                                 N=(2 ** 27, "2^31"), metric=(ops.METRIC_CODES["MSE"], "distance metric")).items():
        why = refusal(_request(**{field: v}))
        assert isinstance(why, str) and word in why, (field, why)
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    assert "SKYEMB_TOPK_PREFILTER" in refusal(_request())


def test_each_fold_has_its_own_smallest_q(monkeypatch):
    """The top-t folds ('min' with 1 <= top_t < P) answer to TOKEN_TOPT_PREFILTER_MIN_Q on a bank of at least
    TOKEN_TOPT_PREFILTER_MIN_ELEMENTS elements and to TOKEN_TOPT_PREFILTER_MIN_Q_SMALL below; 'max' with any top_t and 'min' with
    top_t == P are the plain search and answer to TOKEN_PREFILTER_MIN_Q."""
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    refusal = search._token_prefilter_refusal
    monkeypatch.setattr(search, "TOKEN_TOPT_PREFILTER_MIN_Q_SMALL", 301)
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 17)
    assert "TOKEN_TOPT_PREFILTER_MIN_Q_SMALL" in refusal(_request(top_t=4)) and "TOKEN_TOPT_PREFILTER_MIN_Q_SMALL" in refusal(_request(top_t=1))
    assert refusal(_request(top_t=16)) is None and refusal(_request(top_t=4, combine=MAX)) is None and refusal(_request(top_t=0)) is None
    monkeypatch.setattr(search, "TOKEN_TOPT_PREFILTER_MIN_Q_SMALL", 17)
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 301)
    assert refusal(_request(top_t=4)) is None and refusal(_request(top_t=1)) is None
    assert "TOKEN_PREFILTER_MIN_Q" in refusal(_request(top_t=16)) and "TOKEN_PREFILTER_MIN_Q" in refusal(_request(top_t=4, combine=MAX))
    # the measured banks and anything larger: from TOKEN_TOPT_PREFILTER_MIN_Q on, as shipped
    monkeypatch.undo()
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    assert (search.TOKEN_TOPT_PREFILTER_MIN_Q, search.TOKEN_TOPT_PREFILTER_MIN_Q_SMALL) == (64, 256)
    assert search.TOKEN_TOPT_PREFILTER_MIN_ELEMENTS == 62500 * 64 * 768 == 250000 * 16 * 768
    big = dict(N=250000, P=16, D=768, k=100)
    assert refusal(_request(Q=64, **big)) is None and refusal(_request(Q=64, N=62500, P=64, D=768, k=100, top_t=9)) is None
    assert "TOKEN_TOPT_PREFILTER_MIN_Q = 64" in refusal(_request(Q=63, **big))
    assert "TOKEN_TOPT_PREFILTER_MIN_Q_SMALL" in refusal(_request(Q=255, N=249999, P=16, D=768, k=100))
    assert refusal(_request(Q=256, N=249999, P=16, D=768, k=100)) is None
    assert "TOKEN_PREFILTER_MIN_Q" in refusal(_request(Q=64, top_t=16, **big))          # the plain search keeps its own 256


def test_mapping_onto_the_plain_folds():
    """t = P is the AND fold and the plain min, 'max' the OR fold and the plain max whatever t is, t = 1 the OR fold with the top-t
    re-score, everything between counts: the library's rule (ops.token_topt_folds) equals the reference's."""
    for P, t in pr.all_pairs() + [(P, 0) for P in pr.PS]:
        assert ops.token_topt_folds(P, MAX, t) == pr.folds(P, "max", t) == ("or", "max")
        got = ops.token_topt_folds(P, MIN, t)
        assert got == pr.folds(P, "min", t)
        if t in (0, P):
            assert got == ("and", "min")
        elif t == 1:
            assert got == ("or", "top")
        else:
            assert got == ("count", "top")
    assert dataclasses.replace(_request(top_t=7, select=_selection(9)), Q=3).top_t == 7      # the re-run keeps top_t (and the selection)


def test_new_symbols_are_exported_with_the_declared_signatures():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skyemb.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.build())
    for name in NEW:
        m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/skyemb.h"
        assert hasattr(L, name), f"{name} is not exported"
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int32
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args), (name, len(params), len(args))
        for p, a in zip(params, args):
            want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float") else
                    ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int32)
            assert a is want, (name, p, a)
    # top_t sits right after combine in both calls
    for name in NEW[1:]:
        params = [p.strip() for p in re.search(name + r"\s*\(([^)]*)\)\s*;", text).group(1).split(",")]
        assert params[params.index("int combine") + 1] == "int top_t", name
    assert callable(ops.cosine_topk_tokens_prefiltered_top) and callable(ops.cosine_topk_tokens_prefiltered_top_sel)


def test_the_predicate_states_its_limits():
    lib = _lib.lib()
    ok = lib.skyemb_token_topt_prefilter_applicable
    for P, t in pr.all_pairs():
        assert ok(300, 4096 * 16 // P, P, 128, 10, MIN, t) == 1 and ok(300, 4096 * 16 // P, P, 128, 10, MAX, t) == 1, (P, t)
    for P, t in ((16, 0), (16, 17), (8, 9), (64, 17), (1, 2), (16, -1)):
        assert ok(300, 65536 // P, P, 128, 10, MIN, t) == 0
        assert b"top_t must be 1 .. min(P, 16)" in lib.skyemb_last_error(), (P, t)
    assert ok(300, 4096, 16, 128, 10, MEAN, 4) == 0 and b"top_t under combine mean" in lib.skyemb_last_error()
    assert ok(300, 4096, 16, 128, 10, 7, 4) == 0 and b"combine code 7" in lib.skyemb_last_error()
    assert ok(300, 127, 16, 128, 10, MIN, 4) == 0 and b"N * P" in lib.skyemb_last_error()          # the plain search's own text
    assert ops.token_topt_prefilter_refusal(300, 4096, 16, 128, 10, MIN, 4) is None
    assert "top_t must be" in ops.token_topt_prefilter_refusal(300, 4096, 16, 128, 10, MIN, 17)


def test_bad_arguments_are_refused_before_any_device_work():
    """Every refusal returns before the first launch: the pointers are never dereferenced (no GPU is needed to run this)."""
    lib = _lib.lib()
    one = ctypes.c_void_p(256)                                             # non-null, 16-byte aligned, never read

    def top(combine=MIN, top_t=4, P=16, tw=one):
        return lib.skyemb_cosine_topk_tokens_prefiltered_top(tw, one, 300, one, _lib.F16, one, one, one, 4096, P, 128, 10, combine, top_t, 1e-6, 0,
                                                             None, one, 0, one, one, one, None)

    def top_sel(combine=MIN, top_t=4, tiles=one):
        return lib.skyemb_cosine_topk_tokens_prefiltered_top_sel(one, one, 300, one, _lib.F16, one, one, one, tiles, 16, 1, 1, 4096, 16, 128, 10,
                                                                 combine, top_t, 1e-6, 0, None, one, 0, one, one, one, None)

    assert top(combine=MEAN) != 0 and b"top_t under combine mean" in lib.skyemb_last_error()
    assert top_sel(combine=MEAN) != 0 and b"top_t under combine mean" in lib.skyemb_last_error()
    assert top(top_t=17) != 0 and b"top_t must be 0 (all tokens) or 1 .. min(P, 16)" in lib.skyemb_last_error()
    assert top(top_t=-1) != 0 and top(top_t=9, P=8) != 0
    assert top(tw=None) != 0 and b"null argument" in lib.skyemb_last_error()
    assert top_sel(tiles=None) != 0 and b"null argument" in lib.skyemb_last_error()
    # past the argument checks every variant stops at the workspace size (0 bytes were offered): top_t = 0, 1, between, P; max
    for kw in (dict(top_t=0), dict(top_t=1), dict(top_t=4), dict(top_t=16), dict(combine=MAX, top_t=3)):
        assert top(**kw) != 0 and b"workspace too small" in lib.skyemb_last_error(), kw
        assert top_sel(**kw) != 0 and b"workspace too small" in lib.skyemb_last_error(), kw
    # top_t = 0 IS the plain call: it reports under the plain call's name
    assert top(top_t=0) != 0 and lib.skyemb_last_error().startswith(b"skyemb_cosine_topk_tokens_prefiltered:")
    assert top(top_t=4) != 0 and lib.skyemb_last_error().startswith(b"skyemb_cosine_topk_tokens_prefiltered_top:")
