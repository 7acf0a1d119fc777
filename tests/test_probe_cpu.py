"""CPU: the NumPy statements of the device linear probe (tests/probe_reference.py) against scikit-learn's recorded results
(tests/golden/probe.npz, written by tests/golden/make_probe_golden.py), and the argument refusals of the ABI, which happen before any
device work.  Measured when the golden was written (statement against scikit-learn 1.7.2):
    softmax   a: 11 / 11 L-BFGS iterations, no differing prediction, max|dW| 1.7e-8;   b: 18 / 18, none, 2.8e-8
    elastic   a: 245 / 245 sweeps, max|dw| 1.2e-8;   b: 8638 / 8638 sweeps, max|dw| 1.5e-7;   max_iter = 3: 3 / 3, not converged"""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import probe_reference as pr
from tests.conftest import GOLDEN

CASES = {"a": 3, "b": 5}


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLDEN, "probe.npz")))


@pytest.mark.parametrize("case", CASES)
def test_scaling_statement_is_standard_scaler(case):
    g = golden()
    mean, var, scale, out = pr.scale_reference(g[f"{case}_x"])
    e_mean, e_var, e_scale, e_out = pr.scale_bars(g[f"{case}_x"])
    assert np.all(np.abs(mean - g[f"{case}_mean"]) <= 2 * e_mean) and np.all(np.abs(var - g[f"{case}_var"]) <= 2 * e_var + 1e-300)
    assert np.all(np.abs(scale - g[f"{case}_scale"]) <= 2 * e_scale)
    assert np.all(np.abs(out - g[f"{case}_xs"]) <= 2 * e_out)
    if case == "b":
        assert var[7] == 0.0 and scale[7] == 1.0 and np.all(out[:, 7] == 0.0)      # the constant column


@pytest.mark.parametrize("case", CASES)
def test_softmax_statement_fp32_within_its_bar_of_fp64(case):
    g = golden()
    X, y, K = g[f"{case}_xs"][g[f"{case}_fit"]], g[f"{case}_cls"][g[f"{case}_fit"]], CASES[case]
    W, b = g[f"{case}_lr_coef"].astype(np.float32), g[f"{case}_lr_intercept"].astype(np.float32)
    l2 = 1.0 / (0.01 * X.shape[0])
    l64, gW64, gb64, _ = pr.softmax_objective(X, W, b, y, l2, np.float64)
    l32, gW32, gb32, _ = pr.softmax_objective(X, W, b, y, l2, np.float32)
    e_loss, e_gW, e_gb = pr.softmax_bars(X, W, b, y, l2)
    assert abs(l32 - l64) <= e_loss and np.all(np.abs(gW32 - gW64) <= e_gW) and np.all(np.abs(gb32 - gb64) <= e_gb)
    # at scikit-learn's optimum the gradient is small against its terms
    assert np.abs(gW64).max() < 1e-3 and np.abs(gb64).max() < 1e-3


@pytest.mark.parametrize("case", CASES)
def test_softmax_statement_under_lbfgs_predicts_like_scikit_learn(case):
    g = golden()
    xs, fit, held = g[f"{case}_xs"], g[f"{case}_fit"], g[f"{case}_held"]
    W, b, nit = pr.fit_softmax_reference(xs[fit], g[f"{case}_cls"][fit], CASES[case])
    assert nit == int(g[f"{case}_lr_n_iter"])
    pred = lambda rows: (rows.astype(np.float64) @ W.T + b).argmax(axis=1)
    assert np.array_equal(pred(xs[fit]), g[f"{case}_lr_pred_fit"]) and np.array_equal(pred(xs[held]), g[f"{case}_lr_pred_held"])
    assert np.abs(W - g[f"{case}_lr_coef"]).max() < 1e-6
    if case == "b":
        assert 0 not in g["b_cls"][held] and 0 in g["b_cls"][fit]


@pytest.mark.parametrize("tag", ["enet", "enet3"])
@pytest.mark.parametrize("case", CASES)
def test_coordinate_descent_on_the_fp64_gram_is_scikit_learns(case, tag):
    g = golden()
    xs, fit, held, reg = g[f"{case}_xs"], g[f"{case}_fit"], g[f"{case}_held"], g[f"{case}_reg"]
    iters = 10000 if tag == "enet" else 3
    w, b0, sweeps, conv, gap = pr.enet_fit_reference(xs[fit], reg[fit], 0.0001, 0.9, iters, 1e-4)
    assert sweeps == int(g[f"{case}_{tag}_n_iter"]) and conv == bool(g[f"{case}_{tag}_converged"])
    assert conv == (tag == "enet")                              # max_iter = 3 ends on its last sweep and is NOT converged
    assert np.array_equal(w != 0, g[f"{case}_{tag}_coef"] != 0)
    assert np.abs(w - g[f"{case}_{tag}_coef"]).max() <= float(g[f"{case}_{tag}_w_bar"]) / 4 * 1.0000001
    assert abs(b0 - float(g[f"{case}_{tag}_intercept"])) < 1e-6
    for rows, k in ((fit, 0), (held, 1)):
        assert abs(pr.r2_score(reg[rows], xs[rows].astype(np.float64) @ w + b0) - g[f"{case}_{tag}_r2"][k]) < 1e-6


def test_gram_in_fp32_is_not_good_enough():
    """Why the Gram is fp64: with an fp32 Gram the same descent stops after another number of sweeps."""
    g = golden()
    xs, fit, reg = g["a_xs"], g["a_fit"], g["a_reg"]
    _, _, sweeps32, _, _ = pr.enet_fit_reference(xs[fit], reg[fit], 0.0001, 0.9, 10000, 1e-4, gram_dtype=np.float32)
    _, _, sweeps64, _, _ = pr.enet_fit_reference(xs[fit], reg[fit], 0.0001, 0.9, 10000, 1e-4)
    assert sweeps64 == int(g["a_enet_n_iter"])
    G32, q32, _ = pr.gram_reference(xs[fit] - xs[fit].mean(axis=0), reg[fit], np.float32)
    G64, q64, _ = pr.gram_reference(xs[fit] - xs[fit].mean(axis=0), reg[fit], np.float64)
    eG, _, _ = pr.gram_bars(xs[fit] - xs[fit].mean(axis=0), reg[fit])
    assert np.any(np.abs(G32 - G64) > 1e3 * eG)                # far outside the fp64 bar
    print("sweeps with an fp32 Gram:", sweeps32, "fp64:", sweeps64)


def test_gap_statement_matches_the_definition():
    """primal - dual of the elastic net at the scaled residual, computed from X and y directly."""
    g = golden()
    X = (g["a_xs"][g["a_fit"]] - g["a_xs"][g["a_fit"]].mean(axis=0)).astype(np.float32).astype(np.float64)
    y = (g["a_reg"][g["a_fit"]] - g["a_reg"][g["a_fit"]].mean()).astype(np.float32).astype(np.float64)
    m = X.shape[0]
    a1, b2 = 1e-4 * 0.9 * m, 1e-4 * 0.1 * m
    G, q, yn = pr.gram_reference(X, y)
    w, sweeps, conv, gap = pr.enet_cd(G, q, yn, a1, b2, 5, 1e-4)
    r = y - X @ w
    dn = np.abs(X.T @ r - b2 * w).max()
    c = min(1.0, a1 / dn)
    primal = 0.5 * r @ r + a1 * np.abs(w).sum() + 0.5 * b2 * w @ w
    dual = c * (r @ y) - 0.5 * c * c * (r @ r + b2 * w @ w)
    assert abs(gap - (primal - dual)) <= 1e-9 * (abs(primal) + abs(dual))
    assert abs(pr.enet_gap(G, q, yn, w, G @ w, a1, b2) - gap) <= pr.enet_gap_bar(G, q, yn, w, G @ w, a1, b2)


def test_abi_refuses_bad_shapes_without_a_device():
    from sky_embeddings_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(64)        # never dereferenced: every call below is refused before any launch

    def softmax(m, F, K):
        return L.skyemb_probe_softmax_loss_grad(one, F, one, m, F, K, one, one, 0.1, one, one, one, one, 1 << 40, None)
    for m, F, K, word in ((8, 40, 2, b"K=2"), (8, 40, 17, b"K=17"), (8, 4097, 3, b"F=4097"), (0, 40, 3, b"m=0")):
        assert softmax(m, F, K) == 1 and word in L.skyemb_last_error()
        assert L.skyemb_probe_softmax_ws_bytes(m, F, K) == -1
    assert L.skyemb_probe_softmax_ws_bytes(192, 40, 3) == 16 + 4 * (192 + 192 * 3 + 32 * 3 * 40)
    assert L.skyemb_probe_softmax_loss_grad(one, 40, one, 8, 40, 3, one, one, 0.1, one, one, one, one, 8, None) == 1
    assert b"workspace" in L.skyemb_last_error()
    assert L.skyemb_probe_gram(one, 4097, one, 8, 4097, one, one, one, None) == 1 and b"F=4097" in L.skyemb_last_error()
    assert L.skyemb_probe_gram(one, 39, one, 8, 40, one, one, one, None) == 1                      # row stride below F
    assert L.skyemb_probe_gram(None, 40, one, 8, 40, one, one, one, None) == 1 and b"null" in L.skyemb_last_error()
    assert L.skyemb_probe_enet_cd(one, one, one, 4097, 1.0, 1.0, 10, 1e-4, one, one, one, None) == 1 and b"F=4097" in L.skyemb_last_error()
    assert L.skyemb_probe_enet_cd(one, one, one, 40, 1.0, 1.0, 0, 1e-4, one, one, one, None) == 1
    assert L.skyemb_probe_colstats(one, 40, 0, 40, one, one, one, one, None) == 1
    assert L.skyemb_probe_scale(one, 40, 8, 40, one, one, one, 39, None) == 1
    assert (_lib.PROBE_CHUNKS, _lib.PROBE_MAX_F, _lib.PROBE_MIN_K, _lib.PROBE_MAX_K) == (32, 4096, 3, 16)
