"""GPU: the device linear probe (csrc/probe.hip, sky_embeddings_amd/probe.py) -- every kernel element by element against the fp64
statements of tests/probe_reference.py within the bars derived there, bit-identical repeats under another row stride, the two fits
end to end against scikit-learn's recorded results (tests/golden/probe.npz), ``linear_probe(on_device=True)`` against the host
path, and ``pretrain_mim.py`` with ``lp_device = True``."""
import configparser
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import probe_reference as pr
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
CASES = {"a": 3, "b": 5}


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLDEN, "probe.npz")))


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def padded(x, pad):
    """The same rows inside a wider buffer: (view [n, F] with row stride F + pad)."""
    n, F = x.shape
    buf = torch.full((n, F + pad), float("nan"), device="cuda", dtype=x.dtype)
    buf[:, :F] = x
    return buf[:, :F]


@functools.lru_cache(maxsize=None)
def features(m, F, seed=0):
    """Correlated fp32 features with offset columns (never written)."""
    rng = np.random.default_rng(100 * seed + m + F)
    lat = rng.standard_normal((m, 5))
    x = lat @ rng.standard_normal((5, F)) + 0.5 * rng.standard_normal((m, F)) + 2.0 * rng.standard_normal(F)
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- per element
@pytest.mark.parametrize("n,F", [(97, 130), (1001, 70), (33, 300)])
def test_colstats_and_scale_per_element(n, F):
    from sky_embeddings_amd import ops
    x = features(n, F).copy()
    x[:, 3] = np.float32(-0.75)                                  # a constant column: variance exactly 0, scale exactly 1
    mean, var, scale, out = pr.scale_reference(x)
    e_mean, e_var, e_scale, e_out = pr.scale_bars(x)
    xd = dev(x)
    gm, gv, gs = ops.probe_colstats(xd)
    go = ops.probe_scale(xd, gm, gs, torch.empty_like(xd))
    for name, got, want, bar in (("mean", gm, mean, e_mean), ("var", gv, var, e_var), ("scale", gs, scale, e_scale), ("out", go, out, e_out)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print(name, "max err / bar", float((err / np.maximum(bar, 1e-300)).max()))
        assert np.all(err <= bar), name
    assert float(gv[3]) == 0.0 and float(gs[3]) == 1.0 and bool((go[:, 3] == 0).all())
    # applying the fit split's statistics to other rows, and centring only
    other = features(17, F, seed=1)
    got = ops.probe_scale(dev(other), gm, gs, torch.empty(17, F, device="cuda"))
    want = pr.apply_scale_reference(other, gm.cpu().numpy(), gs.cpu().numpy())
    assert np.all(np.abs(got.cpu().numpy() - want) <= pr.U * np.abs(want) * 1.01 + 2.0 ** -149)
    got = ops.probe_scale(dev(other), gm, None, torch.empty(17, F, device="cuda"))
    want = other.astype(np.float64) - gm.cpu().numpy()
    assert np.all(np.abs(got.cpu().numpy() - want) <= pr.U * np.abs(want) * 1.01 + 2.0 ** -149)
    # another row stride: the same bits
    xp = padded(xd, 5)
    pm, pv, ps = ops.probe_colstats(xp)
    po = ops.probe_scale(xp, pm, ps, padded(torch.empty_like(xd), 3))
    assert torch.equal(pm, gm) and torch.equal(pv, gv) and torch.equal(ps, gs) and torch.equal(po, go)


def run_softmax(xd, yd, W, b, l2):
    from sky_embeddings_amd import ops
    m, F = xd.shape
    K = W.shape[0]
    loss = torch.empty(1, device="cuda", dtype=torch.float64)
    gW, gb = torch.empty(K, F, device="cuda"), torch.empty(K, device="cuda")
    ws = torch.empty(ops.probe_softmax_ws_bytes(m, F, K) // 8 + 1, device="cuda", dtype=torch.float64)
    ops.probe_softmax_loss_grad(xd, yd, W, b, l2, loss, gW, gb, ws)
    return loss, gW, gb


# m odd; F = 1030 crosses the 1024-column LDS tile of W; K = 3 / 5 / 16 are the three register paddings (4, 8, 16)
@pytest.mark.parametrize("m,F,K", [(97, 130, 3), (193, 40, 5), (67, 1030, 16), (129, 70, 16), (31, 2051, 5)])
def test_softmax_objective_per_element(m, F, K):
    rng = np.random.default_rng(m + F + K)
    x = features(m, F)
    y = rng.integers(0, K, m).astype(np.int32)
    W = (rng.standard_normal((K, F)) * 0.05).astype(np.float32)
    b = rng.standard_normal(K).astype(np.float32)
    l2 = 1.0 / (0.01 * m)
    loss, gW, gb, _ = pr.softmax_objective(x, W, b, y, l2, np.float64)
    e_loss, e_gW, e_gb = pr.softmax_bars(x, W, b, y, l2)
    xd, yd, Wd, bd = dev(x), dev(y), dev(W), dev(b)
    gl, ggW, ggb = run_softmax(xd, yd, Wd, bd, l2)
    errW = np.abs(ggW.cpu().numpy().astype(np.float64) - gW)
    errb = np.abs(ggb.cpu().numpy().astype(np.float64) - gb)
    print("loss err / bar", abs(float(gl) - loss) / e_loss, "gW", float((errW / e_gW).max()), "gb", float((errb / e_gb).max()))
    assert abs(float(gl) - loss) <= e_loss and np.all(errW <= e_gW) and np.all(errb <= e_gb)
    # fixed reduction order: again, and with another row stride
    for xin in (xd, padded(xd, 7)):
        l2_, gW2, gb2 = run_softmax(xin, yd, Wd, bd, l2)
        assert torch.equal(l2_, gl) and torch.equal(gW2, ggW) and torch.equal(gb2, ggb)


@pytest.mark.parametrize("m,F", [(97, 130), (193, 70), (45, 257)])
def test_gram_per_element(m, F):
    from sky_embeddings_amd import ops
    rng = np.random.default_rng(m * F)
    xc = features(m, F) - features(m, F).mean(axis=0, dtype=np.float64).astype(np.float32)
    yc = rng.standard_normal(m).astype(np.float32)
    G, q, yn = pr.gram_reference(xc, yc)
    eG, eq, eyn = pr.gram_bars(xc, yc)

    def run(xin):
        Gd = torch.full((F, F), float("nan"), device="cuda", dtype=torch.float64)
        qd, ynd = torch.empty(F, device="cuda", dtype=torch.float64), torch.empty(1, device="cuda", dtype=torch.float64)
        ops.probe_gram(xin, dev(yc), Gd, qd, ynd)
        return Gd, qd, ynd
    Gd, qd, ynd = run(dev(xc))
    assert np.all(np.abs(Gd.cpu().numpy() - G) <= eG) and np.all(np.abs(qd.cpu().numpy() - q) <= eq) and abs(float(ynd) - yn) <= eyn
    assert torch.equal(Gd, Gd.T)
    G2, q2, yn2 = run(padded(dev(xc), 9))
    assert torch.equal(G2, Gd) and torch.equal(q2, qd) and torch.equal(yn2, ynd)


def run_cd(G, q, yn, a1, b2, max_iter, tol):
    from sky_embeddings_amd import ops
    F = q.size
    w = torch.empty(F, device="cuda", dtype=torch.float64)
    status, gap = torch.empty(2, device="cuda", dtype=torch.int32), torch.empty(1, device="cuda", dtype=torch.float64)
    ops.probe_enet_cd(dev(G), dev(q), dev(np.array([yn])), a1, b2, max_iter, tol, w, status, gap)
    return w, status.cpu().tolist(), float(gap)


@pytest.mark.parametrize("case,max_iter", [("a", 10000), ("a", 3), ("b", 40)])
def test_coordinate_descent_per_element(case, max_iter):
    """The kernel on the statement's own (G, q): the same sweeps, the same stop, w within the bar, gap within its bar.  Case b has
    F = 130 (three 64-coordinate groups, the last one ragged), a zero diagonal entry (the constant column) and many active rows."""
    g = golden()
    fit = g[f"{case}_fit"]
    X = g[f"{case}_xs"][fit].astype(np.float64)
    xc = (X - X.mean(axis=0)).astype(np.float32)
    yc = (g[f"{case}_reg"][fit].astype(np.float64) - g[f"{case}_reg"][fit].astype(np.float64).mean()).astype(np.float32)
    m = xc.shape[0]
    a1, b2 = 1e-4 * 0.9 * m, 1e-4 * 0.1 * m
    G, q, yn = pr.gram_reference(xc, yc)
    w, sweeps, conv, gap = pr.enet_cd(G, q, yn, a1, b2, max_iter, 1e-4)
    gw, (gs, gc), ggap = run_cd(G, q, yn, a1, b2, max_iter, 1e-4)
    err = np.abs(gw.cpu().numpy() - w)
    print("sweeps", gs, sweeps, "max|dw|", err.max(), "bar", pr.enet_w_bar(w, sweeps), "gap", ggap, gap)
    assert (gs, bool(gc)) == (sweeps, conv)
    assert conv == (max_iter == 10000)                       # a run that ends on its last sweep is not reported as converged
    assert np.all(err <= pr.enet_w_bar(w, sweeps))
    assert abs(ggap - gap) <= pr.enet_gap_bar(G, q, yn, w, G @ w, a1, b2)
    gw2, st2, gap2 = run_cd(G, q, yn, a1, b2, max_iter, 1e-4)
    assert torch.equal(gw2, gw) and st2 == [gs, gc] and gap2 == ggap


def test_refusals_launch_nothing():
    from sky_embeddings_amd import _lib, ops, probe
    x = dev(features(16, 40))
    y = torch.zeros(16, device="cuda", dtype=torch.int32)
    sentinel = lambda *shape: torch.full(shape, 7.0, device="cuda")
    for K in (2, 17):
        W, b, gW, gb = torch.zeros(K, 40, device="cuda"), torch.zeros(K, device="cuda"), sentinel(K, 40), sentinel(K)
        loss = torch.full((1,), 7.0, device="cuda", dtype=torch.float64)
        assert ops.probe_softmax_ws_bytes(16, 40, K) == -1
        with pytest.raises(_lib.SkyembError, match=f"K={K}"):
            ops.probe_softmax_loss_grad(x, y, W, b, 0.1, loss, gW, gb, torch.zeros(1 << 16, device="cuda", dtype=torch.float64))
        torch.cuda.synchronize()
        assert bool((gW == 7).all()) and bool((gb == 7).all()) and float(loss) == 7.0
    wide = torch.zeros(4, 4097, device="cuda")
    with pytest.raises(_lib.SkyembError, match="F=4097"):
        ops.probe_softmax_loss_grad(wide, y, torch.zeros(3, 4097, device="cuda"), torch.zeros(3, device="cuda"), 0.1,
                                    torch.zeros(1, device="cuda", dtype=torch.float64), sentinel(3, 4097), sentinel(3),
                                    torch.zeros(1 << 16, device="cuda", dtype=torch.float64))
    q = torch.full((4097,), 7.0, device="cuda", dtype=torch.float64)
    with pytest.raises(_lib.SkyembError, match="F=4097"):
        ops.probe_gram(wide, torch.zeros(4, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.float64), q,
                       torch.zeros(1, device="cuda", dtype=torch.float64))
    with pytest.raises(_lib.SkyembError, match="F=4097"):
        ops.probe_enet_cd(q, q, q, 1.0, 1.0, 10, 1e-4, q, torch.zeros(2, device="cuda", dtype=torch.int32), q, F=4097)
    torch.cuda.synchronize()
    assert bool((q == 7).all())
    with pytest.raises(_lib.SkyembError):
        probe.fit_softmax(x, np.arange(16) % 2)
    with pytest.raises(_lib.SkyembError):
        probe.fit_elastic_net(wide, np.zeros(4))


# -------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("case", CASES)
def test_fit_softmax_on_the_goldens(case):
    from sky_embeddings_amd import probe
    g = golden()
    xs, fit, held, cls = dev(g[f"{case}_xs"]), g[f"{case}_fit"], g[f"{case}_held"], g[f"{case}_cls"]
    x_fit, x_held = xs[dev(fit)], xs[dev(held)]
    est = probe.fit_softmax(x_fit, cls[fit], C=0.01, max_iter=10000)
    assert list(est.classes) == list(range(CASES[case]))
    pf, ph = est.predict(x_fit).cpu().numpy(), est.predict(x_held).cpu().numpy()
    differ = int((pf != g[f"{case}_lr_pred_fit"]).sum() + (ph != g[f"{case}_lr_pred_held"]).sum())
    print(case, "iterations", est.n_iter, "scikit-learn", int(g[f"{case}_lr_n_iter"]), "evaluations", est.n_eval, "differing predictions", differ,
          "max|dW|", float(np.abs(est.coef.cpu().numpy() - g[f"{case}_lr_coef"]).max()))
    assert differ <= 0.01 * (len(fit) + len(held))
    for pred, rows, k in ((pf, fit, 0), (ph, held, 1)):
        assert abs(float((pred == cls[rows]).mean()) - g[f"{case}_lr_acc"][k]) <= 0.01


@pytest.mark.parametrize("tag", ["enet", "enet3"])
@pytest.mark.parametrize("case", CASES)
def test_fit_elastic_net_on_the_goldens(case, tag):
    from sky_embeddings_amd import probe
    g = golden()
    xs, fit, held, reg = dev(g[f"{case}_xs"]), g[f"{case}_fit"], g[f"{case}_held"], g[f"{case}_reg"]
    x_fit, x_held = xs[dev(fit)], xs[dev(held)]
    est = probe.fit_elastic_net(x_fit, reg[fit], alpha=0.0001, l1_ratio=0.9, max_iter=10000 if tag == "enet" else 3)
    w = est.coef.cpu().numpy()
    want = g[f"{case}_{tag}_coef"]
    print(case, tag, "sweeps", est.n_iter, "scikit-learn", int(g[f"{case}_{tag}_n_iter"]), "max|dw|", float(np.abs(w - want).max()),
          "bar", float(g[f"{case}_{tag}_w_bar"]), "gap", est.gap)
    assert est.converged == bool(g[f"{case}_{tag}_converged"]) == (tag == "enet")
    assert np.array_equal(w != 0, want != 0)
    assert np.all(np.abs(w - want) <= float(g[f"{case}_{tag}_w_bar"]))
    yt = dev(reg, torch.float64)
    for x_rows, rows, k in ((x_fit, fit, 0), (x_held, held, 1)):
        assert abs(probe.r2(yt[dev(rows)], est.predict(x_rows)) - g[f"{case}_{tag}_r2"][k]) <= 1e-4


def _tiny_ini():
    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(ROOT, "configs", "mim_1.ini"))
    cfg["TRAINING"]["total_batch_iters"] = "5"
    cfg["TRAINING"]["batch_size"] = "8"
    return cfg


def test_linear_probe_on_device_matches_the_host_path(tmp_path, capsys):
    """The tiny model and labelled file of test_api_gpu.py::test_linear_probe_hook_on_hip_embeddings."""
    from collections import defaultdict
    from sky_embeddings_amd import hdf5_lite, probe
    from sky_embeddings_amd.utils.dataloaders import build_h5_dataloader
    from sky_embeddings_amd.utils.mim_vit import build_model
    from sky_embeddings_amd.utils.pretrain_fns import get_embeddings, linear_probe
    rng = np.random.default_rng(5)
    n = 240
    level = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    cut = (rng.standard_normal((n, 5, 64, 64), dtype=np.float32) * 0.3 + level[:, None, None, None]).astype(np.float32)
    path = str(tmp_path / "labelled.h5")
    hdf5_lite.write_datasets(path, {"cutouts": cut, "ra": rng.uniform(0, 360, n).astype(np.float32),
                                    "dec": rng.uniform(-90, 90, n).astype(np.float32),
                                    "class": np.digitize(level, [-0.33, 0.33]).astype(np.int64), "zspec": (level + 1.0).astype(np.float32)})
    cfg = _tiny_ini()
    cfg["TRAINING"]["compute_dtype"] = "f32"
    torch.manual_seed(0)
    model, *_ = build_model(cfg, str(tmp_path / "none.pth.tar"), torch.device("cuda"), build_optimizer=True)
    template = build_h5_dataloader(path, batch_size=8, num_workers=0, patch_size=16, num_channels=5, img_size=64, shuffle=False)
    host, device = defaultdict(list), defaultdict(list)
    linear_probe(model, host, "cuda", template, class_data_path=path, regress_data_path=path, combine="pool")
    linear_probe(model, device, "cuda", template, class_data_path=path, regress_data_path=path, combine="pool", on_device=True)
    print({k: (host[k], device[k]) for k in host})
    assert set(device) == {"train_lp_acc", "val_lp_acc", "train_lp_r2", "val_lp_r2"} and all(len(v) == 1 for v in device.values())
    for k in ("train_lp_acc", "val_lp_acc"):
        assert abs(device[k][0] - host[k][0]) <= 0.01
    for k in ("train_lp_r2", "val_lp_r2"):
        assert abs(device[k][0] - host[k][0]) <= 1e-4
    assert "host path" not in capsys.readouterr().out
    # the device features are get_embeddings' features (compared where the reducer does not depend on the token order)
    D = model.module.engine.cfg.embed_dim
    for combine, width in (("token", D), ("flatten", 16 * D), ("pool", D), ("centralpool", D), ("central", 4 * D), ("mean", D)):
        loader = build_h5_dataloader(path, batch_size=64, num_workers=0, patch_size=16, num_channels=5, img_size=64, shuffle=False)
        x = probe.standard_scale(probe.probe_features(model, loader, "cuda", combine, remove_cls=combine != "token"))[0]
        want, _ = get_embeddings(path, model, "cuda", template, y_label="zspec", combine=combine, remove_cls=combine != "token")
        assert x.shape == (n, width) and want.shape == (n, width), combine
        if combine in ("token", "pool", "mean"):       # an MAE encoder returns the patch tokens in a fresh random order per pass
            assert np.allclose(x.cpu().numpy(), want, atol=2e-3), combine
    # parts outside the device path say so in one line and still fill their keys: 2 classes
    two = str(tmp_path / "two.h5")
    hdf5_lite.write_datasets(two, {"cutouts": cut, "ra": np.zeros(n, np.float32), "dec": np.zeros(n, np.float32),
                                   "class": (level > 0).astype(np.int64), "zspec": (level + 1.0).astype(np.float32)})
    part = defaultdict(list)
    linear_probe(model, part, "cuda", template, class_data_path=two, regress_data_path=None, combine="pool", on_device=True)
    out = capsys.readouterr().out
    assert out.count("host path") == 1 and "2 classes" in out and len(part["val_lp_acc"]) == 1 and part["val_lp_acc"][0] > 0.6


def test_pretrain_entry_point_with_lp_device(tmp_path):
    from sky_embeddings_amd import hdf5_lite
    dd = tmp_path / "data"
    dd.mkdir()
    hdf5_lite.make_synthetic_cutouts(str(dd / "synthetic_cutouts_GRIZY_64_train.h5"), n=64, seed=1234)
    hdf5_lite.make_synthetic_cutouts(str(dd / "synthetic_cutouts_GRIZY_64_val.h5"), n=16, seed=4321)
    hdf5_lite.make_synthetic_cutouts(str(dd / "probe.h5"), n=60, seed=99, with_labels=True)
    work = tmp_path / "work"
    (work / "configs").mkdir(parents=True)
    cfg = _tiny_ini()
    cfg["DATA"].update(lp_class_data_file="probe.h5", lp_regress_data_file="probe.h5", lp_combine="pool", lp_device="True")
    with open(work / "configs" / "mim_t.ini", "w") as fh:
        cfg.write(fh)
    for name in ("pretrain_mim.py", "utils", "sky_embeddings_amd"):
        os.symlink(os.path.join(ROOT, name), work / name)
    out = subprocess.run([sys.executable, str(work / "pretrain_mim.py"), "mim_t", "-v", "2", "-ct", "0.001", "-dd", str(dd)],
                         cwd=str(work), env=dict(os.environ, PYTHONPATH=str(work)), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Linear Probing Results:" in out.stdout and "host path" not in out.stdout
    ck = torch.load(str(work / "models" / "mim_t.pth.tar"), map_location="cpu", weights_only=False)
    for k in ("train_lp_acc", "val_lp_acc", "train_lp_r2", "val_lp_r2"):
        assert len(ck["losses"][k]) >= 1 and np.isfinite(ck["losses"][k]).all(), k
