"""Writes tests/golden/probe.npz: small inputs of the device linear probe with scikit-learn's own results on them (coefficients,
intercepts, iteration counts, predictions, scores), so that the tests need no scikit-learn.  Needs scikit-learn 1.7 and scipy;
run from the repository root:  python tests/golden/make_probe_golden.py

Cases (features are standard-scaled over ALL rows first, as utils/pretrain_fns.get_embeddings does, then split):
  a   192 fit + 48 held rows, F = 40, K = 3
  b   97 fit + 25 held rows, F = 130, K = 5; column 7 is constant; class 0 has no member in the held split
  every case: LogisticRegression(lbfgs, C = 0.01, max_iter = 10000) on `cls`, ElasticNet(1e-4, 0.9, max_iter = 10000) on `reg`, and
  the same ElasticNet with max_iter = 3 (`reg3`: stops on the last sweep without converging).
The estimators are given the fp32 scaled features widened to fp64: scikit-learn then iterates in fp64, which is what the device path
restates (its fp32 solvers differ from its fp64 ones by more than the device path does)."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make_case(seed, n_fit, n_held, F, K, constant_col=None, absent_class=None):
    rng = np.random.default_rng(seed)
    n = n_fit + n_held
    latent = rng.standard_normal((n, 6))
    mix = rng.standard_normal((6, F)) * (rng.random((6, F)) < 0.5)
    x = (latent @ mix + 0.5 * rng.standard_normal((n, F)) + rng.standard_normal(F) * 3.0).astype(np.float32)
    if constant_col is not None:
        x[:, constant_col] = np.float32(1.25)
    score = latent[:, :K] + 0.5 * rng.standard_normal((n, K))
    cls = score.argmax(axis=1).astype(np.int32)
    reg = (0.6 * latent[:, 0] - 0.3 * latent[:, 1] + 0.1 * rng.standard_normal(n) + 1.0).astype(np.float32)
    perm = rng.permutation(n)
    if absent_class is not None:        # every member of that class goes to the fit split
        members = np.flatnonzero(cls == absent_class)
        others = np.setdiff1d(perm, members, assume_unique=False)
        others = perm[np.isin(perm, others)]
        perm = np.concatenate([members, others])
        assert members.size < n_fit
    return x, cls, reg, np.sort(perm[:n_fit]).astype(np.int64), np.sort(perm[n_fit:]).astype(np.int64)


def main():
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.linear_model import ElasticNet, LogisticRegression
    from sklearn.metrics import accuracy_score, r2_score
    from sklearn.preprocessing import StandardScaler
    from tests import probe_reference as pr
    out = {}
    for name, kw in (("a", dict(seed=11, n_fit=192, n_held=48, F=40, K=3)),
                     ("b", dict(seed=23, n_fit=97, n_held=25, F=130, K=5, constant_col=7, absent_class=0))):
        x, cls, reg, fit, held = make_case(**kw)
        K = kw["K"]
        assert set(np.unique(cls[fit])) == set(range(K))
        sc = StandardScaler().fit(x.astype(np.float64))
        xs = ((x.astype(np.float64) - sc.mean_) / sc.scale_).astype(np.float32)
        out.update({f"{name}_x": x, f"{name}_cls": cls, f"{name}_reg": reg, f"{name}_fit": fit, f"{name}_held": held,
                    f"{name}_mean": sc.mean_, f"{name}_var": sc.var_, f"{name}_scale": sc.scale_, f"{name}_xs": xs})
        xf, xh = xs[fit].astype(np.float64), xs[held].astype(np.float64)
        lr = LogisticRegression(solver="lbfgs", max_iter=10000, C=0.01, random_state=42).fit(xf, cls[fit])
        out.update({f"{name}_lr_coef": lr.coef_, f"{name}_lr_intercept": lr.intercept_, f"{name}_lr_n_iter": np.int64(lr.n_iter_[0]),
                    f"{name}_lr_pred_fit": lr.predict(xf).astype(np.int32), f"{name}_lr_pred_held": lr.predict(xh).astype(np.int32),
                    f"{name}_lr_acc": np.array([accuracy_score(cls[fit], lr.predict(xf)), accuracy_score(cls[held], lr.predict(xh))])})
        for tag, iters in (("enet", 10000), ("enet3", 3)):
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                en = ElasticNet(alpha=0.0001, l1_ratio=0.9, max_iter=iters, random_state=42).fit(xf, reg[fit].astype(np.float64))
            warned = any(issubclass(c.category, ConvergenceWarning) for c in caught)
            w, b0, sweeps, conv, gap = pr.enet_fit_reference(xs[fit], reg[fit], 0.0001, 0.9, iters, 1e-4)
            diff = float(np.abs(w - en.coef_).max())
            print(f"{name} {tag}: sklearn n_iter {en.n_iter_} warned {warned} gap {en.dual_gap_:.3e}; statement sweeps {sweeps} converged {conv}; "
                  f"max|dw| {diff:.3e}; non-zero sets equal {np.array_equal(w != 0, en.coef_ != 0)}")
            out.update({f"{name}_{tag}_coef": en.coef_, f"{name}_{tag}_intercept": np.float64(en.intercept_),
                        f"{name}_{tag}_n_iter": np.int64(en.n_iter_), f"{name}_{tag}_converged": np.bool_(not warned),
                        f"{name}_{tag}_pred_fit": en.predict(xf), f"{name}_{tag}_pred_held": en.predict(xh),
                        f"{name}_{tag}_r2": np.array([r2_score(reg[fit], en.predict(xf)), r2_score(reg[held], en.predict(xh))]),
                        f"{name}_{tag}_w_bar": np.float64(max(4 * diff, 1e-7))})
        W, b, nit = pr.fit_softmax_reference(xs[fit], cls[fit], K)
        pred = lambda rows: (rows.astype(np.float64) @ W.T + b).argmax(axis=1)
        print(f"{name} softmax: sklearn n_iter {lr.n_iter_[0]}, statement {nit}; differing predictions "
              f"{int((pred(xs[fit]) != lr.predict(xf)).sum() + (pred(xs[held]) != lr.predict(xh)).sum())}; max|dW| {np.abs(W - lr.coef_).max():.3e}")
    path = os.path.join(ROOT, "tests", "golden", "probe.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
