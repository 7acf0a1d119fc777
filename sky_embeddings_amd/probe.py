"""The linear-probe validation fits on the device (include/skyemb.h "linear-probe fits", csrc/probe.hip).

The reference's probe (utils/pretrain_fns.py:52-159) copies every token to the host, scales them in NumPy and fits scikit-learn's
LogisticRegression and ElasticNet there while the GPU idles.  Here the features never leave HBM:

  probe_features    mae_latent's loop with the ``combine`` reduction done per batch on the device -> [n, F] fp32
  standard_scale    StandardScaler: fp64 column statistics, scale exactly 1 where the variance is 0
  fit_softmax       scikit-learn's own optimiser call (scipy L-BFGS-B) with the loss and gradient evaluated by one kernel sequence;
                    only the K F + K parameters and gradients cross the bus per evaluation
  fit_elastic_net   fp64 Gram of the centred features + cyclic coordinate descent by one persistent workgroup

Limits (refused with SkyembError, no fallback here; utils.pretrain_fns.linear_probe routes uncovered parts to the host path):
3 <= K <= 16 classes, F <= 4096 features.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ops

MAX_F, MIN_K, MAX_K = _lib.PROBE_MAX_F, _lib.PROBE_MIN_K, _lib.PROBE_MAX_K
REDUCERS = ('token', 'flatten', 'pool', 'centralpool', 'central', 'mean')


def _centre_index(n_tokens, n_patches, device):
    from .utils.misc import central_indices
    side = int(n_tokens ** 0.5)
    ij = central_indices(np.empty((side, side)), n_patches)
    return torch.as_tensor(ij[:, 0] * side + ij[:, 1], device=device, dtype=torch.long)


def reduce_tokens(tokens, combine):
    """[b, tokens, D] -> [b, F]: utils/pretrain_fns.get_embeddings' reducers on device tensors."""
    b = tokens.shape[0]
    if combine == 'token':
        return tokens[:, :1].reshape(b, -1)
    if combine == 'flatten':
        return tokens.reshape(b, -1)
    if combine == 'pool':
        return tokens.amax(dim=1)
    if combine == 'centralpool':
        return tokens.index_select(1, _centre_index(tokens.shape[1], 16, tokens.device)).amax(dim=1)
    if combine == 'central':
        return tokens.index_select(1, _centre_index(tokens.shape[1], 4, tokens.device)).reshape(b, -1)
    if combine == 'mean':
        return tokens.mean(dim=1)
    raise ValueError(f"probe_features: combine must be one of {REDUCERS}, got {combine!r}")


def probe_features(model, loader, device, combine='central', remove_cls=True):
    """Encode every batch of ``loader`` and reduce its tokens on the device -> [n, F] fp32, nothing copied to the host
    (utils.eval_fns.mae_latent + the reducers of utils.pretrain_fns.get_embeddings)."""
    if combine not in REDUCERS:
        raise ValueError(f"probe_features: combine must be one of {REDUCERS}, got {combine!r}")
    net = getattr(model, 'module', model)
    model.eval()
    if net.attn_pool:
        combine = 'flatten'          # an attention-pooled encoder returns a single feature row
    if combine == 'token':
        remove_cls = False
    keep_from = 0 if (not remove_cls or net.attn_pool) else net.num_extra_tokens
    rows = []
    with torch.no_grad():
        for samples, _masks, ra_decs in loader:
            latent = net.forward_features(samples.to(device, non_blocking=True), ra_dec=ra_decs, mask=None, reshape_out=False)[0]
            rows.append(reduce_tokens(latent[:, keep_from:].detach().float(), combine))
    return torch.cat(rows).contiguous()


def standard_scale(x, stats=None):
    """StandardScaler on the device: x [n, F] fp32 -> (scaled fp32 [n, F], mean fp64 [F], scale fp64 [F]).  ``stats`` =
    (mean, scale) of another split applies those instead of fitting."""
    x = x.contiguous()
    if stats is None:
        mean, _var, scale = ops.probe_colstats(x)
    else:
        mean, scale = stats
    return ops.probe_scale(x, mean, scale, torch.empty_like(x)), mean, scale


@dataclass
class SoftmaxFit:
    coef: torch.Tensor          # [K, F] fp32, device
    intercept: torch.Tensor     # [K] fp32, device
    classes: np.ndarray         # label of every row of coef
    n_iter: int
    n_eval: int
    loss: float

    def predict(self, x):
        """Row labels as a device tensor of indices into ``classes``."""
        return (x @ self.coef.T + self.intercept).argmax(dim=1)


def fit_softmax(X, y, C=0.01, max_iter=10000, tol=1e-4):
    """LogisticRegression(solver='lbfgs', C=C, max_iter=max_iter, tol=tol) on device features X [m, F] fp32: scikit-learn's optimiser
    call from zeros, l2 = 1 / (C m), with skyemb_probe_softmax_loss_grad as the objective."""
    from scipy.optimize import minimize
    X = X.contiguous()
    m, F = X.shape
    classes, idx = np.unique(np.asarray(y.cpu() if torch.is_tensor(y) else y), return_inverse=True)
    K = len(classes)
    if not (MIN_K <= K <= MAX_K) or F > MAX_F:
        raise _lib.SkyembError(f"fit_softmax: {K} classes, {F} features outside the device path ({MIN_K}..{MAX_K} classes, <= {MAX_F} features)")
    dev = X.device
    labels = torch.as_tensor(idx.astype(np.int32), device=dev)
    params = torch.zeros(K * F + K, device=dev, dtype=torch.float32)
    grad = torch.empty_like(params)
    loss = torch.empty(1, device=dev, dtype=torch.float64)
    ws = torch.empty(ops.probe_softmax_ws_bytes(m, F, K) // 8 + 1, device=dev, dtype=torch.float64)
    W, b, gW, gb = params[:K * F], params[K * F:], grad[:K * F], grad[K * F:]
    l2 = 1.0 / (C * m)
    evals = [0]

    def objective(p):
        params.copy_(torch.from_numpy(p.astype(np.float32)))
        ops.probe_softmax_loss_grad(X, labels, W, b, l2, loss, gW, gb, ws, m=m, F=F, K=K)
        evals[0] += 1
        return float(loss.item()), grad.cpu().numpy().astype(np.float64)

    res = minimize(objective, np.zeros(K * F + K), method='L-BFGS-B', jac=True,
                   options=dict(maxiter=max_iter, maxls=50, gtol=tol, ftol=64 * np.finfo(float).eps))
    final = torch.from_numpy(res.x.astype(np.float32)).to(dev)
    return SoftmaxFit(final[:K * F].reshape(K, F).contiguous(), final[K * F:].contiguous(), classes, int(res.nit), evals[0], float(res.fun))


@dataclass
class ElasticNetFit:
    coef: torch.Tensor          # [F] fp64, device
    intercept: float
    n_iter: int                 # sweeps run
    converged: bool             # the duality-gap test passed (False: max_iter sweeps ran out)
    gap: float

    def predict(self, x):
        return x.double() @ self.coef + self.intercept


def fit_elastic_net(X, y, alpha=1e-4, l1_ratio=0.9, max_iter=10000, tol=1e-4):
    """ElasticNet(alpha, l1_ratio, max_iter=max_iter, tol=tol, selection='cyclic') with an intercept on device features X [m, F]
    fp32: centre, fp64 Gram, coordinate descent on the Gram, intercept = mean(y) - mean(X) . w."""
    X = X.contiguous()
    m, F = X.shape
    if F > MAX_F:
        raise _lib.SkyembError(f"fit_elastic_net: {F} features outside the device path (<= {MAX_F})")
    dev = X.device
    y64 = torch.as_tensor(np.asarray(y, dtype=np.float64) if not torch.is_tensor(y) else y, device=dev).double()
    y_mean = y64.mean()
    yc = (y64 - y_mean).float().contiguous()
    x_mean, _var, _scale = ops.probe_colstats(X)
    Xc = ops.probe_scale(X, x_mean, None, torch.empty_like(X))
    G = torch.empty(F, F, device=dev, dtype=torch.float64)
    q = torch.empty(F, device=dev, dtype=torch.float64)
    ynorm2 = torch.empty(1, device=dev, dtype=torch.float64)
    ops.probe_gram(Xc, yc, G, q, ynorm2)
    w = torch.empty(F, device=dev, dtype=torch.float64)
    status = torch.empty(2, device=dev, dtype=torch.int32)
    gap = torch.empty(1, device=dev, dtype=torch.float64)
    ops.probe_enet_cd(G, q, ynorm2, alpha * l1_ratio * m, alpha * (1.0 - l1_ratio) * m, max_iter, tol, w, status, gap)
    sweeps, converged = (int(v) for v in status.cpu())
    return ElasticNetFit(w, float(y_mean - x_mean @ w), sweeps, bool(converged), float(gap.item()))


def accuracy(y_true, y_pred):
    return float((y_true == y_pred).double().mean())


def r2(y_true, y_pred):
    y_true, y_pred = y_true.double(), y_pred.double()
    return float(1.0 - ((y_true - y_pred) ** 2).sum() / ((y_true - y_true.mean()) ** 2).sum())
