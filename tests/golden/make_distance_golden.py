#!/usr/bin/env python3
"""Generate tests/golden/similarity_distance.npz by RUNNING THE REFERENCE's compute_similarity(metric='MSE' | 'MAE') on the CPU,
on inputs of feature width D = 64 (a width the patch-token kernels accept; similarity.npz holds D = 96).

Usage (where the reference checkout exists; it is imported the way make_golden.py imports it):
    python tests/golden/make_distance_golden.py
    SKYEMB_GOLDEN_OUT=<scratch dir> python tests/golden/make_distance_golden.py     # regenerate elsewhere and compare

Cases (T targets, P patches, N test images): (40, 1, 200), (33, 4, 64), (33, 16, 48), generated as make_golden.similarity_cases
generates its inputs, from seed 64.  Keys per case ``dist/<T>_<P>_<N>``: ``/test`` [N, P, D], ``/avg`` [D] and ``/w`` [D]
(determine_target_features of the targets: what the search takes as query and weights), and
``/<metric>_<combine>_<use_weights>_t<t>`` -> [N] fp32 for metric in {MSE, MAE}, combine in {min, mean, max}, use_weights in
{1, 0}, t in {all, 1, 3, min(P, 16)} where t <= P: 120 result arrays.  Only data is written: no reference source or bytecode is
copied.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("SKYEMB_GOLDEN_OUT") or HERE      # a scratch directory: regenerate there and compare with the committed fixture
CASES = ((40, 1, 200), (33, 4, 64), (33, 16, 48))
D = 64
SEED = 64


def top_ts(P):
    return [None] + sorted({t for t in (1, 3, min(P, 16)) if t <= P})


def main():
    sys.path.insert(0, HERE)
    REF = importlib.import_module("make_golden").REF
    # this repo ships a drop-in ``utils`` package of the same name: keep it off the path so that the REFERENCE is imported
    repo = os.path.dirname(os.path.dirname(HERE))
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or os.getcwd()) != repo]
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "utils"))
    sim = importlib.import_module("utils.similarity")
    assert sim.__file__.startswith(REF), sim.__file__
    torch.set_num_threads(4)
    g = torch.Generator().manual_seed(SEED)
    out, n = {}, 0
    for (T, P, N) in CASES:
        tgt = torch.randn(T, P, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + torch.randn(D, generator=g)
        tst = torch.randn(N, P, D, generator=g) * 1.1 + 0.2
        key = f"dist/{T}_{P}_{N}"
        avg, w = sim.determine_target_features(tgt)
        out[key + "/test"], out[key + "/avg"], out[key + "/w"] = tst.numpy(), avg.numpy(), w.numpy()
        for metric in ("MSE", "MAE"):
            for combine in ("min", "mean", "max"):
                for uw in (True, False):
                    for t in top_ts(P):
                        s = sim.compute_similarity(tgt, tst, metric=metric, combine=combine, use_weights=uw, n_top_sims=t)
                        out[f"{key}/{metric}_{combine}_{int(uw)}_t{'all' if t is None else t}"] = s.numpy().astype(np.float32)
                        n += 1
    assert n == 120, n
    np.savez_compressed(os.path.join(OUT, "similarity_distance.npz"), **out)
    print("wrote similarity_distance:", n, "result arrays")


if __name__ == "__main__":
    main()
