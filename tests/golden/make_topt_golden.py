#!/usr/bin/env python3
"""Generate tests/golden/similarity_topt.npz by RUNNING THE REFERENCE's compute_similarity(metric='cosine', n_top_sims=t) on the
CPU, on the inputs similarity.npz already holds (sim/65_16_128, sim/65_64_64).

Usage (where the reference checkout exists; it imports the way make_golden.py does):
    python tests/golden/make_topt_golden.py

Keys: ``<sim key>/cosine_<combine>_<use_weights>_t<t>`` -> [N] fp32, for t in {1, 2, 3, 4, 8, 16}, combine in {min, mean, max},
use_weights in {1, 0}: 72 arrays.  Only data is written: no reference source or bytecode is copied.
"""
import importlib
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("SKYEMB_GOLDEN_OUT") or HERE      # a scratch directory: regenerate there and compare with the committed fixture
KEYS = ("sim/65_16_128", "sim/65_64_64")
TS = (1, 2, 3, 4, 8, 16)


def main():
    # this repo ships a drop-in ``utils`` package of the same name: keep it off the path so that the REFERENCE is imported
    repo = os.path.dirname(os.path.dirname(HERE))
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or os.getcwd()) != repo]
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "utils"))
    sim = importlib.import_module("utils.similarity")
    assert sim.__file__.startswith(REF), sim.__file__
    torch.set_num_threads(4)
    z = np.load(os.path.join(HERE, "similarity.npz"))
    out = {}
    for key in KEYS:
        tgt, tst = torch.from_numpy(z[key + "/target"]), torch.from_numpy(z[key + "/test"])
        for t in TS:
            for combine in ("min", "mean", "max"):
                for uw in (True, False):
                    s = sim.compute_similarity(tgt, tst, metric="cosine", combine=combine, use_weights=uw, n_top_sims=t)
                    out[f"{key}/cosine_{combine}_{int(uw)}_t{t}"] = s.numpy().astype(np.float32)
    assert len(out) == 72
    np.savez_compressed(os.path.join(OUT, "similarity_topt.npz"), **out)
    print("wrote similarity_topt:", len(out), "arrays")


if __name__ == "__main__":
    main()
