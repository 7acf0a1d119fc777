#!/usr/bin/env python3
"""Generate tests/golden/token_search_refusals.json: the ValueError (type and full text) that the Python layer of the patch-token
search raises for a fixed list of bad requests, recorded from the commit BEFORE a change to that layer so that
tests/test_token_host_cpu.py can hold the changed layer to the same texts and the same precedence.

Usage (at the commit whose behaviour is the reference; needs the built library, no device):
    python tests/golden/make_token_refusal_golden.py

Everything runs on CPU tensors: every listed request is refused before any device work.  ``cases()`` is the list (the test
imports it): seven functions -- the four public token functions, the two floors, ``cosine_topk`` -- times every single fault
and every pair of simultaneous faults that can be put into one request of that function.  A fault the function has no argument
for, or does not look at (the floors check neither k, the bank's dtype nor its shape; ``token_pruning_floor`` reads ``combine``
only after its size rule: ``EXTRA`` reaches that refusal with a bank large enough), is left out for that function; a pair
stays as soon as one of its two faults is looked at.

File: {"messages": [[type, text], ...], "cases": {case id: index into messages}} -- texts repeat a lot, so they are stored once.
"""
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from sky_embeddings_amd import search  # noqa: E402

OUT = os.environ.get("SKYEMB_GOLDEN_OUT") or HERE
Q, N, P, D, K = 5, 600, 4, 64, 3

# fault -> the fields of the request it sets.  Two faults that set the same field cannot be simultaneous.
FAULTS = {
    "combine": dict(combine="median"),
    "metric": dict(metric="cosine"),
    "top_t0": dict(top_t=0), "top_t17": dict(top_t=17), "top_tTrue": dict(top_t=True), "top_t2.5": dict(top_t=2.5),
    "k0": dict(k=0), "kN": dict(k=N + 1), "k513": dict(k=513),
    "w(Q-1,D)": dict(weights="Q-1,D"), "w(Q,D/2)": dict(weights="Q,D/2"), "w(1,Q,D)": dict(weights="1,Q,D"), "w(D+64)": dict(weights="D+64"),
    "pq": dict(weights="Q,D"),                   # not a fault by itself: with a shape fault it is "a shape no group fits"
    "int8": dict(dtype=torch.int8),
    "P3": dict(P=3),
    "D96": dict(D=96),
    "selectN+1": dict(select="N+1"),
    "prepared": dict(bank="prepared"),           # cosine_topk only: a PreparedBank stand-in (with select / [Q, D] weights)
    "notflat": dict(bank="notflat"),             # cosine_topk only: a bank that is neither flat nor a PreparedBank (the same)
}
NOT_ALONE = {"pq", "prepared", "notflat"}
# the faults each function looks at, and those it can be handed but does not check (kept in pairs, never alone)
TOPK = {"combine", "top_t0", "top_t17", "top_tTrue", "top_t2.5", "k0", "kN", "k513", "w(Q-1,D)", "w(Q,D/2)", "w(1,Q,D)", "w(D+64)", "pq",
        "int8", "P3", "D96", "selectN+1"}
SCORES = TOPK - {"k0", "kN", "k513"}
TOP_T = {"top_t0", "top_t17", "top_tTrue", "top_t2.5"}
W_BAD = {"w(Q-1,D)", "w(Q,D/2)", "w(1,Q,D)", "w(D+64)"}
FUNCTIONS = {
    "cosine_topk_tokens": (TOPK, set()),
    "cosine_token_scores": (SCORES, set()),
    "distance_topk_tokens": (TOPK | {"metric"}, set()),
    "distance_token_scores": (SCORES | {"metric"}, set()),
    "token_pruning_floor": (TOP_T | W_BAD | {"selectN+1"}, {"combine", "int8", "P3", "D96"}),
    "distance_pruning_floor": (TOP_T | W_BAD | {"selectN+1", "metric", "combine"}, {"int8", "P3", "D96"}),
    # cosine_topk hands a request to the token search for [Q, D] weights or a select; every case here takes one of the two
    "cosine_topk": ({"k0", "kN", "k513", "w(Q-1,D)", "w(Q,D/2)", "w(1,Q,D)", "pq", "int8", "D96", "selectN+1", "prepared", "notflat"},
                    set()),
}
# token_pruning_floor reads ``combine`` only once its size rule lets the floor run: a bank of 8 x 256 k images, per-query weights
# (a plain tensor is then sampled without a device), and the refusal comes before the sample is scored
EXTRA = [("token_pruning_floor|combine@N2048", "token_pruning_floor", dict(combine="median", N=2048, k=1, weights="Q,D"))]


def _weights(spec, Qn, Dn):
    if spec is None:
        return None
    shape = {"Q-1,D": (Qn - 1, Dn), "Q,D/2": (Qn, Dn // 2), "1,Q,D": (1, Qn, Dn), "D+64": (Dn + 64,), "Q,D": (Qn, Dn)}[spec]
    return torch.ones(shape)


def cases():
    """-> [(case id, function name, request fields)] in a fixed order."""
    out = []
    for fn, (looked_at, carried) in FUNCTIONS.items():
        names = [f for f in FAULTS if f in looked_at or f in carried]
        combos = [(f,) for f in names if f in looked_at and f not in NOT_ALONE] + list(itertools.combinations(names, 2))
        for combo in combos:
            fields = [set(FAULTS[f]) for f in combo]
            if len(combo) == 2 and (fields[0] & fields[1] or (not (set(combo) & looked_at) - NOT_ALONE
                                                              and set(combo) not in ({"pq", "prepared"}, {"pq", "notflat"}))):
                continue
            # cosine_topk: only requests that it hands to the token search or refuses itself (2-D weights or a select)
            if fn == "cosine_topk" and not set(combo) & {"w(Q-1,D)", "w(Q,D/2)", "pq", "selectN+1"}:
                continue
            req = {}
            for f in combo:
                req.update(FAULTS[f])
            out.append((f"{fn}|{'+'.join(combo)}", fn, req))
    return out + EXTRA


def run(fn, req):
    """Build the request on the CPU and call ``fn``; -> whatever it raises (None if it returns)."""
    Dn, Pn, Nn = req.get("D", D), req.get("P", P), req.get("N", N)
    dtype = req.get("dtype", torch.float32)
    q = torch.zeros(Q, Dn)
    flat = fn == "cosine_topk"
    bank = torch.zeros((Nn, Dn) if flat else (Nn, Pn, Dn), dtype=dtype)
    if req.get("bank") == "prepared":
        bank = search.PreparedBank.__new__(search.PreparedBank)   # a stand-in: refused by its type alone
    elif req.get("bank") == "notflat":
        bank = torch.zeros(Nn, P, Dn)
    w = _weights(req.get("weights"), Q, Dn)
    select = torch.ones(Nn + 1, dtype=torch.bool) if req.get("select") == "N+1" else None
    k, combine, metric, top_t = req.get("k", K), req.get("combine"), req.get("metric"), req.get("top_t")
    kw = {} if combine is None else {"combine": combine}
    if metric is not None:
        kw["metric"] = metric
    try:
        if fn == "cosine_topk":
            search.cosine_topk(q, bank, k, weights=w, select=select)
        elif fn == "cosine_topk_tokens":
            search.cosine_topk_tokens(q, bank, k, weights=w, top_t=top_t, select=select, **kw)
        elif fn == "cosine_token_scores":
            search.cosine_token_scores(q, bank, weights=w, top_t=top_t, select=select, **kw)
        elif fn == "distance_topk_tokens":
            search.distance_topk_tokens(q, bank, k, weights=w, top_t=top_t, select=select, **kw)
        elif fn == "distance_token_scores":
            search.distance_token_scores(q, bank, weights=w, top_t=top_t, select=select, **kw)
        elif fn == "token_pruning_floor":
            search.token_pruning_floor(q, torch.zeros(Q), bank, k, top_t=top_t, select=select, weights=w, **kw)
        elif fn == "distance_pruning_floor":
            c = torch.full((Dn,), 1.0 / Dn) if w is None else w
            search.distance_pruning_floor(c, q, bank, k, top_t=top_t, select=select, **kw)
    except Exception as e:            # noqa: BLE001 -- the type is part of what is recorded
        return e
    return None


def main():
    messages, index, table = [], {}, {}
    for cid, fn, req in cases():
        e = run(fn, req)
        assert isinstance(e, ValueError), (cid, repr(e))     # every listed request is refused by the Python layer, device-free
        key = (type(e).__name__, str(e))
        if key not in index:
            index[key] = len(messages)
            messages.append(list(key))
        table[cid] = index[key]
    path = os.path.join(OUT, "token_search_refusals.json")
    with open(path, "w") as f:
        json.dump({"messages": messages, "cases": table}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(table), "cases,", len(messages), "distinct refusals,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
