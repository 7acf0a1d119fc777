#!/usr/bin/env python3
"""Generate tests/golden/row_search_trace.json: what make_token_trace_golden.py records for the grouped token route, for the row-bank
search (``cosine_topk`` / ``cosine_scores`` over tensors and PreparedBanks) and for the two-stage routes of ``cosine_topk_tokens``:
per case the sequence of ``ops`` calls, the ``stats`` dict and a SHA-256 digest of the returned tensors -- for a refused call the
exception's type and full text in the digest's place.  Recorded on a GPU from the commit BEFORE a change to that layer, so that
tests/test_row_host_gpu.py can hold the changed layer to the same launches, the same bits and the same refusals.

Usage (on a machine with a GPU, at the commit whose behaviour is the reference):
    python tests/golden/make_row_trace_golden.py

Section 'rows' (N = 4608 rows = 18 tiles of 256, D = 128): ``cosine_topk`` over bank (fp32 tensor, fp16 tensor, PreparedBank(fp32),
PreparedBank(fp16), PreparedBank.resident(bf16), PreparedBank.resident(fp16); the PreparedBanks with weights of their own and
idx_offset 7) x weights (None, [D], [Q, D]) x select (None, a bool tensor with 4096 rows on, the same as a Selection, a Selection
with rows in the first three tiles only -- below SELECT_MIN_LIVE_TILES --, an empty Selection) x Q (0, 1, 16, 17, 40) x k (KS: 1) x prune
(PRUNES) x SKYEMB_TOPK_PREFILTER (unset, '0'); ``cosine_scores`` over the fp32 tensor, the fp32 PreparedBank and a 16-bit one; and
the refusals of ``REFUSALS``.  Section 'tokens' (N = 2304 images, P = 4, D = 128, TokenBank.resident of fp16 and of bf16, the four
TOKEN_*_MIN_Q* thresholds at 17): ``cosine_topk_tokens`` over combine (min, max, mean) x top_t (None, 1, 2, 4) x select (None, a
Selection of 2048 images, one of 600) x Q (17, 40) x k (KS); what the two-stage route refuses falls to the grouped route and is
recorded as it falls.  Query 20 is all zeros, so every Q = 40 search has a query stage 1 cannot bound; ``main`` fails unless each
two-stage driver (``DRIVERS``) re-ran a query in at least one recorded case.  A section's cases run in order on a fresh fixture:
what a bank or a Selection keeps from one search to the next is part of what is recorded.

File: {"args": [distinct op names and argument descriptions], "ops": [distinct call records: indices into args, the name
first], "traces": [distinct sequences of indices into ops], "digests": [distinct digests or [exception type, text]], "cases": [trace index, digest index,
trace index, ...] flat, in the order of ``cases()``}; ``calls`` reads a trace back.
"""
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from sky_embeddings_amd import ops, search  # noqa: E402
from tests.golden.make_token_trace_golden import Recorder, Table, digest  # noqa: E402,F401

OUT = os.environ.get("SKYEMB_GOLDEN_OUT") or HERE
N, D, QMAX, ZERO_QUERY = 4608, 128, 40, 20
TN, TP = 2304, 4
KS, PRUNES = (1,), (True, False)      # k = 5 as well puts the file past its size limit; at k = 1 the pruning floors engage (N >= 2048)
BANKS = ("f32", "f16", "pb32", "pb16", "res_bf16", "res_f16")
SELECTS = ("none", "bool", "Selection", "Selection3tiles", "SelectionEmpty")
REFUSALS = ("k=0", "k>N", "pb_select_Q16", "pb_weightsQD", "PreparedBank(bf16)", "PreparedBank(misaligned)",
            "TokenBank.resident(misaligned)", "ops.bank16_rowp_lp(misaligned)", "ops.resident_rowp(misaligned)", "select_length")
THRESHOLDS = ("TOKEN_PREFILTER_MIN_Q", "TOKEN_MEAN_PREFILTER_MIN_Q", "TOKEN_TOPT_PREFILTER_MIN_Q", "TOKEN_TOPT_PREFILTER_MIN_Q_SMALL")
DRIVERS = ("rows", "rows under a selection", "tokens", "tokens under a selection", "mean")
SECTIONS = ("rows", "tokens")


def cases():
    """-> [(case id, section, kind, ...)] in a fixed order.  kind 'topk': bank, weights, select, Q, k, prune, switch; 'scores': bank;
    'refusal': its name, bank; 'tokens': dtype, combine, top_t, select, Q, k."""
    out = []
    for c in itertools.product(BANKS, ("none", "D", "QD"), SELECTS, (0, 1, 16, 17, 40), KS, PRUNES, (None, "0")):
        out.append(("rows", "topk", *c))
    for bank in ("f32", "pb32", "res_bf16"):
        out.append(("rows", "scores", bank))
    for name in REFUSALS:
        for bank in (BANKS if name in ("k=0", "k>N") else ("pb32", "res_bf16") if name.startswith("pb_") else
                     ("f32", "pb32") if name == "select_length" else ("-",)):
            out.append(("rows", "refusal", name, bank))
    for c in itertools.product(("f16", "bf16"), ("min", "max", "mean"), (None, 1, 2, 4), ("none", "Selection2048", "Selection600"), (17, 40), KS):
        out.append(("tokens", "tokens", *c))
    return [("|".join(str(x) for x in c), *c) for c in out]


def _flags(n, on, g, first=None):
    f = torch.zeros(n, dtype=torch.bool)
    f[torch.randperm(n if first is None else first, generator=g)[:on]] = True
    return f


class RowFixture:
    """The seeded row bank, queries, weights and selections of section 'rows' (built before anything is recorded)."""

    def __init__(self, device="cuda"):
        g = torch.Generator().manual_seed(2210)
        f32 = torch.randn(N, D, generator=g).to(device)
        q = torch.randn(QMAX, D, generator=g)
        q[ZERO_QUERY] = 0.0
        self.q = q.to(device)
        self.wD = (torch.rand(D, generator=g) + 0.1).to(device)
        self.wQD = (torch.rand(QMAX, D, generator=g) + 0.1).to(device)
        wPB = (torch.rand(D, generator=g) + 0.1).to(device)      # the PreparedBanks' own weights
        self.f16, self.bf16 = f32.half(), f32.bfloat16()
        self.banks = {"f32": f32, "f16": self.f16, "pb32": search.PreparedBank(f32, wPB, idx_offset=7),
                      "pb16": search.PreparedBank(self.f16, wPB, idx_offset=7),
                      "res_bf16": search.PreparedBank.resident(self.bf16, wPB, idx_offset=7),
                      "res_f16": search.PreparedBank.resident(self.f16.clone(), wPB, idx_offset=7)}
        on = _flags(N, 4096, g).to(device)
        self.selects = {"none": None, "bool": on, "Selection": search.Selection(on),
                        "Selection3tiles": search.Selection(_flags(N, 500, g, first=768).to(device)),
                        "SelectionEmpty": search.Selection(torch.zeros(N, dtype=torch.bool, device=device))}
        self.short = search.Selection(torch.ones(N - 1, dtype=torch.bool, device=device))
        odd = torch.empty(N * D + 8, device=device, dtype=torch.float16)[4:4 + N * D]       # 8 bytes past a 16-byte boundary
        odd.copy_(self.f16.view(-1))
        self.odd = odd.view(N, D)
        assert self.odd.is_contiguous() and self.odd.data_ptr() % 16 == 8

    def weights(self, w, Qn):
        return {"none": None, "D": self.wD, "QD": self.wQD[:Qn]}[w]

    def refusal(self, name, bank):
        """The refused call ``name``, as a function of no arguments."""
        q17, b = self.q[:17], self.banks.get(bank)
        norms = self.banks["pb16"].norms
        return {"k=0": lambda: search.cosine_topk(q17, b, 0),
                "k>N": lambda: search.cosine_topk(q17, b, N + 1),
                "pb_select_Q16": lambda: search.cosine_topk(self.q[:16], b, 5, select=self.selects["Selection"]),
                "pb_weightsQD": lambda: search.cosine_topk(q17, b, 5, weights=self.wQD[:17]),
                "PreparedBank(bf16)": lambda: search.PreparedBank(self.bf16),
                "PreparedBank(misaligned)": lambda: search.PreparedBank(self.odd),
                "TokenBank.resident(misaligned)": lambda: search.TokenBank.resident(self.odd.view(N // 4, 4, D)),
                "ops.bank16_rowp_lp(misaligned)": lambda: ops.bank16_rowp_lp(self.odd, norms),
                "ops.resident_rowp(misaligned)": lambda: ops.resident_rowp(self.odd, norms),
                "select_length": lambda: search.cosine_topk(q17, b, 5, select=self.short)}[name]


class TokenFixture:
    """The seeded resident token banks, queries and selections of section 'tokens'."""

    def __init__(self, device="cuda"):
        g = torch.Generator().manual_seed(2211)
        f32 = torch.randn(TN, TP, D, generator=g).to(device)
        q = torch.randn(QMAX, D, generator=g)
        q[ZERO_QUERY] = 0.0
        self.q = q.to(device)
        w = (torch.rand(D, generator=g) + 0.1).to(device)
        self.banks = {"f16": search.TokenBank.resident(f32.half(), w, idx_offset=7),
                      "bf16": search.TokenBank.resident(f32.bfloat16(), w, idx_offset=7)}
        self.selects = {"none": None, "Selection2048": search.Selection(_flags(TN, 2048, g).to(device)),
                        "Selection600": search.Selection(_flags(TN, 600, g).to(device))}


FIXTURES = {"rows": RowFixture, "tokens": TokenFixture}


def set_thresholds(setattr_fn):
    """The smallest Q of every two-stage token route down to 17, as tests/test_token_prefilter_gpu.py sets them (``setattr_fn``: see
    ``Recorder``; whoever passes it puts them back)."""
    for name in THRESHOLDS:
        setattr_fn(search, name, 17)


def _call(fx, case, stats):
    kind = case[2]
    if kind == "topk":
        _, _, _, bank, w, sel, Qn, k, prune, _ = case
        return lambda: search.cosine_topk(fx.q[:Qn], fx.banks[bank], k, weights=fx.weights(w, Qn), prune=prune, stats=stats,
                                          select=fx.selects[sel])
    if kind == "scores":
        return lambda: search.cosine_scores(fx.q[:17], fx.banks[case[3]])
    if kind == "refusal":
        return fx.refusal(case[3], case[4])
    _, _, _, dt, combine, t, sel, Qn, k = case
    return lambda: search.cosine_topk_tokens(fx.q[:Qn], fx.banks[dt], k, combine, stats=stats, top_t=t, select=fx.selects[sel])


def run_case(fx, rec, case):
    """-> (trace: the ops calls of this call + its stats, digest of the returned tensors or [exception type, text])."""
    stats = {}
    call = _call(fx, case, stats)
    switch = case[9] if case[2] == "topk" else None
    saved = os.environ.pop("SKYEMB_TOPK_PREFILTER", None)
    if switch is not None:
        os.environ["SKYEMB_TOPK_PREFILTER"] = switch
    del rec.log[:]
    try:
        result = digest(call())
    except ValueError as e:                                   # a refusal: recorded, never digested (anything else ends the run)
        result = [type(e).__name__, str(e)]
    finally:
        os.environ.pop("SKYEMB_TOPK_PREFILTER", None)
        if saved is not None:
            os.environ["SKYEMB_TOPK_PREFILTER"] = saved
    return list(rec.log) + [["stats", [], dict(sorted(stats.items()))]], result


def driver(case, trace):
    """The two-stage driver that re-ran a query in this case (one of ``DRIVERS``), or None."""
    stats = trace[-1][2]
    if stats.get("path") != "prefiltered" or not stats.get("redone", 0) >= 1:
        return None
    if case[2] == "topk":
        return "rows under a selection" if "selected" in stats else "rows"
    return "mean" if stats["combine"] == "mean" else "tokens under a selection" if "selected" in stats else "tokens"


def record():
    """-> (the file's content, the drivers that re-ran a query)."""
    saved = []

    def put(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    args_t, ops_t, traces_t, digests_t, table, redone = Table(), Table(), Table(), Table(), [], set()
    try:
        set_thresholds(put)
        all_cases = cases()
        fixtures = {s: FIXTURES[s]() for s in SECTIONS}
        rec = Recorder(put)
        for case in all_cases:
            trace, result = run_case(fixtures[case[1]], rec, case)
            trace = json.loads(json.dumps(trace))
            redone.add(driver(case, trace))
            table += [traces_t.add([ops_t.add([args_t.add(a) for a in (call[0], *call[1], *call[2:])]) for call in trace]),
                      digests_t.add(result)]
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)
    return {"args": args_t.items, "ops": ops_t.items, "traces": traces_t.items, "digests": digests_t.items, "cases": table}, redone


def calls(z, ti):
    """Trace ``ti`` of the file's content ``z`` as ``run_case`` returns it."""
    out = []
    for i in z["traces"][ti]:
        name, *args = (z["args"][a] for a in z["ops"][i])
        out.append([name, [], *args] if name == "stats" else [name, args])
    return out


def main():
    z, redone = record()
    missing = [d for d in DRIVERS if d not in redone]
    assert not missing, f"no recorded case re-ran a query on: {missing}"
    path = os.path.join(OUT, "row_search_trace.json")
    with open(path, "w") as f:
        json.dump(z, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "token_search_trace.json"))
    print("wrote", path, len(z["cases"]) // 2, "cases,", len(z["traces"]), "distinct traces,", len(z["ops"]), "distinct calls,",
          len(z["digests"]), "distinct results,", size, "bytes")
    assert size < limit, f"{size} bytes: not below token_search_trace.json's {limit}; trim KS, then PRUNES"


if __name__ == "__main__":
    main()
