#!/usr/bin/env python3
"""Generate tests/golden/token_search_trace.json: for a fixed matrix of patch-token searches on a seeded bank, the sequence of
``ops`` calls the Python layer makes (name and, per parameter of the op, None / the scalar / (shape, dtype) of a tensor), the ``stats`` dict
and a SHA-256 digest of the returned tensors.  Recorded on a GPU from the commit BEFORE a change to that layer, so that
tests/test_token_host_gpu.py can hold the changed layer to the same launches and the same bits.

Usage (on a machine with a GPU, at the commit whose behaviour is the reference):
    python tests/golden/make_token_trace_golden.py

Matrix: the four public functions x bank (fp32 tensor, fp16 tensor, TokenBank with weights of its own) x weights (None, [D], [Q, D]) x select (None,
bool tensor, Selection; 4096 of the 4608 images, so the floor still engages) x top_t (None, 2) x Q (0, 1, 17) x prune (on, off;
the two top-k functions), at N = 4608, P = 4, D = 64, k = 1.  Extras: a Selection of 1000 images (the size rule turns the floor
off) and a bank of N = 64 images (no floor).  ``cases()``, ``Fixture``, ``Recorder`` and ``run_case`` are what the test imports; ``Recorder``, ``describe``, ``digest`` and ``Table``
serve tests/golden/make_row_trace_golden.py too.

File: {"ops": [distinct call records], "traces": [distinct sequences of indices into ops], "digests": [distinct digests],
"cases": [[trace index, digest index], ...] in the order of ``cases()``} -- sequences and digests repeat a lot, so each is stored
once, and a case is named by its place in the list.
"""
import hashlib
import inspect
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from sky_embeddings_amd import search  # noqa: E402

OUT = os.environ.get("SKYEMB_GOLDEN_OUT") or HERE
N, N_SMALL, P, D, K, QMAX = 4608, 64, 4, 64, 1, 17
FUNCTIONS = ("cosine_topk_tokens", "cosine_token_scores", "distance_topk_tokens", "distance_token_scores")
TOPK = ("cosine_topk_tokens", "distance_topk_tokens")


def cases():
    """-> [(case id, function, bank, weights, select, top_t, Q, prune)] in a fixed order."""
    out = []
    for fn in FUNCTIONS:
        prunes = (True, False) if fn in TOPK else (None,)
        for bank, w, sel, t, Qn, prune in itertools.product(("f32", "f16", "tb"), ("none", "D", "QD"), ("none", "bool", "Selection"),
                                                           (None, 2), (0, 1, 17), prunes):
            out.append((fn, bank, w, sel, t, Qn, prune))
        for w, Qn in itertools.product(("none", "QD"), (1, 17)):
            if fn in TOPK:
                out.append((fn, "f32", w, "Selection1000", None, Qn, True))
            out.append((fn, "f32small", w, "none", None, Qn, prunes[0]))
    return [("|".join(str(x) for x in c), *c) for c in out]


class Fixture:
    """The seeded bank, queries, weights and selections of the matrix (device tensors; built before anything is recorded)."""

    def __init__(self, device="cuda"):
        g = torch.Generator().manual_seed(1504)
        bank = torch.randn(N, P, D, generator=g)
        self.q = torch.randn(QMAX, D, generator=g).to(device)
        self.wD = (torch.rand(D, generator=g) + 0.1).to(device)
        self.wQD = (torch.rand(QMAX, D, generator=g) + 0.1).to(device)
        on = torch.zeros(N, dtype=torch.bool)
        on[torch.randperm(N, generator=g)[:4096]] = True
        on1000 = torch.zeros(N, dtype=torch.bool)
        on1000[torch.randperm(N, generator=g)[:1000]] = True
        f32 = bank.to(device)
        wTB = (torch.rand(D, generator=g) + 0.1).to(device)      # the TokenBank's own weights: not the [D] argument, which it replaces
        self.banks = {"f32": f32, "f16": f32.half(), "tb": search.TokenBank(f32, wTB, idx_offset=7),
                      "f32small": f32[:N_SMALL].contiguous()}
        flags = on.to(device)
        self.selects = {"none": None, "bool": flags, "Selection": search.Selection(flags), "Selection1000": search.Selection(on1000.to(device))}

    def weights(self, w, Qn):
        return {"none": None, "D": self.wD, "QD": self.wQD[:Qn]}[w]


_SHORT = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16", torch.int64: "i64", torch.int32: "i32", torch.uint8: "u8",
          torch.bool: "bool"}


def describe(x):
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, torch.Tensor):                       # (shape, dtype) as one short string: "f32[4608,4,64]"
        return f"{_SHORT[x.dtype]}[{','.join(str(n) for n in x.shape)}]"
    if isinstance(x, (tuple, list)):                      # a prepared selection and the like: item by item; a long host list: its length
        if len(x) > 8 and all(isinstance(v, (int, float)) for v in x):
            return f"list[{len(x)}]"
        return [describe(v) for v in x]
    return str(x)


def _bound(sig, args, kw):
    """The call as the op receives it: every parameter in the signature's order, defaults filled in -- so leaving a default out
    and passing its value are the same call.  (*args of an op stay a nested list.)"""
    b = sig.bind(*args, **kw)
    b.apply_defaults()
    return [list(v) if isinstance(v, tuple) else v for v in b.arguments.values()]


class Recorder:
    """Wraps every public function that ``search.ops`` defines with a pass-through that logs the call.  ``setattr_fn(obj, name,
    value)`` installs a wrapper (a test passes ``monkeypatch.setattr``, which also takes them off again)."""

    def __init__(self, setattr_fn):
        self.log = []
        ops = search.ops
        for name, fn in sorted(vars(ops).items()):
            if inspect.isfunction(fn) and fn.__module__ == ops.__name__ and not name.startswith("_"):
                setattr_fn(ops, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        def logged(*args, **kw):
            self.log.append([name, _bound(sig, [describe(a) for a in args], {key: describe(v) for key, v in kw.items()})])
            return fn(*args, **kw)
        sig = inspect.signature(fn)
        return logged


def digest(got):
    """SHA-256 over shape, dtype and bytes of the returned tensor(s)."""
    h = hashlib.sha256()
    for x in (got if isinstance(got, tuple) else (got,)):
        h.update(repr((tuple(x.shape), str(x.dtype))).encode())
        h.update(x.cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def run_case(fx, rec, case):
    """-> (trace: the ops calls of this search + its stats, digest of the returned tensors)."""
    _, fn, bank, w, sel, t, Qn, prune = case
    kw = dict(weights=fx.weights(w, Qn), top_t=t, select=fx.selects[sel])
    stats = {}
    if fn in TOPK:
        kw.update(k=K, prune=prune, stats=stats)
    del rec.log[:]
    got = getattr(search, fn)(fx.q[:Qn], fx.banks[bank], **kw)
    trace = list(rec.log) + [["stats", [], dict(sorted(stats.items()))]]        # a last pseudo-call: the stats dict
    return trace, digest(got)


class Table:
    def __init__(self):
        self.items, self.index = [], {}

    def add(self, item):
        key = json.dumps(item, sort_keys=True)
        if key not in self.index:
            self.index[key] = len(self.items)
            self.items.append(item)
        return self.index[key]


def main():
    fx = Fixture()
    saved = []

    def put(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    rec = Recorder(put)
    ops_t, traces_t, digests_t, table = Table(), Table(), Table(), []
    try:
        for case in cases():
            trace, digest = run_case(fx, rec, case)
            table.append([traces_t.add([ops_t.add(call) for call in trace]), digests_t.add(digest)])
    finally:
        for obj, name, value in saved:
            setattr(obj, name, value)
    path = os.path.join(OUT, "token_search_trace.json")
    with open(path, "w") as f:
        json.dump({"ops": ops_t.items, "traces": traces_t.items, "digests": digests_t.items, "cases": table}, f, separators=(",", ":"),
                  sort_keys=True)
        f.write("\n")
    print("wrote", path, len(table), "cases,", len(traces_t.items), "distinct traces,", len(ops_t.items), "distinct calls,",
          len(digests_t.items), "distinct results,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
