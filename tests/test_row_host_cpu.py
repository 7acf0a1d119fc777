"""CPU: the request plan of the row-bank search (``search._row_request``) -- per case of a small table the route it chooses, what
it hands that route, and which refusal comes first.  The texts and their order are those tests/golden/row_search_trace.json
recorded from the layer before its consolidation (tests/test_row_host_gpu.py replays them on a GPU).  No device is touched: the
banks are CPU tensors and stand-ins for a PreparedBank and a Selection."""
import dataclasses

import pytest
import torch

from sky_embeddings_amd import search

N, D = 4608, 128


def _pb(dtype=torch.float32, n=N):
    """A PreparedBank stand-in (building one needs a device): the fields the request reads."""
    pb = search.PreparedBank.__new__(search.PreparedBank)
    pb.bank, pb.dtype, pb.idx_offset = torch.zeros(n, D, dtype=dtype), dtype, 7
    pb._tokens = None if dtype == torch.float32 else ("the one-token TokenBank of", pb)
    return pb


def _selection(n=N):
    sel = search.Selection.__new__(search.Selection)
    sel.N, sel.count = n, n // 2
    return sel


def _request(Q, bank, k=5, weights=None, select=None, world_size=1):
    return search._row_request("cosine_topk", torch.zeros(Q, D), bank, k, weights, select, world_size)


@pytest.fixture(autouse=True)
def _switch_unset(monkeypatch):
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)


FLAT32, FLAT16, FLATBF = (torch.zeros(N, D, dtype=t) for t in (torch.float32, torch.float16, torch.bfloat16))
FLAGS = torch.ones(N, dtype=torch.bool)

ROUTES = [
    # (Q, bank, weights, select, switch off) -> (route, rerun)
    ((0, "pb32", None, None, False), ("empty", None)),
    ((1, "pb32", None, None, False), ("exact", None)),
    ((16, "flat32", None, None, False), ("exact", None)),
    ((17, "flat32", None, None, False), ("prefiltered", "exact")),
    ((40, "pb32", "D", None, False), ("prefiltered", "exact")),
    ((40, "pb32", None, None, True), ("exact", None)),
    ((0, "pb16", None, None, False), ("empty", None)),
    ((16, "pb16", None, None, False), ("tokens", None)),
    ((40, "pb16", None, None, False), ("prefiltered", "tokens")),
    ((40, "pbbf", None, None, False), ("prefiltered", "tokens")),
    ((40, "pbbf", None, None, True), ("tokens", None)),
    ((40, "pb32", None, "Selection", False), ("prefiltered", "tokens")),
    ((17, "pb16", "D", "Selection", False), ("prefiltered", "tokens")),
    ((0, "flat16", None, None, False), ("tokens", None)),
    ((40, "flatbf", None, None, False), ("tokens", None)),
    ((40, "flat32", "QD", None, False), ("tokens", None)),
    ((40, "flat32", None, "bool", False), ("tokens", None)),
    ((40, "flat16", "QD", "Selection", True), ("tokens", None)),
]


@pytest.mark.parametrize("case,want", ROUTES, ids=[str(c) for c, _ in ROUTES])
def test_route_and_what_it_is_handed(case, want, monkeypatch):
    Q, b, w, s, off = case
    if off:
        monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    bank = {"pb32": _pb(), "pb16": _pb(torch.float16), "pbbf": _pb(torch.bfloat16), "flat32": FLAT32, "flat16": FLAT16, "flatbf": FLATBF}[b]
    weights = {None: None, "D": torch.ones(D), "QD": torch.ones(Q, D)}[w]
    select = {None: None, "bool": FLAGS, "Selection": _selection()}[s]
    rq = _request(Q, bank, 5, weights, select)
    assert (rq.route, rq.rerun) == want
    assert (rq.Q, rq.N, rq.D, rq.k) == (Q, N, D, 5)
    if rq.route != "tokens":                               # the bank as given; a PreparedBank's own weights count; the Selection
        assert rq.bank is bank and rq.weights is None and rq.select is select
    elif isinstance(bank, search.PreparedBank):            # its one-token TokenBank, nothing else
        assert rq.bank is bank._tokens and rq.weights is None and rq.select is None
    else:                                                  # one token per row, a view; weights and select as the caller gave them
        assert tuple(rq.bank.shape) == (N, 1, D) and rq.bank.data_ptr() == bank.data_ptr()
        assert rq.weights is weights and rq.select is select
    with pytest.raises(dataclasses.FrozenInstanceError):
        rq.route = "exact"


PER_QUERY = "cosine_topk: per-query weights [Q, D] are served by the token search"
SELECT_PB = "cosine_topk: select is served by the token search"
REFUSALS = [
    # (Q, bank, k, weights, select, switch off) -> how the first refusal starts
    ((40, "pb32", 0, "QD", "Selection", False), PER_QUERY),                 # before select, before k
    ((40, "3d", 5, "QD", "short", False), PER_QUERY),
    ((40, "3d", 0, None, "Selection", False), "cosine_topk: select needs a flat [N, D] bank tensor"),
    ((16, "pb32", N + 1, None, "short", False), SELECT_PB),                 # Q <= 16: before k and the selection's length
    ((0, "pbbf", 5, None, "Selection", False), SELECT_PB),                  # Q = 0 under a selection is refused, not 'empty'
    ((40, "pb32", 0, None, "Selection", False), SELECT_PB),                 # k < 1 is not a shape the two-stage path takes
    ((40, "pb32", 193, None, "Selection", False), SELECT_PB),
    ((40, "small", 5, None, "Selection", False), SELECT_PB),                # N < 2048
    ((40, "pb16", 5, None, "Selection", True), SELECT_PB),                  # the switch off
    ((40, "pb32", 5, None, "short", False), "cosine_topk: select describes 4607 images, the bank has 4608"),
    ((0, "pb32", 0, None, None, False), "cosine_topk: k = 0"),              # before Q = 0 is 'empty'
    ((0, "pb16", N + 1, None, None, False), "cosine_topk: k = 4609 exceeds the 4608 rows of the bank"),
    ((40, "flat32", 0, None, None, True), "cosine_topk: k = 0"),
    ((40, "pbbf", -1, None, None, False), "cosine_topk: k = -1"),
]


@pytest.mark.parametrize("case,text", REFUSALS, ids=[str(c) for c, _ in REFUSALS])
def test_order_of_refusals(case, text, monkeypatch):
    Q, b, k, w, s, off = case
    if off:
        monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    bank = {"pb32": _pb(), "pb16": _pb(torch.float16), "pbbf": _pb(torch.bfloat16), "small": _pb(n=2047), "flat32": FLAT32,
            "3d": torch.zeros(N, 1, D)}[b]
    n = bank.bank.shape[0] if isinstance(bank, search.PreparedBank) else N
    select = {None: None, "Selection": _selection(n), "short": _selection(n - 1)}[s]
    with pytest.raises(ValueError) as e:
        _request(Q, bank, k, torch.ones(Q, D) if w == "QD" else None, select)
    assert str(e.value).startswith(text), str(e.value)


def test_k_may_exceed_the_shard_when_ranks_merge():
    assert _request(40, _pb(n=2048), 100, world_size=2).route == "prefiltered"
    assert _request(3, _pb(n=2), 5, world_size=2).route == "exact"
    with pytest.raises(ValueError, match="exceeds the 2 rows"):
        _request(3, _pb(n=2), 5)
