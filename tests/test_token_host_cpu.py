"""CPU: the host layer of the patch-token search (sky_embeddings_amd/search.py) -- every refusal of a fixed list of bad requests
has the text and the precedence recorded from the layer before its consolidation (tests/golden/token_search_refusals.json, written
by tests/golden/make_token_refusal_golden.py), and the request plan follows its stated rules.  No device is touched."""
import dataclasses
import json
import os

import pytest
import torch

from sky_embeddings_amd import ops, search
from tests.golden import make_token_refusal_golden as refusals

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_every_listed_refusal_has_the_recorded_text_and_precedence():
    with open(os.path.join(GOLDEN, "token_search_refusals.json")) as f:
        z = json.load(f)
    cases = refusals.cases()
    assert sorted(cid for cid, _, _ in cases) == sorted(z["cases"]) and len(cases) > 600
    for cid, fn, req in cases:
        e = refusals.run(fn, req)
        assert [type(e).__name__, str(e)] == z["messages"][z["cases"][cid]], cid


def _request(Q, N, P, D, k, per_query, **kw):
    args = dict(who="t", queries=torch.zeros(Q, D), bank=torch.zeros(N, P, D), k=k, combine="min", metric=search._COSINE,
                weights=torch.ones(Q, D) if per_query else None, top_t=None, select=None)
    args.update(kw)
    return search._token_request(**args)


@pytest.mark.parametrize("D", (64, 768, 1024))
def test_step_and_groups_follow_the_stated_rule(D):
    """Shared weights: 16 queries per pass, under the shape rule 64 D + 32 min(Q, 16) k <= 163840.  Per-query weights: the largest
    g <= 16 with 128 D + 32 g k <= 163840 (a ValueError when not even g = 1 fits; here one always does)."""
    N, P = 320, 4
    for Q in (1, 16, 17, 35):
        for k in (1, 100, 300):
            for per_query in (False, True):
                for kk in (k, None):                               # None: a scores call, planned at k = 1
                    ke = 1 if kk is None else kk
                    if per_query:
                        step = max(g for g in range(1, 17) if 128 * D + 32 * g * ke <= 163840)
                    elif 64 * D + 32 * min(Q, 16) * ke > 163840:
                        with pytest.raises(ValueError, match="64 D"):
                            _request(Q, N, P, D, kk, per_query)
                        continue
                    else:
                        step = 16
                    rq = _request(Q, N, P, D, kk, per_query)
                    assert (rq.step, rq.groups) == (step, -(-Q // step)), (Q, D, kk, per_query)
                    assert (rq.Q, rq.N, rq.P, rq.D, rq.k, rq.per_query) == (Q, N, P, D, ke, per_query)


def test_codes_weights_and_offset_of_the_request():
    Q, N, P, D = 3, 40, 4, 64
    for name, code in ops.COMBINE_CODES.items():
        assert _request(Q, N, P, D, 2, False, combine=name).combine == code
    assert _request(Q, N, P, D, 2, False).metric is None and _request(Q, N, P, D, 2, False).metric_name is None
    for name, code in ops.METRIC_CODES.items():
        rq = _request(Q, N, P, D, 2, False, metric=name)
        assert (rq.metric, rq.metric_name) == (code, name)
    assert [_request(Q, N, P, D, 2, False, top_t=t).top_t for t in (None, 1, 4)] == [0, 1, 4]
    # a plain tensor: no offset, the argument's weights count
    w = torch.ones(D)
    rq = _request(Q, N, P, D, 2, False, weights=w)
    assert rq.idx_offset == 0 and rq.bank is None and rq.weights is w and rq.select is None
    # a TokenBank (a stand-in: building one needs a device): its offset, its tokens, its own weights instead of a [D] argument ...
    tb = search.TokenBank.__new__(search.TokenBank)
    tb.bank, tb.idx_offset, tb.weights = torch.zeros(N, P, D), 1000, torch.full((D,), 2.0)
    rq = _request(Q, N, P, D, 2, False, bank=tb, weights=w)
    assert rq.idx_offset == 1000 and rq.bank is tb and rq.tokens is tb.bank and rq.weights is tb.weights and not rq.per_query
    # ... which a [Q, D] argument overrides
    W = torch.ones(Q, D)
    rq = _request(Q, N, P, D, 2, True, bank=tb, weights=W)
    assert rq.per_query and rq.weights is W and rq.idx_offset == 1000 and rq.step == 16
    with pytest.raises(dataclasses.FrozenInstanceError):
        rq.step = 1
