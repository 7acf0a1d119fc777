"""GPU: the host layer of the patch-token search makes the launches it made before its consolidation and returns the same bits.
Every public function of ``search.ops`` is wrapped with a pass-through recorder; a fixed matrix of searches over a seeded bank
(tests/golden/make_token_trace_golden.py states it) is compared, call by call, with tests/golden/token_search_trace.json, which that
script recorded from the layer as it was: op names, per argument None / the scalar / (shape, dtype), the ``stats`` dict, and a
SHA-256 digest of the returned tensors."""
import json
import os

import pytest

from tests.golden import make_token_trace_golden as golden

pytestmark = pytest.mark.gpu

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_search_trace.json")


@pytest.fixture(scope="module")
def fixture():
    return golden.Fixture()


@pytest.mark.parametrize("fn", golden.FUNCTIONS)
def test_same_ops_calls_same_stats_same_bits(fn, fixture, monkeypatch):
    with open(PATH) as f:
        z = json.load(f)
    cases = golden.cases()
    assert len(cases) == len(z["cases"]) == 996
    rec = golden.Recorder(monkeypatch.setattr)
    n = 0
    for case, (ti, di) in zip(cases, z["cases"]):
        if case[1] != fn:
            continue
        trace, digest = golden.run_case(fixture, rec, case)
        want = [z["ops"][i] for i in z["traces"][ti]]
        got = json.loads(json.dumps(trace))                            # tuples -> lists, as the golden went through JSON
        assert got == want, (case[0], [(a, b) for a, b in zip(got, want) if a != b][:3], len(got), len(want))
        assert digest == z["digests"][di], case[0]
        n += 1
    assert n == (332 if fn in golden.TOPK else 166)
