"""GPU: the host layer of the row-bank search and of the two-stage token routes makes the launches it made before its consolidation,
returns the same bits and refuses the same calls in the same words.  Every public function of ``search.ops`` is wrapped with a
pass-through recorder; the fixed matrix of tests/golden/make_row_trace_golden.py (which states it) is compared, call by call, with
tests/golden/row_search_trace.json, which that script recorded from the layer as it was: op names, per argument None / the scalar /
(shape, dtype), the ``stats`` dict, and a SHA-256 digest of the returned tensors or the exception's type and text."""
import json
import os

import pytest

from tests.golden import make_row_trace_golden as golden

pytestmark = pytest.mark.gpu

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_search_trace.json")
COUNTS = {"rows": 1826, "tokens": 144}


@pytest.mark.parametrize("section", golden.SECTIONS)
def test_same_ops_calls_same_stats_same_bits_same_refusals(section, monkeypatch):
    with open(PATH) as f:
        z = json.load(f)
    cases = golden.cases()
    assert len(cases) == len(z["cases"]) // 2 == 1970
    golden.set_thresholds(monkeypatch.setattr)
    monkeypatch.delenv("SKYEMB_PREFILTER_LO", raising=False)
    fixture = golden.FIXTURES[section]()                                   # fresh: what banks and Selections keep is part of the trace
    rec = golden.Recorder(monkeypatch.setattr)
    n, redone = 0, set()
    for case, ti, di in zip(cases, z["cases"][0::2], z["cases"][1::2]):
        if case[1] != section:
            continue
        trace, result = golden.run_case(fixture, rec, case)
        want = golden.calls(z, ti)
        got = json.loads(json.dumps(trace))                                # tuples -> lists, as the golden went through JSON
        assert got == want, (case[0], [(a, b) for a, b in zip(got, want) if a != b][:3], len(got), len(want))
        assert result == z["digests"][di], case[0]
        redone.add(golden.driver(case, got))
        n += 1
    assert n == COUNTS[section]
    assert redone - {None} == set(golden.DRIVERS[:2] if section == "rows" else golden.DRIVERS[2:])
