"""CPU: the two-stage many-query patch-token search -- its image-level stage-1 test restated in numpy (tests/
token_prefilter_reference.py) never drops a top-k image and keeps the candidate lists of the GPU cases inside their capacity; the
route decision is one pure function; the new symbols are exported as declared."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from sky_embeddings_amd import _lib, ops, search
from tests import token_prefilter_reference as tpr
from tests import token_search_reference as tsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case_arrays(c):
    P, combine, dt, lo, Q, tail, D, k, weighted, off = c
    q, bank, xw, w = tpr.case_inputs(P, tail, D, Q, weighted, dt)
    exact = tsr.combined_scores(q, xw, combine, w)
    return q, xw, w, exact


@pytest.mark.parametrize("c", tpr.CASES, ids=tpr.case_id)
def test_no_topk_image_is_dropped_and_the_lists_hold(c):
    """Every image of the oracle's top-k passes the image test at tau = the query's exact k-th best, under every flush model; and
    with tau as the design maintains it (bootstrap sample, then the exact k-th best of the images decided so far) the candidates
    of every slice fit the list and the staging region for at least 90 % of the queries (the condition behind the GPU test's cap on
    ``redone``)."""
    P, combine, dt, lo, Q, tail, D, k, weighted, off = c
    dtype = tpr.DTYPES[dt]
    q, xw, w, exact = _case_arrays(c)
    N = xw.shape[0]
    rows = xw.reshape(N * P, D)
    eps_a = ops.topk_prefilter_eps_a_resident(D, dtype, lo=lo)
    ref_s, ref_i = tsr.topk_of_scores(exact, k)
    tau = ref_s[:, k - 1].astype(np.float64)                       # -inf where fewer than k images score above -inf
    worst = None
    for flush in tpr.flush_models(dtype):
        lhs, coef, ub = tpr.row_margins(q, rows, w, dtype, lo, flush, eps_a)
        ok = tpr.image_pass(lhs, coef, ub, tau, P, combine)
        for qi in range(Q):
            top = ref_i[qi][ref_i[qi] >= 0]
            assert ok[qi, top].all(), (flush, qi, top[~ok[qi, top]][:5])
        counts, flagged = tpr.simulate(exact, lhs, coef, ub, P, k, combine, lo)
        assert flagged.sum() <= Q // 10, (flush, int(flagged.sum()), counts.max(axis=1))
        worst = counts.max(axis=1) if worst is None else np.maximum(worst, counts.max(axis=1))
    print(tpr.case_id(c), "largest candidate count per slice:", worst.tolist(), "of", tpr.list_cap(k))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("combine", ["min", "max"])
def test_an_image_with_an_unboundable_row_always_passes_where_it_can_count(dtype, combine):
    """Rows with a NaN or an inf element (bf16: an element outside [2^-60, 2^120) too) pass the row test at every threshold, so
    under 'max' their image always passes, and under 'min' it passes whenever its other rows do."""
    rng = np.random.default_rng(3)
    N, P, D = 64, 4, 128
    q = rng.standard_normal((5, D), dtype=np.float32)
    x = rng.standard_normal((N, P, D), dtype=np.float32)
    x[3, 1, 5] = np.nan
    x[7, 0, 9] = np.inf
    if dtype == torch.bfloat16:
        x[9, 2, 1] = 2.0 ** -70
        x[11, 3, 2] = 2.0 ** 121
    _, xw = tpr.to16(x, dtype)
    eps_a = ops.topk_prefilter_eps_a_resident(D, dtype, lo=False)
    flush = tpr.flush_models(dtype)[-1]
    lhs, coef, ub = tpr.row_margins(q, xw.reshape(N * P, D), None, dtype, False, flush, eps_a)
    bad = [3 * P + 1, 7 * P] + ([9 * P + 2, 11 * P + 3] if dtype == torch.bfloat16 else [])
    assert ub[bad].all() and ub.sum() == len(bad)
    far = np.full(5, 1e30)                                         # a threshold no ordinary row reaches
    ok = tpr.image_pass(lhs, coef, ub, far, P, combine)
    images = [b // P for b in bad]
    if combine == "max":
        assert ok[:, images].all() and ok.sum() == 5 * len(images)
    else:
        assert not ok.any()                                        # their other rows fail, and with them the image
        ok = tpr.image_pass(lhs, coef, ub, np.full(5, -1e30), P, combine)
        assert ok[:, images].all()


def _request(**kw):
    tb = search.TokenBank.__new__(search.TokenBank)               # no device: the decision reads the flag only
    tb._resident = True
    base = dict(who="cosine_topk_tokens", Q=64, N=4096, P=16, D=128, k=10, combine=ops.COMBINE_CODES["min"], metric=None,
                metric_name=None, top_t=0, per_query=False, step=16, idx_offset=0, tokens=None, bank=tb, weights=None, select=None)
    base.update(kw)
    return search.TokenRequest(**base)


def test_route_decision(monkeypatch):
    """Every listed condition sends the request to the grouped route, and nothing else does."""
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 17)
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    refusal = search._token_prefilter_refusal
    assert refusal(_request()) is None
    for P in (1, 2, 4, 8, 16, 32, 64):
        assert refusal(_request(P=P, N=4096 * 16 // P)) is None
    assert refusal(_request(combine=ops.COMBINE_CODES["max"], Q=17, k=256, D=4096, idx_offset=5)) is None
    plain = search.TokenBank.__new__(search.TokenBank)
    plain._resident = False
    grouped = dict(bank=[plain, None], combine=[ops.COMBINE_CODES["mean"]], top_t=[1, 4], select=[object()], per_query=[True],
                   P=[3, 48, 128], Q=[16, 1], metric=[ops.METRIC_CODES["MSE"]], D=[96, 144, 4128], k=[257], N=[127, 9])
    for field, values in grouped.items():
        for v in values:
            why = refusal(_request(**{field: v}))
            assert isinstance(why, str) and why, (field, v)
    assert "N * P" in refusal(_request(N=127)) and "2^31" in refusal(_request(N=2 ** 27))      # the library's own text
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    assert "SKYEMB_TOPK_PREFILTER" in refusal(_request())
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "1")
    assert refusal(_request()) is None
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 65)
    assert "TOKEN_PREFILTER_MIN_Q" in refusal(_request())
    assert dataclasses.is_dataclass(search.TokenRequest)


def test_resident_refuses_what_it_cannot_read():
    with pytest.raises(ValueError, match="torch.float16 or torch.bfloat16"):
        search.TokenBank.resident(torch.zeros(8, 4, 128))
    with pytest.raises(ValueError, match="torch.float16 or torch.bfloat16"):
        search.TokenBank.resident(np.zeros((8, 4, 128), np.float16))
    with pytest.raises(ValueError, match=r"contiguous \[N, P, D\]"):
        search.TokenBank.resident(torch.zeros(32, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match=r"contiguous \[N, P, D\]"):
        search.TokenBank.resident(torch.zeros(8, 4, 256, dtype=torch.bfloat16)[:, :, ::2])
    flat = torch.zeros(8 * 4 * 128 + 8, dtype=torch.float16)
    odd = flat[1:1 + 8 * 4 * 128].view(8, 4, 128)
    assert odd.data_ptr() % 16 and odd.is_contiguous()
    with pytest.raises(ValueError, match="16-byte aligned"):
        search.TokenBank.resident(odd)


def test_new_symbols_are_exported_with_the_declared_signatures():
    """skyemb_token_prefilter_applicable, skyemb_token_prefilter_ws_bytes and skyemb_cosine_topk_tokens_prefiltered: declared in
    the header, exported by the library, bound with the header's parameter kinds; the predicate states its limits as its error."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skyemb.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.build())
    for name in ("skyemb_token_prefilter_applicable", "skyemb_token_prefilter_ws_bytes", "skyemb_cosine_topk_tokens_prefiltered"):
        m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/skyemb.h"
        assert hasattr(L, name), f"{name} is not exported"
        res, args = _lib.PROTOTYPES[name]
        assert res is (ctypes.c_int64 if m.group(1) == "int64_t" else ctypes.c_int32)
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args), (name, len(params), len(args))
        for p, a in zip(params, args):
            want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float") else
                    ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int32)
            assert a is want, (name, p, a)
    lib = _lib.lib()
    assert lib.skyemb_token_prefilter_applicable(17, 512, 4, 128, 100) == 1
    assert lib.skyemb_token_prefilter_applicable(17, 511, 4, 128, 100) == 0
    msg = lib.skyemb_last_error().decode()
    assert "divisor of 64" in msg and "N=511" in msg and "P=4" in msg
    for Q, N, P, D, k in ((17, 512, 3, 128, 1), (17, 512, 4, 96, 1), (17, 512, 4, 4128, 1), (17, 512, 4, 128, 257), (17, 40, 64, 128, 41),
                          (17, 2 ** 29, 4, 128, 1), (0, 512, 4, 128, 1)):
        assert lib.skyemb_token_prefilter_applicable(Q, N, P, D, k) == 0, (Q, N, P, D, k)
    assert lib.skyemb_token_prefilter_ws_bytes(130, 128, 100) > lib.skyemb_topk_prefilter_ws_bytes(130, 128, 100)
    rc = lib.skyemb_cosine_topk_tokens_prefiltered(None, None, 17, None, _lib.F16, None, None, None, 512, 4, 128, 1, 0, 1e-6, 0, None, None, 0,
                                                   None, None, None, None)
    assert rc != 0 and b"null argument" in lib.skyemb_last_error()
