"""CPU: the two-stage weighted-MSE token search with per-query weights -- the route decision and every refusal text, the answers
without the opt-in (today's strings), eps_pq against the library, the new symbols, and the soundness of the bound
(tests/token_mse_pq_reference.py restates its constants): under three models of stage 1's dot products no pair whose fp64 distance
is within the query's true k-th best fails the row test."""
import os
import re

import numpy as np
import pytest
import torch

from sky_embeddings_amd import _lib, ops, search
from tests import token_mse_pq_reference as pqr
from tests import token_mse_prefilter_reference as mpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN, MEAN, MAX = (ops.COMBINE_CODES[c] for c in ("min", "mean", "max"))
NEW = ("skyemb_token_mse_pq_prefilter_applicable", "skyemb_token_mse_pq_prefilter_eps", "skyemb_token_mse_pq_image",
       "skyemb_distance_topk_tokens_prefiltered_pq")


def _bank(prepared=False, top_t=False):
    tb = search.TokenBank.__new__(search.TokenBank)               # no device: the decision reads the flags only
    tb._resident, tb.dtype, tb._mse_pq = True, torch.float16, (None, None) if prepared else None
    if top_t:
        tb.prepare_mse_top_t()
    return tb


def _request(**kw):
    base = dict(who="distance_topk_tokens", Q=2048, N=4096, P=16, D=128, k=10, combine=MIN, metric=ops.METRIC_CODES["MSE"],
                metric_name="MSE", top_t=0, per_query=True, step=16, idx_offset=0, tokens=None, bank=_bank(True), weights=None, select=None)
    base.update(kw)
    return search.TokenRequest(**base)


def test_route_decision_and_refusal_texts(monkeypatch):
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    refusal = search._token_prefilter_refusal
    assert search.TOKEN_MSE_PQ_PREFILTER_MIN_Q in (16, 32, 64, 128, 256, 1024)        # a point of the tool's grid (1024: the fallback)
    # not prepared: the pinned words, unchanged; a bank built without the attribute too
    assert refusal(_request(bank=_bank())) == "per-query weights"
    bare = search.TokenBank.__new__(search.TokenBank)
    bare._resident, bare.dtype = True, torch.float16
    assert refusal(_request(bank=bare)) == "per-query weights"
    # prepared
    for combine in (MIN, MAX):
        assert refusal(_request(combine=combine)) is None
    for P in (1, 2, 4, 8, 16, 32, 64):
        assert refusal(_request(P=P, N=4096 * 16 // P)) is None
    assert refusal(_request(per_query=False)) is None               # shared weights over a prepared bank: the plain route, as ever
    # prepared plus top_t or select: their existing reasons, never combined with per-query weights
    assert refusal(_request(top_t=2)) == "top_t under a distance metric"
    assert refusal(_request(select=object())) == "select under a distance metric"
    assert refusal(_request(bank=_bank(True, top_t=True), top_t=2)) == "per-query weights"
    # prepared plus MAE or 'mean'
    assert "MAE" in refusal(_request(metric=ops.METRIC_CODES["MAE"], metric_name="MAE"))
    assert refusal(_request(combine=MEAN)) == "combine 'mean' under a distance metric"
    assert refusal(_request(P=48)) == "P = 48 does not divide 64"
    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    assert refusal(_request()) == "SKYEMB_TOPK_PREFILTER=0"
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER")
    # the library's own text: D = 2080 (rows of 2 D = 4160 > 4096), D = 144, too few rows, k
    for kw in (dict(D=2080), dict(D=144), dict(D=96), dict(N=127), dict(k=257)):
        why = refusal(_request(**kw))
        assert why == ops.token_mse_pq_prefilter_refusal(*(_request(**kw).__dict__[f] for f in ("Q", "N", "P", "D", "k")))
        assert why.startswith("many-query weighted-MSE patch-token search with per-query weights"), why
    assert "128 <= D <= 2048" in refusal(_request(D=2080)) and refusal(_request(D=2048)) is None
    # Q below the constant: on a bank of the measured size its own name, on a smaller one the shared small-bank constant
    big, small = dict(N=15625, P=64, D=768), search.TOKEN_MSE_PREFILTER_MIN_Q_SMALL
    monkeypatch.setattr(search, "TOKEN_MSE_PQ_PREFILTER_MIN_Q", 128)
    assert refusal(_request(Q=127, **big)) == "Q = 127 < TOKEN_MSE_PQ_PREFILTER_MIN_Q = 128"
    assert refusal(_request(Q=128, **big)) is None
    assert refusal(_request(Q=small - 1)).startswith(f"Q = {small - 1} < TOKEN_MSE_PREFILTER_MIN_Q_SMALL = {small}")
    assert refusal(_request(Q=small)) is None
    # the same decision from plain facts
    plain = search.token_mse_route_refusal
    assert plain(small, 4096, 16, 128, 10, "MSE", "min", per_query=True, per_query_prepared=True) is None
    assert plain(small, 4096, 16, 128, 10, "MSE", "min", per_query=True) == "per-query weights"
    assert plain(small, 4096, 16, 128, 10, "MSE", "max", 2, per_query=True, per_query_prepared=True, top_t_prepared=True) == "per-query weights"
    assert plain(small, 4096, 16, 128, 10, "MSE", "max", None, True, True, per_query_prepared=True, select_prepared=True) == "per-query weights"


def test_without_the_opt_in_every_answer_is_what_it_was(monkeypatch):
    """``per_query_prepared=False`` (the default): the cases of tests/test_token_mse_select_topt_cpu.py, answer for answer."""
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER", raising=False)
    plain = search.token_mse_route_refusal
    small = search.TOKEN_MSE_PREFILTER_MIN_Q_SMALL
    kw = dict(top_t_prepared=True, select_prepared=True)
    cases = [((2048, 4096, 16, 128, 10, "MSE", "max"), dict(top_t=2), "top_t under a distance metric"),
             ((2048, 4096, 16, 128, 10, "MSE", "max"), dict(select=True), "select under a distance metric"),
             ((2048, 4096, 16, 128, 10, "MSE", "max", 2, True), {}, "top_t under a distance metric"),
             ((2048, 4096, 16, 128, 10, "MSE", "max"), {}, None),
             ((small, 4096, 16, 128, 10, "MSE", "max", 2), kw, None),
             ((small, 4096, 16, 128, 10, "MSE", "max", 2, True), dict(selected=2000, **kw), None),
             ((small, 4096, 16, 128, 10, "MSE", "max", 2, True), dict(top_t_prepared=True), "select under a distance metric"),
             ((small, 4096, 16, 128, 10, "MSE", "max", 2, True), dict(select_prepared=True), "top_t under a distance metric"),
             ((small, 4096, 16, 128, 10, "MSE", "mean", 2), kw, "combine 'mean' under a distance metric"),
             ((17, 4096, 16, 128, 10, "MSE", "min", None, False, True), {}, "per-query weights"),
             ((small, 4096, 16, 128, 10, "MSE", "max", 2, False, True), kw, "per-query weights")]
    for args, kws, want in cases:
        assert plain(*args, **kws) == want == plain(*args, per_query_prepared=False, **kws), (args, kws)
    got = plain(small, 4096, 16, 128, 10, "MSE", "max", None, True, selected=100, **kw)
    assert got.startswith("the selected images alone: ") and got == plain(small, 4096, 16, 128, 10, "MSE", "max", None, True, selected=100,
                                                                          per_query_prepared=False, **kw)
    # the opt-in changes nothing for a request without per-query weights
    for args, kws, want in cases:
        if not (len(args) > 9 and args[9]):
            assert plain(*args, per_query_prepared=True, **kws) == want, (args, kws)


def test_the_way_in_checks_its_bank():
    tb = search.TokenBank.__new__(search.TokenBank)
    tb._resident, tb._mse_pq = False, None
    with pytest.raises(ValueError, match="TokenBank.resident"):
        tb.prepare_mse_per_query()
    assert tb._mse_pq is None


def test_eps_pq_follows_the_library():
    for D in (128, 160, 768, 2048):
        for lo in (False, True):
            for dt, tdt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
                assert pqr.eps_pq(D, lo, dt) == ops.token_mse_pq_prefilter_eps(D, tdt, lo), (D, lo, dt)
                rho = pqr.RHO[dt]
                base = ops.topk_prefilter_eps_a_resident(2 * D, tdt, lo) + rho * (1.0 + rho) + 2.0 ** -22
                assert pqr.eps_pq(D, lo, dt) == (base + pqr.kappa(lo, dt) if dt == "bf16" else base)
    assert pqr.kappa(False, "f16") == pqr.kappa(True, "f16") == 0.0


def _mantissas(dt):
    """Every number of the format in [1, 2), as fp32."""
    bits = 10 if dt == "f16" else 7
    return (1.0 + np.arange(2 ** bits) * 2.0 ** -bits).astype(np.float32)


def test_rho_is_the_unit_roundoff_of_the_format_itself():
    """One round-to-nearest-even of the format (NumPy's fp16; the bit rule of bf16), measured on every square of a number of
    [1, 2): never above rho 2^e, and attained to within 2 % -- so no smaller constant bounds the squares' rounding."""
    for dt in ("f16", "bf16"):
        m = _mantissas(dt)
        v = (m.astype(np.float64) ** 2)
        stored = mpr.to16((m * m).astype(np.float32), dt).astype(np.float64)
        assert ((m * m).astype(np.float64) == v).all()                              # the fp32 square is exact
        rel = np.abs(stored - v) / np.exp2(np.floor(np.log2(v)))
        assert rel.max() <= pqr.RHO[dt] and rel.max() >= 0.98 * pqr.RHO[dt], (dt, rel.max())
        assert (np.abs(stored - v) <= pqr.RHO[dt] * np.minimum(v, stored)).all()
        # the query split: a number halfway between two neighbours moves by the whole unit roundoff
        half = np.float32(1.0 + pqr.RHO[dt])
        assert abs(float(mpr.to16(np.array([half]), dt)[0]) - float(half)) == pqr.RHO[dt]
    assert float(mpr.to16(np.array([95.5 * 95.5], np.float32), "bf16")[0]) == 9152.0


def test_new_symbols_are_exported_and_the_version_stands():
    header = open(os.path.join(ROOT, "include", "skyemb.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.PROTOTYPES and hasattr(L, n), n
    assert L.skyemb_version() == _lib.ABI_VERSION
    assert ops.token_mse_pq_prefilter_refusal(17, 1037, 4, 160, 100) is None
    assert ops.token_mse_pq_prefilter_refusal(17, 1024, 16, 2048, 1) is None
    assert "128 <= D <= 2048" in ops.token_mse_pq_prefilter_refusal(17, 1024, 16, 2080, 1)
    assert "Q=17 N=100 P=4 D=128 k=1" in ops.token_mse_pq_prefilter_refusal(17, 100, 4, 128, 1)
    # the bad calls are refused before any device work
    f16 = ops.resident_dtype_code(torch.float16, "test")
    assert L.skyemb_token_mse_pq_image(None, f16, 10, 128, None, None, None) != 0
    assert b"skyemb_token_mse_pq_image" in L.skyemb_last_error()
    assert L.skyemb_distance_topk_tokens_prefiltered_pq(None, None, 17, None, f16, None, None, 1024, 16, 128, 1, MIN, 0, None, None, 0, None,
                                                        None, None, None) != 0
    assert b"skyemb_distance_topk_tokens_prefiltered_pq" in L.skyemb_last_error()


# ---- soundness of the bound ----------------------------------------------------------------------------------------------------------
def _sound_bank(D, dt, seed):
    """2048 widened 16-bit rows: standardised rows of very different scale; rows with all |x| < 2^-7 (fp16: every square is rounded
    on the subnormal grid, or to zero); rows of fp16 subnormals; rows with elements just below 2^8 (fp16: squares next to 65504);
    a zero row; rows next to the queries."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((2048, D)) * rng.uniform(0.05, 8.0, (2048, 1))).astype(np.float32)
    x[100:140] = (rng.standard_normal((40, D)) * 2.0 ** -9).astype(np.float32).clip(-2.0 ** -7.01, 2.0 ** -7.01)
    x[140:160] = 2.0 ** -20 * rng.integers(-15, 16, (20, D))
    x[160:180] = rng.uniform(-1, 1, (20, D)) * 2.0 ** -12.4         # squares around 2^-25: to zero or to the smallest subnormal
    x[180:200, ::3] = np.sign(rng.standard_normal((20, (D + 2) // 3))) * rng.uniform(250.0, 255.9, (20, (D + 2) // 3))
    x[200] = 0.0
    x[201] = 255.875                                                  # the largest fp16 below 2^8 in every element
    return mpr.to16(x, dt)


def _sound_queries(x, D, seed):
    rng = np.random.default_rng(seed)
    Q = 24
    t = rng.standard_normal((Q, D)).astype(np.float32)
    t[0:4] = x[[100, 141, 161, 181]]                                  # queries that ARE hostile rows
    t[4:8] = x[300:304] + 1e-2 * rng.standard_normal((4, D)).astype(np.float32)
    t[8] *= 2.0 ** -8
    t[9] *= 40.0
    w = (rng.random((Q, D)) + 0.05).astype(np.float32)
    w[10] = 1.0
    w[11, rng.random(D) < 0.5] = 0.0
    w[12] = 1e-6
    w[12, D // 3] = 1.0                                               # one dominant feature
    w[13] *= 2.0 ** -20                                               # (normalised away by c = w / sum w)
    c = np.stack([(r / r.sum(dtype=np.float32)).astype(np.float32) for r in w])
    c[14] = c[14] * np.float32(2.0 ** 9 * D / 4)                      # un-normalised rows: weights up to ~2^9 ...
    c[15] = c[15] * np.float32(2.0 ** -20)                            # ... and down to 2^-20 x
    return c, t


def _flush(a, dt):
    lim = 2.0 ** -14 if dt == "f16" else 2.0 ** -126
    return np.where(np.abs(a) < lim, 0.0, a)


@pytest.mark.parametrize("D", [128, 160])
@pytest.mark.parametrize("lo", [False, True], ids=["hi", "hilo"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_no_pair_within_the_kth_best_fails_the_row_test(dt, lo, D):
    x = _sound_bank(D, dt, 7 * D + (dt == "bf16"))
    c, t = _sound_queries(x, D, D + 1)
    y, ub = pqr.image(x, dt)
    ny, _ = pqr.row_constants(x, dt)
    qc = pqr.query_constants(c, t, dt, lo)
    assert not ub.any() and not qc["flagged"].any()                  # everything here is inside what the route bounds
    if dt == "f16":
        sq = y[:, D:]
        assert (sq[100:140] < 2.0 ** -14).all() and (sq[160:180] <= 2.0 ** -24).all() and sq[180:200].max() > 62000.0
        assert sq[201, 0] == 65472.0
    x64, c64, t64 = x.astype(np.float64), c.astype(np.float64), t.astype(np.float64)
    dist64 = np.stack([(c64[q] * (x64 - t64[q]) ** 2).sum(axis=1) / D for q in range(len(t))])
    dist32 = pqr.contract_distances(c, t, x)
    y64 = y.astype(np.float64)
    ops16 = [qc["qh"].astype(np.float64)] + ([qc["ql"].astype(np.float64)] if lo else [])
    stored = sum(o @ y64.T for o in ops16)
    flushed = sum(_flush(o, dt) @ _flush(y64, dt).T for o in ops16)
    absum = sum(np.abs(o) @ np.abs(y64).T for o in ops16)
    n_prod = 2 * D * len(ops16)
    models = {"stored": stored.astype(np.float32).astype(np.float64), "flushed": flushed.astype(np.float32).astype(np.float64),
              "one ulp per product, downwards": stored - n_prod * 2.0 ** -23 * absum}
    for k in (1, 100):
        # the true k-th best, in fp64 and as the contract rounds it (the threshold the kernel holds is a contract value)
        for name, d, theta in (("fp64", dist64, np.sort(dist64, axis=1)[:, k - 1]), ("contract", dist32, np.sort(dist32, axis=1)[:, k - 1])):
            within = d <= theta[:, None]
            assert within.sum() >= k * len(t)
            th = theta.astype(np.float32).astype(np.float64)
            th = np.where(th < theta, np.nextafter(th.astype(np.float32), np.float32(np.inf)).astype(np.float64), th)   # fp32, not below
            for model, dot in models.items():
                ok = pqr.row_test(dot, qc, ny, D, th)
                miss = within & ~ok
                assert not miss.any(), (name, model, k, np.argwhere(miss)[:4])
    # ... and the bound is worth something: under unit weights (query 10) the test at the k = 100 threshold keeps a minority of the rows
    th = np.sort(dist32, axis=1)[:, 99].astype(np.float64)
    kept = pqr.row_test(models["stored"], qc, ny, D, th)[10].mean()
    assert kept < 0.5, kept


def _adversarial(D, dt):
    """Rows of EQUAL elements whose squares round by nearly half an ulp of the format, all in one direction -- the element is found
    by measuring every number of [1, 2), not taken from the restatement --, so that Cauchy-Schwarz over the second half is tight;
    uniform c = 1 / D (a power of two at D = 128: c o t and -c / 2 are exact); queries with |t| << |x| (the squares' half carries the
    distance), and queries whose scaled elements all lie halfway between two neighbours of the format (the split's worst case)."""
    m = _mantissas(dt)
    v = m.astype(np.float64) ** 2
    err = (mpr.to16((m * m).astype(np.float32), dt).astype(np.float64) - v) / np.exp2(np.floor(np.log2(v)))
    up, down = m[np.argsort(err)[-3:]], m[np.argsort(err)[:3]]
    scales = np.exp2(np.array([-3.0, 0.0, 2.0, 6.0], np.float32))
    x = np.concatenate([np.full((1, D), e * s, np.float32) for e in np.concatenate([up, down, -up]) for s in scales])
    if dt == "bf16":
        x = np.concatenate([x, np.full((1, D), 95.5, np.float32)])                # the reviewer's own row
    assert np.array_equal(mpr.to16(x, dt), x)
    rng = np.random.default_rng(D)
    half = np.float32(1.0 + (2.0 ** -11 if dt == "f16" else 2.0 ** -8))           # halfway between 1 and its upper neighbour
    t = np.concatenate([1e-3 * rng.standard_normal((4, D)), np.full((1, D), 2.0 ** -6), np.full((1, D), 0.0) + 2.0 ** -20,
                        np.full((4, D), half) * np.exp2(np.arange(4.0) * 3 - 2)[:, None],
                        -np.full((2, D), half) * np.array([[1.0], [64.0]])]).astype(np.float32)
    c = np.full((len(t), D), 1.0 / D, np.float32)
    return c, t, x


@pytest.mark.parametrize("D", [128, 160])
@pytest.mark.parametrize("lo", [False, True], ids=["hi", "hilo"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_adversarial_rows_pass_the_row_test_at_their_own_distance(dt, lo, D):
    """Every (query, row) pair must pass under the threshold that is the pair's OWN distance -- in fp64 and as the contract rounds it
    --, which is what a row that is the query's true k-th best meets; under the three models of stage 1."""
    c, t, x = _adversarial(D, dt)
    y, ub = pqr.image(x, dt)
    ny, _ = pqr.row_constants(x, dt)
    qc = pqr.query_constants(c, t, dt, lo)
    assert not ub.any() and not qc["flagged"].any()
    sq_err = np.abs(y[:, D:].astype(np.float64) - x.astype(np.float64) ** 2) / (x.astype(np.float64) ** 2)
    assert sq_err.max() > 0.8 * 2.0 ** (-11 if dt == "f16" else -8)                # nearly half an ulp just above a power of two
    x64, c64, t64 = x.astype(np.float64), c.astype(np.float64), t.astype(np.float64)
    dist64 = np.stack([(c64[q] * (x64 - t64[q]) ** 2).sum(axis=1) / D for q in range(len(t))])
    dist32 = pqr.contract_distances(c, t, x)
    y64 = y.astype(np.float64)
    ops16 = [qc["qh"].astype(np.float64)] + ([qc["ql"].astype(np.float64)] if lo else [])
    stored = sum(o @ y64.T for o in ops16)
    flushed = sum(_flush(o, dt) @ _flush(y64, dt).T for o in ops16)
    absum = sum(np.abs(o) @ np.abs(y64).T for o in ops16)
    models = {"exact": stored, "stored": stored.astype(np.float32).astype(np.float64),
              "flushed": flushed.astype(np.float32).astype(np.float64),
              "one ulp per product, downwards": stored - 2 * D * len(ops16) * 2.0 ** -23 * absum}
    # the figure the bound is about, under exact accumulation: never above eps_pq, and the construction comes close to it
    real = (qc["u"].astype(np.float64) * qc["s"][:, None]) @ np.concatenate([x64, x64 ** 2], axis=1).T
    nq = np.sqrt(((qc["u"].astype(np.float64) * qc["s"][:, None]) ** 2).sum(axis=1))
    ratio = np.abs(stored - real) / (nq[:, None] * ny[None, :])
    print(dt, lo, D, "largest |dot^ - real| / (||u'|| ny):", ratio.max(), "eps_pq:", pqr.eps_pq(D, lo, dt))
    assert ratio.max() <= pqr.eps_pq(D, lo, dt)
    if dt == "bf16":
        assert ratio.max() > 0.003                                                 # above what rho = 2^-9 could have covered under hi + lo
    for name, d in (("fp64", dist64), ("contract", dist32)):
        for model, dot in models.items():
            for q in range(len(t)):
                th = d[q].astype(np.float64)
                ok = np.array([pqr.row_test(dot[q:q + 1, r:r + 1], {k: v[q:q + 1] for k, v in qc.items()}, ny[r:r + 1], D, th[r:r + 1])[0, 0]
                               for r in range(len(x))])
                assert ok.all(), (name, model, q, np.argwhere(~ok)[:4].ravel())


def test_rows_and_queries_the_bound_gives_up_on():
    D = 128
    rng = np.random.default_rng(5)
    x = rng.standard_normal((8, D)).astype(np.float32)
    x[1, 5] = np.inf
    x[2, 7] = np.nan
    x[3, 9] = 300.0                                                # fp16: the square leaves the format; bf16: fine
    x[4, 11] = 1e-20                                               # bf16: the square is below 2^-60; fp16: rounds to zero
    x[5, 3] = 2.0 ** 60                                            # bf16: the square reaches 2^120; fp16: inf
    x[6, 2] = 256.0
    for dt, want in (("f16", [0, 1, 1, 1, 0, 1, 1, 0]), ("bf16", [0, 1, 1, 0, 1, 1, 0, 0])):
        xs = mpr.to16(x, dt)
        y, ub = pqr.image(xs, dt)
        assert ub.tolist() == [bool(v) for v in want], (dt, ub)
        assert (y[ub] == 0).all() and np.isinf(pqr.row_constants(xs, dt)[0][ub]).all()
    t = rng.standard_normal((6, D)).astype(np.float32)
    c = np.full((6, D), 1.0 / D, np.float32)
    t[1] = 0.0                                                     # c o t = 0
    c[2, 17] = -1e-3
    c[3, 17] = np.nan
    c[4, 17] = 2048.0
    for dt in ("f16", "bf16"):
        assert pqr.query_constants(c, t, dt, True)["flagged"].tolist() == [False, True, True, True, True, False], dt
