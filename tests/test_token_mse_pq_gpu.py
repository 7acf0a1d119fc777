"""GPU: the two-stage many-query weighted-MSE search with per-query weights --
``distance_topk_tokens(q, TokenBank.resident(bank).prepare_mse_per_query(), k, 'MSE', combine, weights=W[Q, D])``.

The reference of every case is the same call over the same device bank in a ``TokenBank.resident`` never asked (the grouped
per-query route); distances and indices must be bit-equal.  D = 160 is a shape the grouped kernels do not take (they need
D % 64 == 0), so there the library call is compared with the NumPy restatement of the contract
(tests/token_mse_pq_reference.contract_distances)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import prefilter_gpu_harness as H
from tests import token_distance_reference as tdr
from tests import token_mse_pq_reference as pqr
from tests import token_mse_prefilter_reference as mpr

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(autouse=True)
def _min_q(monkeypatch):
    from sky_embeddings_amd import search
    monkeypatch.setattr(search, "TOKEN_MSE_PQ_PREFILTER_MIN_Q", 17)
    monkeypatch.setattr(search, "TOKEN_MSE_PREFILTER_MIN_Q_SMALL", 17)


def _to16(x, dt):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DTYPES[dt])
    return t, t.float().numpy()


def _bank(rng, N, P, D, dt):
    """Images of very different scale whose tokens share a direction, as a 16-bit tensor and the fp32 array it widens to."""
    x = (rng.standard_normal((N, 1, D)) * rng.uniform(0.3, 2.0, (N, 1, 1)) + 0.7 * rng.standard_normal((N, P, D))).astype(np.float32)
    return _to16(x, dt)


def _weights(rng, Q, D):
    """One row per query, rows scaled by 2^-20 .. 2^9 across the queries and elements spread over 2^-10 .. 1 inside a row.  Through
    ``distance_topk_tokens`` the row scale is normalised away (c = w / sum w): there only the spread inside a row reaches the kernels.
    The cases that call ``ops`` directly (D = 160, and ``test_unnormalised_weight_rows_d128``) hand c over as it is, rows between
    2^-20 and 2^9 x."""
    w = (rng.random((Q, D)).astype(np.float32) + 0.05) * np.exp2(-10.0 * rng.random((Q, D))).astype(np.float32)
    return (w * np.exp2(rng.integers(-20, 10, (Q, 1))).astype(np.float32)).astype(np.float32)


def _both(q, bank, w, k, combine, idx_offset=0, prepared=None):
    """((distances, indices, stats) of the prepared bank, the same of a resident bank never asked); bank: a 16-bit tensor."""
    from sky_embeddings_amd import search
    qd, xd, wd = torch.from_numpy(q).cuda(), bank.cuda(), torch.from_numpy(w).cuda()
    asked = search.TokenBank.resident(xd, None, idx_offset).prepare_mse_per_query() if prepared is None else prepared
    out = []
    for tb in (asked, search.TokenBank.resident(xd, None, idx_offset)):
        stats = {}
        s, i = search.distance_topk_tokens(qd, tb, k, "MSE", combine, weights=wd, stats=stats)
        out.append((s, i, stats))
    return out


def _assert_same(got, ref):
    assert torch.equal(got[1], ref[1]), (got[2], torch.nonzero(got[1] != ref[1])[:5].tolist())
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)), got[2]


# bank (1024, 16): 16384 rows in whole tiles; bank (256, 64): P = 64.  Q = 130: two 128-query tiles under hi + lo, one partial;
# Q = 17.  k in {1, 100}; both dtypes, combines and variants.
CASES = [
    (1024, 16, "f16", "min", 0, 130, 100, 0), (1024, 16, "bf16", "max", 1, 130, 1, 7), (1024, 16, "f16", "max", 1, 17, 100, 0),
    (1024, 16, "bf16", "min", 0, 17, 1, 0), (256, 64, "f16", "min", 1, 130, 100, 1000), (256, 64, "bf16", "max", 0, 17, 1, 0),
    (256, 64, "f16", "max", 0, 130, 1, 0), (256, 64, "bf16", "min", 1, 17, 100, 3),
]


@pytest.mark.parametrize("c", CASES, ids=lambda c: "N%d-P%d-%s-%s-lo%d-Q%d-k%d-off%d" % c)
def test_two_stage_per_query_topk_is_bit_exact(c, monkeypatch):
    N, P, dt, combine, lo, Q, k, off = c
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", str(lo))
    rng = np.random.default_rng(N + P + Q + k)
    D = 128
    bank, xw = _bank(rng, N, P, D, dt)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    q[3] = xw[N // 2, P - 1]                                       # a query that is itself a bank row
    got, ref = _both(q, bank, _weights(rng, Q, D), k, combine, off)
    print(got[2])
    _assert_same(got, ref)
    assert ref[2]["path"] == "tokens" and ref[2]["per_query_weights"] is True
    assert got[2]["path"] == "prefiltered" and got[2]["per_query_weights"] is True, got[2]
    assert got[2]["combine"] == combine and got[2]["metric"] == "MSE" and got[2]["redone"] == 0, got[2]
    if combine == "min":
        assert got[1][3, 0].item() == off + N // 2 and got[0][3, 0].item() == 0.0


@pytest.mark.parametrize("dt,combine,lo,k", [("f16", "min", 1, 100), ("bf16", "max", 0, 1), ("f16", "max", 0, 1), ("bf16", "min", 1, 100)])
def test_ragged_d160_against_the_contract(dt, combine, lo, k, monkeypatch):
    """bank (1037, 4, 160): 4148 rows, 52 past the last whole tile, ten 32-element k-steps in stage 1: the library call against
    NumPy, with un-normalised weight rows between 2^-20 and 2^9."""
    from sky_embeddings_amd import ops
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", str(lo))
    rng = np.random.default_rng(160 + k)
    N, P, D, Q, off = 1037, 4, 160, 17, 11
    bank, xw = _bank(rng, N, P, D, dt)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    q[2] = xw[N - 1, P - 1]                                        # the bank's last row, in the ragged tile
    c = (_weights(rng, Q, D) / np.float32(D)).astype(np.float32)
    c = np.minimum(c, np.float32(2.0 ** 9))
    xd, qd, cd = bank.cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    image, rowp = ops.token_mse_pq_image(xd)
    assert image.shape == (4352, 2 * D) and rowp.shape == (4352, 4)
    out_s, out_i = torch.empty(Q, k, device="cuda"), torch.empty(Q, k, device="cuda", dtype=torch.int64)
    redo = torch.empty(Q, device="cuda", dtype=torch.int32)
    ops.distance_topk_tokens_prefiltered_pq(cd, qd, xd, image, rowp, k, ops.COMBINE_CODES[combine], off, out_s, out_i, redo)
    assert int(redo.sum()) == 0
    a = pqr.contract_distances(c, q, xw.reshape(N * P, D)).reshape(Q, N, P)
    rs, ri = tdr.topk_of_token_distances(a, k, combine, idx_offset=off)
    assert np.array_equal(out_i.cpu().numpy(), ri)
    assert np.array_equal((-out_s).cpu().numpy().view(np.uint32), rs.view(np.uint32))
    if combine == "min":
        assert ri[2, 0] == off + N - 1


def _direct(ops, cd, qd, xd, k, combine, off, image=None, rowp=None, ws=None):
    """The library call itself: -> (keys, images, redo, ws)."""
    Q = qd.shape[0]
    if image is None:
        image, rowp = ops.token_mse_pq_image(xd)
    out_s, out_i = torch.empty(Q, k, device="cuda"), torch.empty(Q, k, device="cuda", dtype=torch.int64)
    redo = torch.empty(Q, device="cuda", dtype=torch.int32)
    ws = ops.distance_topk_tokens_prefiltered_pq(cd, qd, xd, image, rowp, k, ops.COMBINE_CODES[combine], off, out_s, out_i, redo, None, ws)
    return out_s, out_i, redo, ws


@pytest.mark.parametrize("dt,combine,lo", [("f16", "min", 0), ("bf16", "max", 1)])
def test_unnormalised_weight_rows_d128(dt, combine, lo, monkeypatch):
    """c handed over as it is, rows between 2^-20 and 2^9 x across the queries: the library call against the grouped per-query
    kernel (skyemb_distance_token_topk_pq + the merge) on the same c, bit for bit."""
    from sky_embeddings_amd import ops
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", str(lo))
    rng = np.random.default_rng(128 + lo)
    N, P, D, Q, k, off = 1024, 4, 128, 16, 100, 5
    bank, xw = _bank(rng, N, P, D, dt)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    c = np.minimum(_weights(rng, Q, D) / np.float32(D), np.float32(2.0 ** 9)).astype(np.float32)
    c[0] *= np.float32(2.0 ** 9 / c[0].max())                      # one row reaches 2^9 itself, one stays near 2^-30
    c[1] *= np.float32(2.0 ** -20)
    xd, qd, cd = bank.cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    out_s, out_i, redo, _ = _direct(ops, cd, qd, xd, k, combine, off)
    assert int(redo.sum()) == 0
    nl = ops.cosine_token_topk_chunks(N, P, Q, D, k)
    ps, pi = torch.empty(Q, nl, k, device="cuda"), torch.empty(Q, nl, k, device="cuda", dtype=torch.int64)
    ops.distance_token_topk_pq(cd, qd, xd, ops.METRIC_CODES["MSE"], ops.COMBINE_CODES[combine], k, off, nl, ps, pi, None, 0, None)
    ref_s, ref_i = torch.empty(Q, k, device="cuda"), torch.empty(Q, k, device="cuda", dtype=torch.int64)
    ops.topk_merge(ps, pi, Q, nl, k, ref_s, ref_i, torch.empty(Q, device="cuda", dtype=torch.int32))
    assert torch.equal(out_i, ref_i) and torch.equal(out_s.view(torch.int32), ref_s.view(torch.int32))


def _worst_mantissas(dt, n):
    """The n numbers of [1, 2) of the format whose squares round UP by the most, measured on the format itself."""
    bits = 10 if dt == "f16" else 7
    m = (1.0 + np.arange(2 ** bits) * 2.0 ** -bits).astype(np.float32)
    v = m.astype(np.float64) ** 2
    err = (mpr.to16((m * m).astype(np.float32), dt).astype(np.float64) - v) / np.exp2(np.floor(np.log2(v)))
    return m[np.argsort(err)[-n:]]


@pytest.mark.parametrize("dt,lo,combine", [("bf16", 1, "min"), ("bf16", 0, "max"), ("f16", 1, "min"), ("f16", 0, "min")])
def test_rows_of_equal_elements_with_half_ulp_squares(dt, lo, combine, monkeypatch):
    """A bank made ONLY of rows of equal elements whose squares round up by nearly half an ulp of the format (Cauchy-Schwarz over
    the squares' half is tight), uniform c, queries with |t| << |x| and queries whose scaled elements lie halfway between two
    neighbours of the format: the k-th best of every query is such a row, so a bound that is too narrow drops it.  Against NumPy."""
    from sky_embeddings_amd import ops
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", str(lo))
    rng = np.random.default_rng(95)
    P, D, off = 4, 128, 0
    ms = _worst_mantissas(dt, 64)
    vals = np.concatenate([ms * s for s in np.exp2(np.arange(-3.0, 5.0)).astype(np.float32)])        # 512 images, |x| < 32
    if dt == "bf16":
        vals[7] = 95.5
    N = len(vals)
    x = np.repeat(vals[rng.permutation(N)], P * D).reshape(N, P, D).astype(np.float32)
    x[:, 2] *= -1.0                                                # one token of every image on the other side
    bank, xw = _to16(x, dt)
    assert np.array_equal(xw, x)
    half = np.float32(1.0 + (2.0 ** -11 if dt == "f16" else 2.0 ** -8))
    t = np.concatenate([1e-3 * rng.standard_normal((4, D)), np.full((1, D), 2.0 ** -6), np.full((4, D), half) * np.exp2(np.arange(4.0) * 2 - 2)[:, None],
                        -np.full((2, D), half) * np.array([[1.0], [16.0]])]).astype(np.float32)
    Q = len(t)
    c = np.full((Q, D), 1.0 / D, np.float32)
    xd, qd, cd = bank.cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(c).cuda()
    a = pqr.contract_distances(c, t, xw.reshape(N * P, D)).reshape(Q, N, P)
    for k in (1, 100):
        out_s, out_i, redo, _ = _direct(ops, cd, qd, xd, k, combine, off)
        assert int(redo.sum()) == 0
        rs, ri = tdr.topk_of_token_distances(a, k, combine, idx_offset=off)
        assert np.array_equal(out_i.cpu().numpy(), ri), (k, np.argwhere(out_i.cpu().numpy() != ri)[:4])
        assert np.array_equal((-out_s).cpu().numpy().view(np.uint32), rs.view(np.uint32))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("lo", [0, 1])
def test_query_images_and_constants_against_the_reference(dt, lo, monkeypatch):
    """What mse_pq_query_kernel leaves in the workspace -- qh, ql, qbase = {A_dn, eps_pq ||u'||, 2^-f, flag} -- against
    tests/token_mse_pq_reference.query_constants, the model the CPU soundness tests run on: the images value for value, the scale
    exactly, A_dn never above the fp64 sum and within the stated slack below it, eps_pq ||u'|| never below its fp64 value and within
    the slack above; the flags, and redo, query for query."""
    from sky_embeddings_amd import ops
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", str(lo))
    rng = np.random.default_rng(53 + lo)
    N, P, D, Q, k = 1024, 4, 160, 21, 5
    bank, _ = _bank(rng, N, P, D, dt)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    c = np.minimum(_weights(rng, Q, D) / np.float32(D), np.float32(2.0 ** 9)).astype(np.float32)
    q[3] = 0.0                                                     # c o t = 0
    q[4] *= 1e-3
    q[5] *= 300.0
    c[6, 17] = -1e-3
    c[7, 5] = np.nan
    c[8, 9] = 2048.0
    c[9, ::2] = 0.0
    xd, qd, cd = bank.cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    _, _, redo, ws = _direct(ops, cd, qd, xd, k, "min", 0)
    torch.cuda.synchronize()
    arr = H.ws_arrays(ws.cpu().numpy(), ops.token_prefilter_ws_layout(Q, 2 * D, k), Q, 2 * D)
    qc = pqr.query_constants(c, q, dt, bool(lo))
    wide = (lambda u16: torch.from_numpy(np.ascontiguousarray(u16).view(np.int16)).view(DTYPES[dt]).float().numpy())
    qb = arr["qbase"].astype(np.float64)
    fl = qc["flagged"]
    assert fl.tolist() == [i in (3, 6, 7, 8) for i in range(Q)]
    assert np.array_equal(redo.cpu().numpy() != 0, fl)
    ok = ~fl
    assert np.array_equal(wide(arr["qh"][:Q])[ok], qc["qh"][ok])
    if lo:
        assert np.array_equal(wide(arr["ql"][:Q])[ok], qc["ql"][ok])
    assert (arr["qh"][Q:] == 0).all() and (arr["ql"][Q:] == 0).all()           # the padding rows of the query tile
    assert np.array_equal(qb[ok, 2], qc["s"][ok]) and (qb[ok, 3] == 0).all() and (qb[[6, 7, 8], 3] != 0).all()
    slack = 2.0 * (2 * D) * 2.0 ** -22
    assert (qb[ok, 0] <= qc["A64"][ok]).all() and (qb[ok, 0] >= qc["A64"][ok] * (1.0 - slack)).all()
    nq64 = np.sqrt(((qc["u"].astype(np.float64) * qc["s"][:, None]) ** 2).sum(axis=1))
    need = pqr.eps_pq(D, bool(lo), dt) * nq64
    assert (qb[ok, 1] >= need[ok]).all() and (qb[ok, 1] <= need[ok] * (1.0 + slack)).all()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("combine", ["min", "max"])
def test_hostile_banks_and_queries_are_decided_exactly(dt, combine):
    """A query with a negative weight and an all-zero query are re-run, they alone; an image with an element of magnitude 300 (fp16:
    its square leaves the format, the row is unboundable) that belongs to a top-k is returned; an image with a NaN token is ignored
    token-wise under 'min' and dropped under 'max'; duplicated images come back lower index first."""
    rng = np.random.default_rng(23)
    N, P, D, Q, k = 1024, 4, 128, 40, 12
    q = rng.standard_normal((Q, D)).astype(np.float32)
    x = (rng.standard_normal((N, 1, D)) + 0.7 * rng.standard_normal((N, P, D))).astype(np.float32)
    x[10, 2] = np.nan
    x[11] = np.nan
    x[12, 1, 7] = np.inf
    x[13, 3] = 0.0
    x[200:206] = x[100]                                            # six copies of image 100
    x[300] = x[301] + 0.01 * rng.standard_normal((P, D)).astype(np.float32)
    x[300, :, 9] = 300.0                                           # every token of image 300 holds it
    if dt == "bf16":
        x[15, 0, 4] = 1e-20                                        # the square is below the bf16 window
        x[16, 1, 3] = 2.0 ** 61
    bank, xw = _to16(x, dt)
    q[5] = xw[100, 0]
    q[6] = xw[300, 1]                                              # image 300 is this query's best under min and max
    q[7] = xw[10, 0]                                               # a finite token of the image with a NaN token
    q[20] = 0.0
    w = rng.random((Q, D)).astype(np.float32) + 0.5
    w[30, 9] = -0.25
    got, ref = _both(q, bank, w, k, combine)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] == 2, got[2]     # queries 20 and 30, no other
    flat = got[1].flatten().tolist()
    assert 11 not in flat and ((10 not in flat and 12 not in flat) if combine == "max" else True)
    assert got[1][6, 0].item() == 300
    if combine == "min":
        assert got[1][7, 0].item() == 10 and got[0][7, 0].item() == 0.0
        assert got[1][5].tolist()[:7] == [100, 200, 201, 202, 203, 204, 205]      # ties: the lower image first


def test_fewer_finite_images_than_k():
    """k = 30 over 40 images of which 25 hold a NaN token: under 'max' 15 images have a finite distance, the tail is (+inf, -1)."""
    rng = np.random.default_rng(31)
    N, P, D, Q, k = 40, 64, 128, 33, 30
    x = rng.standard_normal((N, P, D)).astype(np.float32)
    x[15:, 5, 3] = np.nan
    bank, _ = _to16(x, "bf16")
    q = rng.standard_normal((Q, D)).astype(np.float32)
    got, ref = _both(q, bank, _weights(rng, Q, D), k, "max")
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered"
    assert (got[1][:, 15:] == -1).all() and torch.isinf(got[0][:, 15:]).all() and (got[1][:, :15] >= 0).all()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_image_and_row_constants_against_the_reference(dt):
    """The image read back bit for bit, ny never below its fp64 value and within the stated slack above, unboundable rows (zero
    image row, {0, inf, 1, 0}), the padding (zero rows, the sentinel) -- written into guarded buffers: nothing outside them."""
    from sky_embeddings_amd import ops
    rng = np.random.default_rng(37)
    N, P, D = 523, 4, 160
    x = (rng.standard_normal((N, P, D)) * rng.uniform(0.01, 30.0, (N, P, 1))).astype(np.float32)
    x[3, 1, 5] = np.inf
    x[4, 2, 7] = np.nan
    x[5, 0] = 2.0 ** -20 * rng.integers(-15, 16, D)
    x[6, 3] = 0.0
    x[7, 0, 9] = 1e-20
    x[8, 1] = 255.875
    x[9, 2, 11] = 256.0
    x[10, 0] = rng.uniform(-1, 1, D) * 2.0 ** -8                    # fp16: every square on the subnormal grid
    x[11, 3, 0] = 2.0 ** 61
    bank, xw = _to16(x, dt)
    xd = bank.cuda()
    R, rows, size = N * P, 2304, bank.element_size()
    gi, gr = H.Guarded(rows * 2 * D * size), H.Guarded(rows * 16)
    image, rowp = ops.token_mse_pq_image(xd, gi.t(DTYPES[dt], rows, 2 * D), gr.t(torch.float32, rows, 4))
    torch.cuda.synchronize()
    assert gi.intact() and gr.intact()
    y, ub = pqr.image(xw.reshape(R, D), dt)
    ny64, _ = pqr.row_constants(xw.reshape(R, D), dt)
    want = _to16(y, dt)[0]
    assert torch.equal(image[:R].cpu().view(torch.int16), want.view(torch.int16))
    assert (image[R:] == 0).all()
    rp = rowp.cpu().numpy().astype(np.float64)
    assert ub.sum() >= 3 and np.array_equal(np.isinf(rp[:R, 1]), ub)
    assert (rp[:R][ub] == np.array([0.0, np.inf, 1.0, 0.0])).all() and (image[:R].cpu().float().numpy()[ub] == 0).all()
    ok = ~ub
    slack = 2.0 * (2 * D) * 2.0 ** -22
    assert (rp[:R, 1][ok] >= ny64[ok]).all() and (rp[:R, 1][ok] <= ny64[ok] * (1.0 + slack)).all()
    assert (rp[:R, 0] == 0.0).all() and (rp[:R, 2] == 1.0).all() and (rp[:, 3] == 0.0).all()
    assert np.isnan(rp[R:, 1]).all() and (rp[R:, 0] == 0.0).all() and (rp[R:, 2] == 0.0).all()


def test_a_search_after_set_weights_still_takes_the_route():
    from sky_embeddings_amd import search
    rng = np.random.default_rng(41)
    N, P, D, Q, k = 1024, 4, 128, 20, 7
    bank, _ = _bank(rng, N, P, D, "f16")
    q = rng.standard_normal((Q, D)).astype(np.float32)
    tb = search.TokenBank.resident(bank.cuda()).prepare_mse_per_query()
    held = tb._mse_pq
    tb.set_weights(torch.from_numpy(rng.random(D).astype(np.float32) + 0.1).cuda())
    assert tb._mse_pq is held and tb.prepare_mse_per_query() is tb and tb._mse_pq is held
    got, ref = _both(q, bank, _weights(rng, Q, D), k, "min", prepared=tb)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["per_query_weights"] is True and ref[2]["path"] == "tokens"
