"""GPU: the two-stage many-query weighted-MSE search over a resident 16-bit patch-token bank --
``distance_topk_tokens(queries, TokenBank.resident(bank), k, 'MSE', combine)`` with combine 'min' | 'max'.

The reference of every case is the same call over the same device bank in a plain ``TokenBank`` (the grouped route); distances and
indices must be bit-equal.  D = 160 is a shape the grouped kernels do not take (they need D % 64 == 0), so there the library call is
compared with the NumPy restatement of the contract instead (tests/token_mse_prefilter_reference.contract_distances)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import token_distance_reference as tdr
from tests import token_mse_prefilter_reference as mpr

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(autouse=True)
def _min_q(monkeypatch):
    from sky_embeddings_amd import search
    monkeypatch.setattr(search, "TOKEN_MSE_PREFILTER_MIN_Q", 17)
    monkeypatch.setattr(search, "TOKEN_MSE_PREFILTER_MIN_Q_SMALL", 17)


def _bank(rng, N, P, D, dt):
    """Images of very different scale whose tokens share a direction, as a 16-bit tensor and the fp32 array it widens to."""
    x = (rng.standard_normal((N, 1, D)) * rng.uniform(0.3, 2.0, (N, 1, 1)) + 0.7 * rng.standard_normal((N, P, D))).astype(np.float32)
    return _to16(x, dt)


def _to16(x, dt):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DTYPES[dt])
    return t, t.float().numpy()


def _both(q, bank, w, k, combine, idx_offset=0):
    """((distances, indices, stats) of the resident bank, the same of the plain one); bank: a 16-bit tensor."""
    from sky_embeddings_amd import search
    qd, xd = torch.from_numpy(q).cuda(), bank.cuda()
    wd = None if w is None else torch.from_numpy(w).cuda()
    out = []
    for tb in (search.TokenBank.resident(xd, wd, idx_offset), search.TokenBank(xd, wd, idx_offset)):
        stats = {}
        s, i = search.distance_topk_tokens(qd, tb, k, "MSE", combine, stats=stats)
        out.append((s, i, stats))
    return out


def _assert_same(got, ref):
    assert torch.equal(got[1], ref[1]), (got[2], torch.nonzero(got[1] != ref[1])[:5].tolist())
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)), got[2]


# (N, P): 2092 rows with a tail tile and images straddling tiles (P = 4), the same rows as a row bank, 2560 rows without a tail
# and with whole-strip images.  Q crosses the 128- and the 256-query tile, k the list sizes; every dtype, combine and variant.
CASES = [
    (523, 4, "f16", "min", 0, 130, 8, 0), (523, 4, "bf16", "max", 1, 300, 1, 7), (523, 4, "f16", "max", 1, 300, 256, 0),
    (2092, 1, "bf16", "min", 0, 130, 256, 1000), (2092, 1, "f16", "max", 1, 130, 1, 0), (2092, 1, "bf16", "min", 1, 300, 8, 0),
    (40, 64, "f16", "min", 1, 300, 8, 3), (40, 64, "bf16", "max", 0, 130, 1, 0), (40, 64, "f16", "max", 0, 130, 8, 0),
    (40, 64, "bf16", "min", 1, 130, 8, 0), (523, 4, "bf16", "min", 0, 130, 8, 0), (2092, 1, "f16", "min", 0, 300, 8, 5),
]


@pytest.mark.parametrize("c", CASES, ids=lambda c: "N%d-P%d-%s-%s-lo%d-Q%d-k%d-off%d" % c)
def test_two_stage_mse_topk_is_bit_exact(c, monkeypatch):
    N, P, dt, combine, lo, Q, k, off = c
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", str(lo))
    rng = np.random.default_rng(N + P + Q + k)
    D = 128
    bank, xw = _bank(rng, N, P, D, dt)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    q[3] = xw[N // 2, P - 1]                                       # a query that is itself a bank row
    w = (rng.random(D, dtype=np.float32) + 0.05) if (N + Q) % 2 else None
    got, ref = _both(q, bank, w, k, combine, off)
    print(got[2])
    _assert_same(got, ref)
    assert ref[2]["path"] == "tokens"
    assert got[2]["path"] == "prefiltered" and got[2]["combine"] == combine and got[2]["metric"] == "MSE", got[2]
    # no query is flagged: weights in [0, 1], scales and A_q inside the windows (tests/test_token_mse_prefilter_cpu.py), a 4096-entry
    # list holds every image of these banks, and the flags depend on the data alone
    assert got[2]["redone"] == 0, got[2]
    if combine == "min":
        assert got[1][3, 0].item() == off + N // 2 and got[0][3, 0].item() == 0.0


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("combine", ["min", "max"])
def test_d160_against_the_contract(dt, combine, monkeypatch):
    """D = 160 (five 32-element k-steps; the 16 partials hold unequal numbers of terms): the library call against NumPy."""
    from sky_embeddings_amd import ops
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", "1" if dt == "f16" else "0")
    rng = np.random.default_rng(160)
    N, P, D, Q, k, off = 523, 4, 160, 130, 8, 11
    bank, xw = _bank(rng, N, P, D, dt)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    cd = (torch.from_numpy(rng.random(D, dtype=np.float32) + 0.05).cuda())
    cd = (cd / cd.sum()).contiguous()
    xd, qd = bank.cuda(), torch.from_numpy(q).cuda()
    tail, rowp = ops.token_mse_rowp(xd, cd)
    out_s, out_i = torch.empty(Q, k, device="cuda"), torch.empty(Q, k, device="cuda", dtype=torch.int64)
    redo = torch.empty(Q, device="cuda", dtype=torch.int32)
    ops.distance_topk_tokens_prefiltered(cd, qd, xd, tail, rowp, k, ops.COMBINE_CODES[combine], off, out_s, out_i, redo)
    assert int(redo.sum()) == 0
    a = mpr.contract_distances(cd.cpu().numpy(), q, xw.reshape(N * P, D)).reshape(Q, N, P)
    rs, ri = tdr.topk_of_token_distances(a, k, combine, idx_offset=off)
    assert np.array_equal(out_i.cpu().numpy(), ri)
    assert np.array_equal((-out_s).cpu().numpy().view(np.uint32), rs.view(np.uint32))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("combine", ["min", "max"])
def test_hostile_banks_are_decided_exactly(dt, combine):
    """Duplicated images (tie order), an image with a NaN token and one with an inf token, a zero row, a zero query; bf16: a row
    outside the [2^-60, 2^120) window."""
    rng = np.random.default_rng(23)
    N, P, D, Q, k = 640, 4, 128, 40, 12
    q = rng.standard_normal((Q, D)).astype(np.float32)
    x = (rng.standard_normal((N, 1, D)) + 0.7 * rng.standard_normal((N, P, D))).astype(np.float32)
    x[10, 2] = np.nan
    x[11] = np.nan
    x[12, 1, 7] = np.inf
    x[13, 3] = 0.0
    x[200:206] = x[100]                                            # six copies of image 100
    q[20] = 0.0
    q[5] = x[100, 0]
    if dt == "bf16":
        x[15, 0, 4] = 1e-30
        x[16, 1, 3] = 1e+37
    bank, _ = _to16(x, dt)
    got, ref = _both(q, bank, None, k, combine)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] >= 1, got[2]     # the zero query is outside what stage 1 bounds
    flat = got[1].flatten().tolist()
    assert 11 not in flat and ((10 not in flat and 12 not in flat) if combine == "max" else True)
    if combine == "min":                                           # query 5 is a token of image 100 and of its six copies
        assert got[1][5].tolist()[:7] == [100, 200, 201, 202, 203, 204, 205]      # ties: the lower image first


def test_a_negative_weight_sends_every_query_back():
    rng = np.random.default_rng(29)
    N, P, D, Q, k = 523, 4, 128, 40, 5
    bank, _ = _bank(rng, N, P, D, "f16")
    q = rng.standard_normal((Q, D)).astype(np.float32)
    w = rng.random(D, dtype=np.float32) + 0.5
    w[9] = -0.25
    got, ref = _both(q, bank, w, k, "min")
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] == Q, got[2]


def test_fewer_finite_images_than_k():
    """k = 30 over 40 images of which 25 hold a NaN token: under 'max' 15 images have a finite distance, the tail is (+inf, -1)."""
    rng = np.random.default_rng(31)
    N, P, D, Q, k = 40, 64, 128, 33, 30
    x = rng.standard_normal((N, P, D)).astype(np.float32)
    x[15:, 5, 3] = np.nan
    bank, _ = _to16(x, "bf16")
    q = rng.standard_normal((Q, D)).astype(np.float32)
    got, ref = _both(q, bank, None, k, "max")
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered"
    assert (got[1][:, 15:] == -1).all() and torch.isinf(got[0][:, 15:]).all() and (got[1][:, :15] >= 0).all()


def test_more_near_duplicates_than_a_list_holds():
    """10 000 images that are copies of query 3: more candidates than the 4096-entry list.  The query is flagged, re-run by the
    grouped route, and the result is still bit-equal (ties to the lower image)."""
    rng = np.random.default_rng(13)
    N, P, D, Q, k = 12000, 2, 128, 20, 9
    q = rng.standard_normal((Q, D)).astype(np.float32)
    x = rng.standard_normal((N, P, D)).astype(np.float32)
    x[1000:11000] = q[3]
    bank, xw = _to16(x, "f16")
    q[3] = xw[1000, 0]
    got, ref = _both(q, bank, None, k, "min")
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] >= 1, got[2]
    assert got[1][3].tolist() == list(range(1000, 1000 + k))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_row_constants_against_the_reference(dt):
    """rowp read back: B_dn never above the fp64 value of B_r and within the stated slack (2 D 2^-22) below it; the norm slot never
    below its fp64 value and within the same slack above; unboundable rows, the padding sentinel and the tail tile as stated."""
    from sky_embeddings_amd import ops, search
    rng = np.random.default_rng(37)
    N, P, D = 523, 4, 160
    x = (rng.standard_normal((N, P, D)) * rng.uniform(0.01, 30.0, (N, P, 1))).astype(np.float32)
    x[3, 1, 5] = np.inf
    x[4, 2, 7] = np.nan
    x[5, 0] = 2.0 ** -20 * rng.integers(-15, 16, D)
    x[6, 3] = 0.0
    x[7, 0, 9] = 1e-30
    x[8, 1] = 60000.0
    bank, xw = _to16(x, dt)
    w = rng.random(D, dtype=np.float32)
    w[::7] = 0.0
    c = search.prepare_distance_weights(torch.from_numpy(w), D, "cuda")
    xd = bank.cuda()
    tail, rowp = ops.token_mse_rowp(xd, c)
    R = N * P
    rp = rowp.cpu().numpy().astype(np.float64)
    assert rowp.shape == (2304, 4) and tail.shape == (256, D) and tail.dtype == bank.dtype
    B64, B_dn, nx64, ub = mpr.row_constants(c.cpu().numpy(), xw.reshape(R, D), dt)
    assert ub.sum() >= 2 and np.array_equal(np.isinf(rp[:R, 1]), ub)
    assert (rp[:R][ub] == np.array([0.0, np.inf, 1.0, 0.0])).all()
    ok = ~ub
    slack = 2.0 * D * 2.0 ** -22
    assert (rp[:R, 0][ok] <= B64[ok]).all() and (rp[:R, 0][ok] >= B64[ok] * (1.0 - slack)).all()
    assert (rp[:R, 1][ok] >= nx64[ok]).all() and (rp[:R, 1][ok] <= nx64[ok] * (1.0 + slack)).all()
    assert (rp[:R, 2] == 1.0).all() and (rp[:, 3] == 0.0).all()
    assert np.isnan(rp[R:, 1]).all() and (rp[R:, 0] == 0.0).all() and (rp[R:, 2] == 0.0).all()
    tl = tail.cpu()
    assert torch.equal(tl[:R - 2048].view(torch.int16), xd.view(R, D)[2048:].cpu().view(torch.int16)) and (tl[R - 2048:] == 0).all()
    # ... and a TokenBank keeps them for the last c seen
    tb = search.TokenBank.resident(xd)
    first = tb.stage1_mse(c)
    assert tb.stage1_mse(c.clone())[1] is first[1]
    assert tb.stage1_mse((c * 0.5).contiguous())[1] is not first[1]
