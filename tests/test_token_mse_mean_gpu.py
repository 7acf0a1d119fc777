"""GPU: the two-stage many-query weighted-MSE search under combine 'mean' --
``distance_topk_tokens(q, TokenBank.resident(bank).prepare_mse_mean(), k, 'MSE', 'mean')``.

The reference of every case is the same call over the same device bank in a plain ``TokenBank`` (the grouped route); distances and
indices must be bit-equal.  D = 160 is a shape the grouped kernels do not take (they need D % 64 == 0), so there the library call is
compared with the NumPy restatement of the contract (tests/token_mse_mean_reference.contract_mean).  The conditions the cases put on
their inputs (no flagged query, no list that could overflow) are checked on the CPU, tests/test_token_mse_mean_cpu.py."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import token_mse_mean_reference as mr
from tests import token_mse_prefilter_reference as mpr

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
D = 128


@pytest.fixture(autouse=True)
def _min_q(monkeypatch):
    from sky_embeddings_amd import search
    monkeypatch.setattr(search, "TOKEN_MSE_MEAN_PREFILTER_MIN_Q", 17)
    monkeypatch.setattr(search, "TOKEN_MSE_PREFILTER_MIN_Q_SMALL", 17)


def _to16(x, dt):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DTYPES[dt])
    return t, t.float().numpy()


def _bank(rng, N, P, Dn, dt):
    """Images of very different scale whose tokens share a direction, as a 16-bit tensor and the fp32 array it widens to."""
    x = (rng.standard_normal((N, 1, Dn)) * rng.uniform(0.3, 2.0, (N, 1, 1)) + 0.7 * rng.standard_normal((N, P, Dn))).astype(np.float32)
    return _to16(x, dt)


def weights_c(w, Dn):
    """c = fp32(w / sum w) as ``prepare_distance_weights`` forms it (on the CPU here: the flags do not depend on the last bit)."""
    from sky_embeddings_amd import search
    return search.prepare_distance_weights(None if w is None else torch.from_numpy(w), Dn, "cpu").numpy()


# (N, P, dtype, SKYEMB_PREFILTER_LO, Q, k, weighted, idx_offset).  (2092, 4): a tail tile; (2560, 1): no tail, the mean of one token;
# (2100, 16); (2048, 64): the smallest N the rule takes and the widest fold.  Q = 130 / 300 cross the 128- and 256-query tiles.
CASES = [
    (2092, 4, "f16", 1, 130, 8, True, 0), (2092, 4, "bf16", 0, 300, 256, False, 7), (2092, 4, "bf16", 1, 130, 1, True, 1000),
    (2560, 1, "f16", 0, 300, 8, False, 0), (2560, 1, "bf16", 1, 130, 256, True, 0), (2100, 16, "f16", 1, 300, 1, False, 3),
    (2100, 16, "bf16", 0, 130, 8, True, 0), (2100, 16, "f16", 0, 130, 256, True, 0), (2048, 64, "f16", 1, 130, 256, False, 0),
    (2048, 64, "bf16", 1, 300, 8, True, 11), (2048, 64, "f16", 0, 300, 1, True, 0), (2048, 64, "bf16", 0, 130, 1, False, 0),
]


def inputs(case):
    """-> (the widened bank fp32 [N, P, D], queries fp32 [Q, D], weights fp32 [D] or None) of a case; query 3 is an image's pooled
    tokens (the fp32 mean of its widened tokens)."""
    N, P, dt, lo, Q, k, weighted, off = case
    rng = np.random.default_rng(N + P + Q + k + lo)
    _, xw = _bank(rng, N, P, D, dt)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    q[3] = xw[N // 2].mean(axis=0)
    w = (rng.random(D).astype(np.float32) + 0.05) * np.exp2(-8.0 * rng.random(D)).astype(np.float32) if weighted else None
    return xw, q, w


def _both(q, bank, w, k, idx_offset=0, prepared=None, **kw):
    """((distances, indices, stats) of the prepared bank, the same of a plain TokenBank); bank: a 16-bit tensor."""
    from sky_embeddings_amd import search
    qd, xd = torch.from_numpy(q).cuda(), bank.cuda()
    wd = None if w is None else torch.from_numpy(w).cuda()
    asked = search.TokenBank.resident(xd, wd, idx_offset).prepare_mse_mean() if prepared is None else prepared
    out = []
    for tb in (asked, search.TokenBank(xd, wd, idx_offset)):
        stats = {}
        s, i = search.distance_topk_tokens(qd, tb, k, "MSE", "mean", stats=stats, **kw)
        out.append((s, i, stats))
    return out


def _assert_same(got, ref):
    assert torch.equal(got[1], ref[1]), (got[2], torch.nonzero(got[1] != ref[1])[:5].tolist())
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)), got[2]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-P%d-%s-lo%d-Q%d-k%d-w%d-off%d" % c)
def test_two_stage_mean_topk_is_bit_exact(case, monkeypatch):
    N, P, dt, lo, Q, k, weighted, off = case
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", str(lo))
    xw, q, w = inputs(case)
    bank = torch.from_numpy(xw).to(DTYPES[dt])
    got, ref = _both(q, bank, w, k, off)
    print(got[2])
    _assert_same(got, ref)
    assert ref[2]["path"] == "tokens"
    assert got[2]["path"] == "prefiltered" and got[2]["metric"] == "MSE" and got[2]["combine"] == "mean" and got[2]["redone"] == 0, got[2]
    assert got[1][3, 0].item() == off + N // 2


D160_PARAMS = [("f16", 1, 100), ("bf16", 0, 1), ("f16", 0, 1), ("bf16", 1, 100)]


def d160_inputs(dt, lo, k):
    """-> (the widened bank fp32 [2092, 4, 160], queries [33, 160], c [160]) of a D = 160 case."""
    rng = np.random.default_rng(160 + k)
    N, P, Dn, Q = 2092, 4, 160, 33
    _, xw = _bank(rng, N, P, Dn, dt)
    q = rng.standard_normal((Q, Dn)).astype(np.float32)
    q[2] = xw[N - 1].mean(axis=0)                                  # the bank's last image, in the ragged tile
    c = rng.random(Dn).astype(np.float32) + 0.05
    return xw, q, (c / c.sum()).astype(np.float32)


@pytest.mark.parametrize("dt,lo,k", D160_PARAMS)
def test_ragged_d160_against_the_contract(dt, lo, k, monkeypatch):
    """bank (2092, 4, 160) through the C ABI entry: five 32-element k-steps in stage 1, a tail tile; against NumPy."""
    from sky_embeddings_amd import ops
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", str(lo))
    N, P, Dn, Q, off = 2092, 4, 160, 33, 11
    xw, q, c = d160_inputs(dt, lo, k)
    bank = torch.from_numpy(xw).to(DTYPES[dt])
    xd, qd, cd = bank.cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    pooled, tail, aux = ops.token_mse_mean_pool(xd)
    rowp = ops.token_mse_mean_rowp(xd, cd, aux)
    assert pooled.shape == (N, Dn) and tail.shape == (256, Dn) and aux.shape == (2304, 2) and rowp.shape == (2304, 4)
    out_s, out_i = torch.empty(Q, k, device="cuda"), torch.empty(Q, k, device="cuda", dtype=torch.int64)
    redo = torch.empty(Q, device="cuda", dtype=torch.int32)
    ops.distance_topk_tokens_mean_prefiltered(cd, qd, xd, pooled, tail, rowp, k, off, out_s, out_i, redo)
    assert int(redo.sum()) == 0
    rs, ri = mr.topk(mr.contract_mean(c, q, xw), k, idx_offset=off)
    assert np.array_equal(out_i.cpu().numpy(), ri)
    assert np.array_equal((-out_s).cpu().numpy().view(np.uint32), rs.view(np.uint32))
    assert ri[2, 0] == off + N - 1


READBACK_PARAMS = [("f16", 1), ("bf16", 1), ("f16", 0), ("bf16", 0)]


def readback_inputs(dt, lo):
    """-> (the widened bank fp32 [2092, 4, 128], queries [64, 128], c [128]) of a read-back case; image 17 pools to exact zero."""
    rng = np.random.default_rng(64 + lo)
    N, P, Q = 2092, 4, 64
    _, xw = _bank(rng, N, P, D, dt)
    xw[17] = np.stack([xw[17, 0], -xw[17, 0], xw[17, 1], -xw[17, 1]])        # an exactly zero pooled row
    q = rng.standard_normal((Q, D)).astype(np.float32)
    q[5] = xw[40].mean(axis=0)
    c = rng.random(D).astype(np.float32) + 0.05
    return xw, q, (c / c.sum()).astype(np.float32)


@pytest.mark.parametrize("dt,lo", READBACK_PARAMS)
def test_per_image_constants_read_back(dt, lo):
    """64 queries x (2092, 4): every element of the pooled image bit for bit, the tail tile, rowp on the safe side of its fp64 values,
    and for every pair L <= D mean^ (1 + gamma) + 2^-126 from the DEVICE's constants, against the fp64 mean and the contract's fp32
    value.  dot^ is the exact sum of the 16-bit operands' products over the device's pooled image, rounded to fp32 (one of the values
    the matrix cores may return).  The margins are printed, and appended as one JSON line to $SKYEMB_MSE_MEAN_MARGINS when that names a
    file: tools/mse_mean_margins.py runs this test that way and writes profiles/mse_mean_margins.json."""
    from sky_embeddings_amd import ops
    N, P, Q = 2092, 4, 64
    xw, q, c = readback_inputs(dt, lo)
    bank = torch.from_numpy(xw).to(DTYPES[dt])
    xd, cd = bank.cuda(), torch.from_numpy(c).cuda()
    pooled, tail, aux = ops.token_mse_mean_pool(xd)
    rowp = ops.token_mse_mean_rowp(xd, cd, aux).cpu().numpy()
    got = pooled.float().cpu().numpy()
    assert mr.check_pooled(got, xw, dt)
    assert not got[17].any() and np.isfinite(rowp[17]).all() and rowp[17, 2] == 1.0
    tl = tail.float().cpu().numpy()
    assert np.array_equal(tl[:N - 2048].view(np.uint32), got[2048:].view(np.uint32)) and not tl[N - 2048:].any()
    assert mr.check_rowp(rowp, c, xw, dt)
    assert np.isnan(rowp[N:, 1]).all() and not rowp[N:, [0, 2, 3]].any()
    L, trusted, dot = mr.lower_bounds(c, q, xw, dt, bool(lo), rowp=rowp)
    assert trusted.all()
    g = mr.gamma(D, P)
    d32 = mr.contract_mean(c, q, xw).astype(np.float64) * D
    # (sum_d c_d (x_d - t_d)^2 IS D x the distance: the contract divides by D)
    d64 = (c.astype(np.float64) * (xw.astype(np.float64)[None] - q.astype(np.float64)[:, None, None]) ** 2).sum(axis=3).mean(axis=2)
    for rhs in (d64 * (1.0 + g) + 2.0 ** -126, d32 * (1.0 + g) + 2.0 ** -126):
        assert (L <= rhs).all()
    qc = mr.query_constants(c, q, dt, bool(lo))
    s_img = rowp[:N, 2].astype(np.float64)
    real = ((c.astype(np.float64) * q.astype(np.float64)) @ xw.astype(np.float64).mean(axis=1).T) * qc["s"][:, None] * s_img[None, :]
    bound = qc["cq"][:, None] * rowp[:N, 1].astype(np.float64)[None, :]
    pos = d64 > 2.0 ** -20
    figures = dict(dtype=dt, lo=lo, N=N, P=P, D=D, Q=Q, max_L_over_rhs=float((L[pos] / (d64[pos] * (1.0 + g))).max()),
                   max_dot_error_over_bound=float((np.abs(dot - real) / bound).max()))
    print(figures)
    assert figures["max_dot_error_over_bound"] <= 1.0
    path = os.environ.get("SKYEMB_MSE_MEAN_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(figures) + "\n")


def _hostile(dt):
    rng = np.random.default_rng(99)
    N, P = 2092, 4
    _, x = _bank(rng, N, P, D, dt)
    x[100] = x[50]
    x[101] = x[50]                                                 # duplicated images: tie order
    x[200, 1, :] = np.nan                                          # one NaN token
    x[201] = np.nan                                                # an all-NaN image
    x[202, 3, 5] = np.inf                                          # an inf element
    x[300, 2] = 0.0                                                # a zero token row
    x[301] = np.stack([x[301, 0], -x[301, 0], x[301, 1], -x[301, 1]])     # the pooled row is exactly zero
    if dt == "f16":
        x[400:410] *= np.float32(2.0 ** -12)
        x[410:420] *= np.float32(2.0 ** 12)                        # (standard-normal x 2^12 stays inside fp16)
    else:
        x[400, 0, 3] = np.float32(2.0 ** 121)
        x[401, 2, 9] = np.float32(2.0 ** -70)                      # outside the bf16 window on either side
        x[402, 1, :] = np.float32(2.0 ** 100)
    return _to16(x, dt)


HOSTILE_PARAMS = [("f16", 1, 8), ("bf16", 1, 8), ("f16", 0, 256), ("bf16", 0, 1)]
HOSTILE_ZERO_QUERY = 9


def hostile_inputs(dt):
    """-> (the 16-bit bank, the fp32 array it widens to, queries [130, 128]); query HOSTILE_ZERO_QUERY is zero, the one query the
    route hands back."""
    bank, xw = _hostile(dt)
    rng = np.random.default_rng(7)
    q = rng.standard_normal((130, D)).astype(np.float32)
    q[0] = xw[50].mean(axis=0)                                     # the duplicates' own pooled tokens: a three-way tie at the top
    q[1] = xw[405].mean(axis=0) if dt == "f16" else q[1]
    q[2] = xw[415].mean(axis=0) if dt == "f16" else q[2]
    q[HOSTILE_ZERO_QUERY] = 0.0                                    # a zero query: re-run by the grouped route
    return bank, xw, q


@pytest.mark.parametrize("dt,lo,k", HOSTILE_PARAMS)
def test_hostile_banks_are_bit_equal(dt, lo, k, monkeypatch):
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", str(lo))
    bank, xw, q = hostile_inputs(dt)
    got, ref = _both(q, bank, None, k)
    print(got[2])
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] == 1, got[2]       # the zero query alone (the CPU file predicts the rest)
    idx = got[1].cpu().numpy()
    assert not np.isin(idx, [200, 201, 202]).any()                # never returned under 'mean'
    if k >= 3:
        assert idx[0, :3].tolist() == [50, 100, 101]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_a_negative_weight_sends_every_query_back(dt):
    rng = np.random.default_rng(3)
    N, P, Q = 2092, 4, 40
    bank, _ = _bank(rng, N, P, D, dt)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    w = np.ones(D, np.float32)
    w[5] = -0.25
    got, ref = _both(q, bank, w, 8)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] == Q, got[2]


def optin_inputs():
    """-> (the widened fp16 bank fp32 [2092, 4, 128], queries [130, 128], the weights set_weights installs [128])."""
    rng = np.random.default_rng(11)
    _, xw = _bank(rng, 2092, 4, D, "f16")
    q = rng.standard_normal((130, D)).astype(np.float32)
    return xw, q, rng.random(D).astype(np.float32) + 0.1


def test_opt_in_selection_top_t_and_set_weights():
    from sky_embeddings_amd import search
    N, P, Q, k = 2092, 4, 130, 8
    xw, q, w = optin_inputs()
    bank = torch.from_numpy(xw).to(torch.float16)
    xd, qd = bank.cuda(), torch.from_numpy(q).cuda()
    # the same resident bank without the opt-in
    stats = {}
    search.distance_topk_tokens(qd, search.TokenBank.resident(xd), k, "MSE", "mean", stats=stats)
    assert stats["path"] == "tokens"
    tb = search.TokenBank.resident(xd).prepare_mse_mean()
    assert tb.prepare_mse_mean() is tb
    for kw in (dict(top_t=2), dict(select=search.Selection(torch.arange(N, device="cuda") % 2 == 0))):
        stats = {}
        search.distance_topk_tokens(qd, tb, k, "MSE", "mean", stats=stats, **kw)
        assert stats["path"] == "tokens", (kw, stats)
    got, ref = _both(q, bank, None, k, prepared=tb)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered"
    pooled0, tail0, rowp0 = tb.stage1_mse_mean(search.prepare_distance_weights(None, D, "cuda"))
    # after set_weights: the pooled image is kept (same storage), rowp is rebuilt, the results are bit-equal again
    tb.set_weights(torch.from_numpy(w).cuda())
    stats = {}
    s, i = search.distance_topk_tokens(qd, tb, k, "MSE", "mean", stats=stats)
    pooled1, tail1, rowp1 = tb.stage1_mse_mean(search.prepare_distance_weights(tb.weights, D, "cuda"))
    assert pooled1.data_ptr() == pooled0.data_ptr() and tail1.data_ptr() == tail0.data_ptr()
    assert rowp1 is not rowp0 and not torch.equal(rowp1[:N, 0], rowp0[:N, 0]) and torch.equal(rowp1[:N, 1:], rowp0[:N, 1:])
    s2, i2 = search.distance_topk_tokens(qd, search.TokenBank(xd, torch.from_numpy(w).cuda()), k, "MSE", "mean")
    assert stats["path"] == "prefiltered" and stats["redone"] == 0
    assert torch.equal(i, i2) and torch.equal(s.view(torch.int32), s2.view(torch.int32))
    with pytest.raises(ValueError, match="TokenBank.resident"):
        search.TokenBank(xd).prepare_mse_mean()


def bbar_adversary(dt, P=64):
    """-> (bank fp32 [8, P, 128] of 16-bit values, c [128]): in every image one lane of the row-constants kernel sums a dominant
    first term followed by 8 P - 1 terms just above half an ulp of it, so every fp32 addition rounds UP: the fp32 sum exceeds the
    real one by about (8 P - 1) 2^-24 relative, the most its chain of 8 P fused multiply-adds allows."""
    x = np.zeros((8, P, D), np.float32)
    small = np.float32(2.0 ** -12) * (np.float32(1) + np.float32(2.0 ** -10 if dt == "f16" else 2.0 ** -7))
    for i in range(8):
        x[i, :, 8 * i:8 * i + 8] = small                           # image i loads lane i
        x[i, 0, 8 * i] = 1.0
    return x, np.ones(D, np.float32)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_bbar_is_never_raised_by_its_own_summation(dt):
    """D = 128, P = 64: 16 lanes are active and each adds 8 P = 512 terms, four times P D / 64.  On a bank built to round up at
    every step the device's R0 still lies at or below the real Bbar 2^-e."""
    from sky_embeddings_amd import ops
    xw, c = bbar_adversary(dt)
    assert np.array_equal(mpr.to16(xw, dt), xw)
    rc = mr.row_constants(c, xw, dt)
    modelled = mr.bbar_kernel_order(c, xw).astype(np.float64)
    assert (modelled > rc["Bbar64"] * (1.0 + 400 * 2.0 ** -24)).all()                # the premise: the fp32 sum IS too high
    xd = torch.from_numpy(xw).to(DTYPES[dt]).cuda()
    pooled, tail, aux = ops.token_mse_mean_pool(xd)
    rowp = ops.token_mse_mean_rowp(xd, torch.from_numpy(c).cuda(), aux).cpu().numpy().astype(np.float64)
    s = rc["s"].astype(np.float64)
    print(dict(dtype=dt, device_over_real=(rowp[:8, 0] / s / rc["Bbar64"]).max(), modelled_over_real=(modelled / rc["Bbar64"]).max()))
    assert not rc["unboundable"].any() and (rowp[:8, 2] == s).all()
    assert (rowp[:8, 0] <= rc["Bbar64"] * s).all()
    assert mr.check_rowp(rowp, c, xw, dt)
