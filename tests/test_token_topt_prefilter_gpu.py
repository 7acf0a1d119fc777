"""GPU: the two-stage token search under ``top_t`` ('min' scores an image by its top_t-th best token): stage 1's counting fold image
by image against tests/token_topt_prefilter_reference.py at a pinned threshold, and the whole search through the public API, bit
for bit the grouped route over the same bank -- alone, under selections, on hostile banks --, with no query re-run on the random
banks (a re-run query would compare the grouped route with itself) and one deliberately flat bank where re-runs must happen.

Shapes: D = 128, N P = 2240 rows (eight whole 256-row tiles and a tail tile with padding rows); (P, t) = pr.PAIRS cover every DPP
step of the fold, both nibble steps, t = 1 (the OR fold) and t = P (the AND fold)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import prefilter_stage1_reference as sr
from tests import token_prefilter_stage_reference as tr
from tests import token_topt_prefilter_reference as pr
from tests import token_topt_reference as ttr
from tests.prefilter_gpu_harness import FILL32, TORCH16, Guarded, dev, prepare, ptr, set_lo, stream, ws_arrays

OFFSET = 2 ** 33 + 7
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()
    return _ops


class TopSearch:
    """One call of skyemb_cosine_topk_tokens_prefiltered_top through the C ABI over xw [N, P, D] (float32 values of `fmt`), with
    guarded outputs and a guarded workspace pre-filled with FILL (prefilter_gpu_harness.TokenSearch's construction, which has no
    top_t): .candidates(q) are the images left in query q's candidate row."""
    def __init__(self, ops, fmt, tw, qn, xw, xn, k, combine, top_t, thr0=None, idx_offset=0):
        L = ops.lib()
        Q, D = tw.shape
        N, P = xw.shape[:2]
        self.Q, self.N = Q, N
        bank, xn_d, rowp, side = prepare(ops, fmt, xw.reshape(N * P, D), xn)
        lay = ops.token_prefilter_ws_layout(Q, D, k)
        nbytes = L.skyemb_token_prefilter_ws_bytes(Q, D, k)
        ws = Guarded(nbytes)
        out_s, out_i, redo = Guarded(Q * k * 4), Guarded(Q * k * 8), Guarded(Q * 4)
        tw_d, qn_d, thr_d = dev(tw), dev(qn), dev(thr0)
        rc = L.skyemb_cosine_topk_tokens_prefiltered_top(ptr(tw_d), ptr(qn_d), Q, ptr(bank), ops.dtype_code(TORCH16[fmt]), ptr(xn_d),
                                                         side.ptr() if side is not None else None, rowp.ptr(), N, P, D, k,
                                                         ops.COMBINE_CODES[combine], top_t, sr.EPS, idx_offset, ptr(thr_d), ws.ptr(), nbytes,
                                                         out_s.ptr(), out_i.ptr(), redo.ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0, L.skyemb_last_error()
        self.guards_ok = all(g.intact() for g in (ws, out_s, out_i, redo, rowp) + ((side,) if side is not None else ()))
        self.ws = ws_arrays(ws.mem.cpu().numpy(), lay, Q, D)
        self.out_s, self.out_i, self.redo = out_s.np(np.float32, Q, k), out_i.np(np.int64, Q, k), redo.np(np.int32, Q)

    def candidates(self, q):
        row = self.ws["cand_i"][q]
        return row[row != FILL32].astype(np.int64)


# ------------------------------------------------------------------------------------------------ stage 1: the fold, image by image
@pytest.mark.parametrize("P,t", pr.PAIRS)
def test_stage1_lists_exactly_the_images_with_t_passing_rows(ops, monkeypatch, P, t):
    """One slice at the pinned threshold thr0: the images read back from the workspace contain every image with at least t rows
    that must pass the reference's row test and no image with fewer than t rows that may pass; for q* every planted image -- exactly
    t - 1, t, t + 1 high tokens at varying positions, all, none -- is listed iff it holds at least t; the result is the contract's."""
    fmt, lo = ("fp16" if (P + t) % 2 else "bf16"), bool(t % 2)
    set_lo(monkeypatch, lo)
    c = pr.planted_case(P, t, fmt, lo)
    s = TopSearch(ops, fmt, c["tw"], c["qn"], c["xw"], c["xn"], c["k"], "min", t, c["thr0"], OFFSET)
    assert s.guards_ok and not s.redo.any()
    must_in, must_out = pr.image_classes(c, c["thr0"])
    lists = [s.candidates(q) for q in range(s.Q)]
    for q, l in enumerate(lists):
        assert len(l) == 0 or (l.min() >= 0 and l.max() < s.N), q
        assert len(set(l.tolist())) == len(l), (q, "an image is listed twice")
    r = sr.check_sandwich(lists, must_in, must_out)
    assert r is None, r
    have = np.zeros(c["N"], dtype=bool)
    have[lists[pr.QSTAR]] = True
    planted = c["highs"] >= 0
    assert np.array_equal(have[planted], (c["highs"] >= t)[planted]), np.flatnonzero(planted & (have != (c["highs"] >= t)))[:8]
    print("TOPT-STAGE1", dict(P=P, t=t, fmt=fmt, lo=lo, k=c["k"], N=c["N"], must_in=int(must_in.sum()), must_out=int(must_out.sum()),
                              pairs=int(must_in.size), listed=sum(len(l) for l in lists)))
    ref_s, ref_i = tr.tsr.topk_of_scores(c["combined"], c["k"], OFFSET)
    assert np.array_equal(s.out_i, ref_i) and np.array_equal(sr.f32bits(s.out_s), sr.f32bits(ref_s))


# ------------------------------------------------------------------------------------------------ the whole search, public API
def _both(q, bank, k, combine, top_t, select=None, weights=None):
    """((scores, indices, stats) of the resident bank, ... of the plain one: the grouped route)."""
    from sky_embeddings_amd import search
    qd, xd = torch.from_numpy(q).cuda(), bank.cuda()
    wd = None if weights is None else torch.from_numpy(weights).cuda()
    out = []
    for tb in (search.TokenBank.resident(xd, wd), search.TokenBank(xd, wd)):
        sel = None if select is None else search.Selection(torch.from_numpy(select).cuda())
        stats = {}
        s, i = search.cosine_topk_tokens(qd, tb, k, combine, stats=stats, top_t=top_t, select=sel)
        out.append((s, i, stats))
    return out


def _assert_same(got, ref):
    assert torch.equal(got[1], ref[1]), (got[2], torch.nonzero(got[1] != ref[1])[:5].tolist())
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)), got[2]
    assert ref[2]["path"] == "tokens"


FULL = [(P, t, ("fp16", "bf16")[n % 2], bool((n // 2) % 2), (1, 100, 256)[n % 3]) for n, (P, t) in enumerate(pr.PAIRS)]
FULL += [(16, 2, "bf16", True, 256), (16, 15, "fp16", False, 100), (64, 9, "fp16", True, 1), (4, 2, "bf16", False, 256)]   # each dtype x variant


@pytest.mark.parametrize("P,t,dt,lo,k", FULL, ids=lambda v: str(v))
def test_full_search_is_bit_equal_to_the_grouped_route(monkeypatch, P, t, dt, lo, k):
    """Q = 256 random queries over a random bank of 2240 rows: scores and indices bit for bit the grouped route's, path 'prefiltered',
    top_t in the stats, and NO query re-run."""
    set_lo(monkeypatch, lo)
    N = 2240 // P
    k = min(k, N)
    q, bank, _ = pr.random_bank(P, 128, DT[dt], seed=100 * P + t)
    assert bank.shape[0] == N
    got, ref = _both(q, bank, k, "min", t)
    print("TOPT-FULL", dict(P=P, t=t, dt=dt, lo=lo, k=k), got[2])
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["combine"] == "min" and got[2]["top_t"] == t and ref[2]["top_t"] == t
    assert got[2]["redone"] == 0, got[2]


@pytest.mark.parametrize("P,t,dt", [(16, 4, "fp16"), (32, 3, "bf16"), (4, 2, "bf16"), (64, 16, "fp16")])
def test_max_under_top_t_is_the_plain_max(P, t, dt):
    q, bank, _ = pr.random_bank(P, 128, DT[dt], seed=5 + P)
    got, ref = _both(q, bank, 10, "max", t)
    plain, _ = _both(q, bank, 10, "max", None)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] == 0 and got[2]["top_t"] == t
    assert torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32)) and torch.equal(got[1], plain[1])


@pytest.mark.parametrize("P,t,dt,lo,kind", [(16, 2, "fp16", False, "random"), (16, 15, "bf16", True, "runs"), (4, 2, "bf16", False, "random"),
                                            (32, 3, "fp16", True, "runs"), (64, 9, "bf16", False, "random"), (8, 1, "fp16", False, "runs")])
def test_full_search_under_a_selection(monkeypatch, P, t, dt, lo, kind):
    """A random ~10 % selection and one in whole-tile runs, over a bank ten times the smallest (the selected images must themselves be
    a bank the route takes): bit for bit the grouped route under the same selection, no re-run, every index selected."""
    set_lo(monkeypatch, lo)
    rng = np.random.default_rng(31 * P + t)
    q, bank, _ = pr.random_bank(P, 128, DT[dt], seed=7 * P + t, rows=2240 * 11)
    N = bank.shape[0]
    ipt = 256 // P
    if kind == "random":
        flags = rng.random(N) < 0.1
        flags[rng.permutation(N)[:-(-2048 // P) + 4]] = True            # never fewer than the route's 2048 rows
    else:
        flags = np.zeros(N, dtype=bool)
        for t0 in (3, 4, 5, 40, 41, 42, 60, 61, 62, 63, N // ipt):         # whole tiles, in runs; the last one is the tail tile
            flags[t0 * ipt:(t0 + 1) * ipt] = True
    k = min(100, int(flags.sum()))
    got, ref = _both(q, bank, k, "min", t, select=flags)
    print("TOPT-SEL", dict(P=P, t=t, dt=dt, lo=lo, kind=kind, k=k), got[2])
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["top_t"] == t and got[2]["selected"] == int(flags.sum()), got[2]
    assert got[2]["redone"] == 0, got[2]
    idx = got[1].cpu().numpy()
    assert flags[idx[idx >= 0]].all()


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("P,t", [(4, 2), (16, 5), (64, 9)])
def test_d160_is_held_to_the_cpu_contract(ops, P, t, dt):
    """D = 160 has no grouped route (its kernels need D % 64 == 0): the library call against tests/token_topt_reference.py."""
    from oracle import similarity_oracle as so
    q, bank, xw = pr.random_bank(P, 160, DT[dt], seed=11 * P + t, Q=40)
    tw, qn = so.prep_queries_np(q, None)
    with np.errstate(all="ignore"):
        xn = so.wnorms_np(np.ascontiguousarray(xw.reshape(-1, 160)))
    k = min(10, xw.shape[0])
    s = TopSearch(ops, dt, tw, qn, xw, xn, k, "min", t, None, OFFSET)
    ref_s, ref_i = ttr.topk_tokens_top(q, xw, k, "min", t, idx_offset=OFFSET)
    assert s.guards_ok and not s.redo.any()
    assert np.array_equal(s.out_i, ref_i) and np.array_equal(sr.f32bits(s.out_s), sr.f32bits(ref_s))


# ------------------------------------------------------------------------------------------------------------------- edge banks
def _edge_bank(P, rng, N, D=128):
    return (rng.standard_normal((N, 1, D)) + 0.7 * rng.standard_normal((N, P, D))).astype(np.float32)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("P,t", [(4, 2), (16, 5), (32, 16), (64, 3)])
def test_hostile_banks_are_decided_exactly(P, t, dt):
    """NaN tokens that leave fewer than t finite scores (and exactly t), all-zero rows and rows of mixed-sign zeros so that +-0 ties
    reach d[t-1], an inf element in an image whose other rows fail, duplicate images (ties: the lower image first): bit for bit the
    grouped route."""
    rng = np.random.default_rng(1000 + P + t)
    N, Q, k = 2240 // P + 200, 256, 12
    q = rng.standard_normal((Q, 128), dtype=np.float32)
    x = _edge_bank(P, rng, N)
    x[10, :P - t + 1] = np.nan                  # t - 1 finite scores: -inf, never returned
    x[11, :P - t] = np.nan                      # exactly t finite scores
    x[12] = np.nan
    x[13, 0, 5] = np.nan
    for i in (20, 21, 22):                      # zero rows: their scores are +-0 (the sign of 0 * tw summed), t or more of them per image
        x[i, :t + (i - 21)] = 0.0
    x[23] = 0.0
    x[24] = 0.0
    x[24, :, ::2] = -0.0                        # rows of mixed-sign zeros
    x[25, :t] = 0.0
    x[25, :t, 1::3] = -0.0
    x[30] = -np.abs(x[30]) * np.sign(q[0])[None, :]     # every row far below query 0's threshold ...
    x[30, P // 2, 7] = np.inf                           # ... but one row the bound gives up on
    x[44] = q[7][None, :] * (1.0 + 0.05 * rng.standard_normal((P, 128))).astype(np.float32)    # query 7's best image ...
    x[40:44] = x[44]                            # ... six times, one of them at the far end of the bank
    x[N - 1] = x[44]
    bank = torch.from_numpy(x).to(DT[dt])
    got, ref = _both(q, bank, k, "min", t)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered", got[2]
    flat = got[1].flatten().tolist()
    assert 10 not in flat and 12 not in flat
    assert got[1][7, :6].tolist() == [40, 41, 42, 43, 44, N - 1]          # an exact tie: image ascending
    print("TOPT-EDGE", dict(P=P, t=t, dt=dt), got[2])


@pytest.mark.parametrize("P,t", [(8, 3), (32, 5)])
def test_fewer_eligible_images_than_k(P, t):
    """All but 7 images hold P - t + 1 NaN tokens (fewer than t finite scores): the tail of every result is (-inf, -1)."""
    rng = np.random.default_rng(77 + P)
    N, k = 2240 // P + 8, 20
    x = _edge_bank(P, rng, N)
    keep = rng.permutation(N)[:7]
    gone = np.ones(N, dtype=bool)
    gone[keep] = False
    x[gone, :P - t + 1] = np.nan                # t - 1 finite scores are left: d[t-1] = -inf
    q = rng.standard_normal((256, 128), dtype=np.float32)
    got, ref = _both(q, torch.from_numpy(x).to(torch.float16), k, "min", t)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered"
    assert (got[1][:, 7:] == -1).all() and torch.isinf(got[0][:, 7:]).all() and (got[1][:, :7] >= 0).all()
    assert set(got[1][0, :7].tolist()) == set(keep.tolist())


def test_a_flat_bank_overflows_the_list_and_is_re_run():
    """10 000 images whose tokens are copies of query 3: more candidates than its list holds.  The query is flagged, re-run by the
    grouped route under the same top_t, and the result is still bit-equal (ties to the lower image)."""
    rng = np.random.default_rng(13)
    N, P, t, k = 12000, 4, 2, 9
    q = rng.standard_normal((256, 128), dtype=np.float32)
    x = rng.standard_normal((N, P, 128), dtype=np.float32)
    x[1000:11000] = q[3]
    got, ref = _both(q, torch.from_numpy(x).to(torch.float16), k, "min", t)
    _assert_same(got, ref)
    assert got[2]["path"] == "prefiltered" and got[2]["redone"] >= 1 and got[2]["top_t"] == t, got[2]
    assert got[1][3].tolist() == list(range(1000, 1000 + k))
