"""GPU: the two-stage many-query search over a RESIDENT bf16 bank -- ``cosine_topk(queries, PreparedBank.resident(bank_bf16), k)``.

The stored bank is the fp32 bank its elements widen to: the oracle is ``oracle.similarity_oracle.cosine_topk_np`` on
``bank_bf16.float().numpy()``, and scores and indices must be bit-equal.  The 16-bit bank is always made on the CPU by torch's
``tensor.to(torch.bfloat16)`` (round to nearest even, overflow to inf, subnormals kept)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import similarity_oracle as so
from tests import prefilter_select_reference as psr

VARIANTS = [pytest.param("0", id="hi"), pytest.param("1", id="hi+lo")]


def _bf16(x):
    """numpy fp32 -> (the bf16 tensor on the CPU, the fp32 array it widens to)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    return t, t.float().numpy()


def _search(q, bank, w, k, idx_offset=0, **kw):
    """(scores, indices, stats) of cosine_topk over PreparedBank.resident(bf16 bank); bank a CPU or device bf16 tensor."""
    from sky_embeddings_amd import search
    stats = {}
    pb = search.PreparedBank.resident(bank.cuda(), None if w is None else torch.from_numpy(w).cuda(), idx_offset)
    assert pb.dtype == torch.bfloat16
    s, i = search.cosine_topk(torch.from_numpy(q).cuda(), pb, k, stats=stats, **kw)
    return s.cpu().numpy(), i.cpu().numpy(), stats


def _assert_equal(got, ref, stats=None):
    (s, i), (ref_s, ref_i) = got[:2], ref
    assert np.array_equal(i, ref_i), (stats, np.argwhere(i != ref_i)[:5])
    assert np.array_equal(s.view(np.uint32), ref_s.view(np.uint32)), stats


CASES = [(64, 2048, 128, 10, True),        # no tail tile
         (130, 21000, 128, 100, True),     # tail of 8 rows
         (17, 2049, 768, 100, True),       # tail of 1 row
         (33, 5119, 128, 7, False),        # tail of 255 rows
         (77, 9000, 192, 150, True)]


@functools.lru_cache(maxsize=None)
def _case(Q, N, D, k, weighted):
    """Inputs of one bit-exact case + the oracle's answer, computed once for the hi-only and the hi + lo run: the inputs of
    test_prefilter_lp_gpu._case, the bank rounded to bf16."""
    rng = np.random.default_rng(Q * 7 + N)
    q = rng.standard_normal((Q, D), dtype=np.float32)
    _, x = _bf16(rng.standard_normal((N, D)) * rng.uniform(0.2, 5.0, size=(N, 1)))   # rows of very different scale
    sc0 = so.cosine_scores_np(q[:1], x, None)[0]
    best = np.argsort(-sc0)[:3]
    x[N - 1], x[N // 2 + 1], x[7] = x[best[0]], x[best[1]], x[best[2]]      # exact ties: lower index first
    w = None
    if weighted:
        w = (1.0 / (rng.random(D, dtype=np.float32) + 0.05) ** 2).astype(np.float32)   # weights spread over 2.5 decades
        w /= w.sum()
    bank, x = _bf16(x)                                                     # (already bf16 values: exact)
    return q, bank, w, so.cosine_topk_np(q, x, k, w)


@pytest.mark.parametrize("lo", VARIANTS)
@pytest.mark.parametrize("Q,N,D,k,weighted", CASES)
def test_resident_bf16_bank_two_stage_topk_is_bit_exact(Q, N, D, k, weighted, lo, monkeypatch):
    """Ragged query tiles, every kind of last bank tile (none, 1, 8, 255 rows), k up to 150, planted exact ties; one bf16 query
    pass (SKYEMB_PREFILTER_LO=0) and two (=1).  The cap on re-run queries is a condition: under the hi-only bf16 eps_a the rows
    whose upper bound reaches the k-th best lower bound number at most 17, 139, 144, 12 and 192 per query in these five cases,
    against a re-score quota of 256 (fewer under hi + lo)."""
    monkeypatch.setenv("SKYEMB_PREFILTER_LO", lo)
    q, bank, w, ref = _case(Q, N, D, k, weighted)
    s, i, stats = _search(q, bank, w, k)
    print(stats)
    _assert_equal((s, i), ref, stats)
    assert stats["path"] == "prefiltered" and stats["redone"] <= Q // 10, stats


def test_rows_the_bound_cannot_hold_and_bf16_ties_are_decided_exactly():
    """The fp16 test of this name plus two rows: a NaN row, a row with an inf element, a zero row, a zero query, 600 near-copies of
    one query's best row that collapse to ties in bf16 (more candidates than the re-score quota: that query is flagged and re-run
    by the token search), a row with an element of 1e+35 (its weighted norm overflows: it scores +-0 for every query) and a row of
    nothing but 1e-38-scale elements aligned with query 0.  That row's weighted norm underflows to 0, so the contract scores it
    dot / eps, about 1e-32 for query 0: positive, but far below the 0.3 of the best ordinary rows -- the oracle does not rank it
    first, whatever its direction (test_rows_of_bf16_subnormals_are_not_lost has the banks in which such rows are on top).  Both
    rows are outside the window of the stage-1 bound and ride through every query's candidate list."""
    rng = np.random.default_rng(5)
    Q, N, D, k = 96, 12000, 128, 60
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = rng.standard_normal((N, D), dtype=np.float32)
    x[1000:1600] = q[3] + 1e-5 * rng.standard_normal((600, D)).astype(np.float32)
    x[50] = np.nan
    x[51, 7] = np.inf
    x[52] = 0.0
    q[20] = 0.0
    x[53, 11] = 1e+35
    w = rng.random(D, dtype=np.float32) + 0.1
    w /= w.sum()
    x[54] = 1e-38 * np.sign(q[0])
    bank, xw = _bf16(x)
    assert (xw[1000:1600] == xw[1000]).mean() > 0.9              # bf16 left them a few last-place steps apart: tied scores
    assert np.abs(xw[54]).max() < 2.0 ** -125 and np.abs(xw[54]).min() > 0 and xw[53, 11] > 2.0 ** 115
    ref = so.cosine_topk_np(q, xw, k, w)
    sc0 = so.cosine_scores_np(q[:1], xw, w)[0]
    assert 0 < sc0[54] < 1e-30 and sc0[53] == 0 and ref[0][0, k - 1] > 0.1, (sc0[53], sc0[54], ref[0][0, k - 1])
    s, i, stats = _search(q, bank, w, k)
    _assert_equal((s, i), ref, stats)
    assert stats["path"] == "prefiltered" and stats["redone"] >= 1, stats


@pytest.mark.parametrize("kind", ["anti-aligned", "ordinary"])
def test_rows_of_bf16_subnormals_are_not_lost(kind):
    """Two rows whose elements are ALL bf16 subnormals (|x| ~ 3e-39 and 5e-39), aligned with query 0, belong at the top of its
    list.  The rows are not rescaled, so a matrix core that flushes subnormals multiplies zeros: such rows are outside the window
    of the bound and must be kept for every query by their row constants.  Their weighted norm underflows to 0, so they score
    dot / eps, a positive number around 1e-31 -- not the 0.9 of the fp16 test's rows, whose norms survive: among unrelated random
    rows the oracle ranks them about 3000th, so the fp16 test's 'ordinary' bank cannot be copied as it is.  'anti-aligned': every
    other score of query 0 is negative (the bank of the fp32 test of denormal-scale rows), the planted rows are first and second.
    'ordinary': random rows; three of them score above 0.08 for query 0 and stay, every other row that scores >= 0 for it is
    negated, so the planted rows are fourth and fifth of k = 5, right behind scores 10^29 times theirs -- a lost row would show."""
    rng = np.random.default_rng(17)
    Q, N, D, k = 40, 6000, 128, 5
    base = rng.standard_normal(D).astype(np.float32)
    q = (base + 0.3 * rng.standard_normal((Q, D))).astype(np.float32)
    if kind == "anti-aligned":
        x = -np.abs(rng.uniform(0.5, 2.0, size=(N, 1))) * base + 0.3 * rng.standard_normal((N, D))
    else:
        _, x = _bf16(rng.standard_normal((N, D)))
        sc0 = so.cosine_scores_np(q[:1], x, None)[0]
        keep = np.argsort(-sc0)[:3]                                        # three rows stay above the planted ones for query 0;
        flip = sc0 >= 0                                                    # every other row that scores >= 0 is negated (exact in
        flip[keep] = False                                                 # bf16, and the chain's score changes sign exactly)
        x[flip] *= -1.0
    x = x.astype(np.float32)
    x[123] = q[0] / np.abs(q[0]).max() * 5e-39
    x[4567] = q[0] / np.abs(q[0]).max() * 3e-39
    bank, xw = _bf16(x)
    for r in (123, 4567):
        a = np.abs(xw[r].astype(np.float64))
        assert a.max() < 2.0 ** -126 and (a > 0).sum() > D // 2            # bf16 subnormals
    ref = so.cosine_topk_np(q, xw, k, None)
    top = 0 if kind == "anti-aligned" else 3
    assert ref[1][0, top:top + 2].tolist() == [123, 4567] and ref[0][0, top + 1] > 0, (ref[1][0], ref[0][0])
    if kind == "anti-aligned":
        assert (ref[0][0] < 0).sum() >= k - 2
    else:
        assert ref[0][0, 2] > 0.08 and k == 5                              # ordinary scores above them; both planted rows inside the top k
    s, i, stats = _search(q, bank, None, k)
    _assert_equal((s, i), ref, stats)
    assert stats["path"] == "prefiltered"


@pytest.mark.parametrize("N", [2049, 2303, 4096])
def test_no_tile_reads_past_the_last_row(N):
    """The bank is the first N rows of one larger allocation whose next 256 rows are copies of the queries: a tile read past row N
    would score 1.0 and come back as an index >= N.  Everything stays inside one allocation."""
    rng = np.random.default_rng(N)
    Q, D, k = 40, 128, 10
    q = rng.standard_normal((Q, D), dtype=np.float32)
    big = rng.standard_normal((N + 256, D), dtype=np.float32)
    big[N:] = q[np.arange(256) % Q]
    big_t, big_w = _bf16(big)
    w = rng.random(D, dtype=np.float32) + 0.1
    w /= w.sum()
    big_d = big_t.cuda()
    bank = big_d[:N]
    assert bank.is_contiguous() and bank.data_ptr() == big_d.data_ptr()
    s, i, stats = _search(q, bank, w, k)
    assert int(i.max()) < N and int(i.min()) >= 0, stats
    _assert_equal((s, i), so.cosine_topk_np(q, big_w[:N], k, w), stats)
    assert stats["path"] == "prefiltered"


def test_sharded_bf16_bank_merge_equals_whole_bank():
    """Two PreparedBank.resident(bf16) shards (ragged sizes, idx_offset) + ops.topk_merge == the whole bank == the oracle."""
    from sky_embeddings_amd import ops, search
    rng = np.random.default_rng(3)
    Q, N, D, k = 50, 12000, 128, 12
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = rng.standard_normal((N, D), dtype=np.float32)
    x[9000] = x[100]
    bank, xw = _bf16(x)
    qd, xd = torch.from_numpy(q).cuda(), bank.cuda()
    st = {}
    whole_s, whole_i = search.cosine_topk(qd, search.PreparedBank.resident(xd), k, stats=st)
    assert st["path"] == "prefiltered"
    parts = []
    for lo, hi in ((0, 6100), (6100, N)):
        st = {}
        parts.append(search.cosine_topk(qd, search.PreparedBank.resident(xd[lo:hi], None, idx_offset=lo), k, stats=st))
        assert st["path"] == "prefiltered"
    gs = torch.stack([p[0] for p in parts], dim=1).contiguous()
    gi = torch.stack([p[1] for p in parts], dim=1).contiguous()
    out_s, out_i = torch.empty(Q, k, device="cuda"), torch.empty(Q, k, device="cuda", dtype=torch.int64)
    ops.topk_merge(gs, gi, Q, 2, k, out_s, out_i)
    assert torch.equal(out_i, whole_i) and torch.equal(out_s, whole_s)
    _assert_equal((out_s.cpu().numpy(), out_i.cpu().numpy()), so.cosine_topk_np(q, xw, k, None))


@functools.lru_cache(maxsize=None)
def _select_base():
    """One bank of 21 000 x 128 (82 whole tiles and a tail of 8 rows), 130 queries, weights, and the unselected oracle answer."""
    Q, N, D, k = 130, 21000, 128, 100
    q, bank, w, ref = _case(Q, N, D, k, True)
    return q, bank, bank.float().numpy(), w, k, ref


SELECTIONS = ["all", "random10", "runs", "few_tiles", "none"]


def _flags(name, N):
    rng = np.random.default_rng(len(name))
    if name == "all":
        return np.ones(N, bool)
    if name == "random10":
        return rng.random(N) < 0.1
    if name == "runs":                      # whole tiles emptied: tiles 0-9, every third tile after that, and the tail tile
        f = rng.random(N) < 0.6
        t = np.arange(N) // 256
        f[(t < 10) | (t % 3 == 0) | (t == N // 256)] = False
        return f
    if name == "few_tiles":                 # 5 live whole tiles + the live tail: fewer than 8 -> the token route
        f = np.zeros(N, bool)
        for t in (3, 17, 40, 41, 80):
            f[t * 256 + 5:t * 256 + 200] = True
        f[N - 3:] = True
        return f
    return np.zeros(N, bool)


@pytest.mark.parametrize("name", SELECTIONS)
def test_search_under_a_selection(name):
    """Each result equals the oracle on bank[select], indices mapped back; all-True equals the unselected search; a selection
    with fewer than 8 live whole tiles takes the token route; none selected: all (-inf, -1)."""
    from sky_embeddings_amd import search
    q, bank, xw, w, k, ref_all = _select_base()
    N = xw.shape[0]
    flags = _flags(name, N)
    pb = search.PreparedBank.resident(bank.cuda(), torch.from_numpy(w).cuda())
    stats = {}
    s, i = search.cosine_topk(torch.from_numpy(q).cuda(), pb, k, stats=stats, select=torch.from_numpy(flags))
    got = (s.cpu().numpy(), i.cpu().numpy())
    print(name, stats)
    _assert_equal(got, psr.topk_select(q, xw, k, flags, w), stats)
    assert stats["selected"] == int(flags.sum())
    if name == "few_tiles":
        assert stats["path"] == "tokens" and stats["tiles"] == (6, 83), stats
    else:
        assert stats["path"] == "prefiltered" and stats["redone"] <= q.shape[0] // 10, stats
    if name == "all":
        _assert_equal(got, ref_all, stats)
        s0, i0 = search.cosine_topk(torch.from_numpy(q).cuda(), pb, k)
        assert torch.equal(s0, s) and torch.equal(i0, i)
    if name == "runs":
        assert stats["tiles"][0] < 60 and stats["tiles"][1] == 83, stats
    if name == "none":
        assert (got[1] == -1).all() and np.isneginf(got[0]).all()


def test_routes_and_refusals(monkeypatch):
    """Q = 16, k = 200, N = 2047 and SKYEMB_TOPK_PREFILTER=0 take the token route with the bare tensor's bits; [Q, D] weights are
    a ValueError; PreparedBank.resident(fp16) gives what PreparedBank(fp16) gives."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(23)
    Q, N, D, k = 40, 5000, 128, 9
    q = rng.standard_normal((Q, D), dtype=np.float32)
    bank, xw = _bf16(rng.standard_normal((N, D), dtype=np.float32))
    w = rng.random(D, dtype=np.float32) + 0.1
    w /= w.sum()
    qd, xd, wd = torch.from_numpy(q).cuda(), bank.cuda(), torch.from_numpy(w).cuda()
    pb = search.PreparedBank.resident(xd, wd)
    assert pb.dtype == torch.bfloat16 and pb.sample(64)[0].dtype == torch.bfloat16

    st = {}
    s2, i2 = search.cosine_topk(qd, pb, k, stats=st)
    assert st["path"] == "prefiltered" and "redone" in st
    _assert_equal((s2.cpu().numpy(), i2.cpu().numpy()), so.cosine_topk_np(q, xw, k, w), st)

    bare = {}
    sb, ib = search.cosine_topk(qd, xd, k, weights=wd, stats=bare)
    assert bare["path"] == "tokens"                          # a bare bf16 tensor keeps its route
    assert torch.equal(sb, s2) and torch.equal(ib, i2)

    st = {}
    s16, i16 = search.cosine_topk(qd[:16], pb, k, stats=st)            # Q = 16
    assert st["path"] == "tokens"
    sb16, ib16 = search.cosine_topk(qd[:16], xd, k, weights=wd)
    assert torch.equal(s16, sb16) and torch.equal(i16, ib16)

    st = {}
    s200, i200 = search.cosine_topk(qd, pb, 200, stats=st)             # k = 200 > 192
    assert st["path"] == "tokens"
    sb200, ib200 = search.cosine_topk(qd, xd, 200, weights=wd)
    assert torch.equal(s200, sb200) and torch.equal(i200, ib200)

    st = {}
    small = search.PreparedBank.resident(xd[:2047], wd)                # N = 2047 < 2048
    ss, si = search.cosine_topk(qd, small, k, stats=st)
    assert st["path"] == "tokens"
    sbs, ibs = search.cosine_topk(qd, xd[:2047], k, weights=wd)
    assert torch.equal(ss, sbs) and torch.equal(si, ibs)

    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    st = {}
    s0, i0 = search.cosine_topk(qd, pb, k, stats=st)
    assert st["path"] == "tokens" and torch.equal(s0, sb) and torch.equal(i0, ib)
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER")

    with pytest.raises(ValueError, match=r"per-query weights \[Q, D\]"):
        search.cosine_topk(qd, pb, k, weights=wd.expand(Q, D).contiguous())

    x16 = xd.to(torch.float16)
    a, b = search.PreparedBank.resident(x16, wd), search.PreparedBank(x16, wd)
    assert type(a) is type(b) and a.dtype == b.dtype == torch.float16 and a.bank.data_ptr() == b.bank.data_ptr()
    assert torch.equal(a.norms, b.norms)
    ra, rb = search.cosine_topk(qd, a, k), search.cosine_topk(qd, b, k)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])


def test_no_second_image_of_the_bank_is_kept():
    """PreparedBank.resident(bf16) + a search keep the norms (4 B per row), rowp (16 B per row) and one 256 x D tile alive with the
    bank: about 0.8 MB against a 30.7 MB bank.  A second 16-bit image of the bank would be 100 %, an fp32 copy 200 %."""
    from sky_embeddings_amd import search
    N, D = 20000, 768
    bank = torch.randn(N, D, device="cuda").to(torch.bfloat16)
    q = torch.randn(20, D, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    pb = search.PreparedBank.resident(bank)
    st = {}
    s, i = search.cosine_topk(q, pb, 10, stats=st)
    assert st["path"] == "prefiltered"
    del s, i
    bank16, rowp = pb.half_image()
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    print(f"grown {grown} bytes, bank {bank.numel() * 2} bytes")
    assert bank16.data_ptr() == bank.data_ptr() and pb.tail_tile.shape == (256, D) and pb.tail_tile.dtype == torch.bfloat16
    want = N * 4 + rowp.numel() * 4 + 256 * D * 2
    assert want <= grown <= want + 64 * 1024 and grown < 0.10 * bank.numel() * 2
