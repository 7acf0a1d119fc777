"""GPU: the two-stage many-query search over a RESIDENT fp16 bank -- ``cosine_topk(queries, PreparedBank(bank_fp16), k)``.

The stored bank is the fp32 bank its elements widen to: the oracle is ``oracle.similarity_oracle.cosine_topk_np`` on
``x16.astype(np.float32)``, and scores and indices must be bit-equal.  The 16-bit bank is always made on the CPU by numpy's
``astype(np.float16)`` (round to nearest even, overflow to inf, subnormals kept)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import similarity_oracle as so


def _search(q, x16, w, k, **kw):
    """(scores, indices, stats) of cosine_topk over PreparedBank(fp16 bank); x16 a numpy fp16 array or a device tensor."""
    from sky_embeddings_amd import search
    bank = torch.from_numpy(x16).cuda() if isinstance(x16, np.ndarray) else x16
    stats = {}
    pb = search.PreparedBank(bank, None if w is None else torch.from_numpy(w).cuda())
    s, i = search.cosine_topk(torch.from_numpy(q).cuda(), pb, k, stats=stats, **kw)
    return s.cpu().numpy(), i.cpu().numpy(), stats


def _assert_equal(got, ref, stats=None):
    (s, i), (ref_s, ref_i) = got, ref
    assert np.array_equal(i, ref_i), (stats, np.argwhere(i != ref_i)[:5])
    assert np.array_equal(s.view(np.uint32), ref_s.view(np.uint32)), stats


CASES = [(64, 2048, 128, 10, True),        # no tail tile
         (130, 21000, 128, 100, True),     # tail of 8 rows
         (17, 2049, 768, 100, True),       # tail of 1 row
         (33, 5119, 128, 7, False),        # tail of 255 rows
         (77, 9000, 192, 150, True)]


@functools.lru_cache(maxsize=None)
def _case(Q, N, D, k, weighted):
    """Inputs of one bit-exact case + the oracle's answer, computed once for the hi-only and the hi + lo run."""
    rng = np.random.default_rng(Q * 7 + N)
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x16 = (rng.standard_normal((N, D)) * rng.uniform(0.2, 5.0, size=(N, 1))).astype(np.float32).astype(np.float16)   # rows of very different scale
    sc0 = so.cosine_scores_np(q[:1], x16.astype(np.float32), None)[0]
    best = np.argsort(-sc0)[:3]
    x16[N - 1], x16[N // 2 + 1], x16[7] = x16[best[0]], x16[best[1]], x16[best[2]]      # exact ties: lower index first
    w = None
    if weighted:
        w = (1.0 / (rng.random(D, dtype=np.float32) + 0.05) ** 2).astype(np.float32)   # weights spread over 2.5 decades
        w /= w.sum()
    return q, x16, w, so.cosine_topk_np(q, x16.astype(np.float32), k, w)


@pytest.mark.parametrize("lo", [False, True], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("Q,N,D,k,weighted", CASES)
def test_resident_fp16_bank_two_stage_topk_is_bit_exact(Q, N, D, k, weighted, lo, monkeypatch):
    """Ragged query tiles, every kind of last bank tile (none, 1, 8, 255 rows), k up to 150, planted exact ties; one fp16 query
    pass and two (SKYEMB_PREFILTER_LO=1).  The cap on re-run queries is the fp32 tests' on the same inputs: the intervals are
    no wider."""
    if lo:
        monkeypatch.setenv("SKYEMB_PREFILTER_LO", "1")
    q, x16, w, ref = _case(Q, N, D, k, weighted)
    s, i, stats = _search(q, x16, w, k)
    print(stats)
    _assert_equal((s, i), ref, stats)
    assert stats["path"] == "prefiltered" and stats["redone"] <= Q // 10, stats


def test_rows_the_bound_cannot_hold_and_fp16_ties_are_decided_exactly():
    """A NaN row, a row with an inf element, a zero row, a zero query, and 600 near-copies of one query's best row that collapse
    to ties in fp16: more candidates than the re-score quota, so that query is flagged and re-run by the token search."""
    rng = np.random.default_rng(5)
    Q, N, D, k = 96, 12000, 128, 60
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x = rng.standard_normal((N, D), dtype=np.float32)
    x[1000:1600] = q[3] + 1e-5 * rng.standard_normal((600, D)).astype(np.float32)
    x[50] = np.nan
    x[51, 7] = np.inf
    x[52] = 0.0
    q[20] = 0.0
    x16 = x.astype(np.float16)
    assert (x16[1000:1600] == x16[1000]).mean() > 0.9            # fp16 left them a few last-place steps apart: tied scores
    w = rng.random(D, dtype=np.float32) + 0.1
    w /= w.sum()
    s, i, stats = _search(q, x16, w, k)
    _assert_equal((s, i), so.cosine_topk_np(q, x16.astype(np.float32), k, w), stats)
    assert stats["path"] == "prefiltered" and stats["redone"] >= 1, stats


@pytest.mark.parametrize("kind", ["anti-aligned", "ordinary"])
def test_rows_of_fp16_subnormals_are_not_lost(kind):
    """Two rows whose elements are ALL fp16 subnormals (|x| ~ 3e-6), aligned with query 0, belong at the top of its list.  The
    rows are not rescaled, so a matrix core that flushes subnormals multiplies zeros: only the row's additive term keeps it a
    candidate.  'anti-aligned': every other score of query 0 is negative (the bank of the fp32 test of denormal-scale rows);
    'ordinary': the k-th best score is far above the plain bound of a zero dot product, so a lost row would show."""
    rng = np.random.default_rng(17)
    Q, N, D, k = 40, 6000, 128, 5
    base = rng.standard_normal(D).astype(np.float32)
    q = (base + 0.3 * rng.standard_normal((Q, D))).astype(np.float32)
    if kind == "anti-aligned":
        x = -np.abs(rng.uniform(0.5, 2.0, size=(N, 1))) * base + 0.3 * rng.standard_normal((N, D))
    else:
        x = rng.standard_normal((N, D))
    x16 = x.astype(np.float32).astype(np.float16)
    x16[123] = (q[0] / np.abs(q[0]).max() * 5e-6).astype(np.float16)
    x16[4567] = (q[0] / np.abs(q[0]).max() * 3e-6).astype(np.float16)
    for r in (123, 4567):
        a = np.abs(x16[r].astype(np.float64))
        assert a.max() < 2.0 ** -14 and (a > 0).sum() > D // 2
    ref = so.cosine_topk_np(q, x16.astype(np.float32), k, None)
    assert {123, 4567} == set(ref[1][0, :2].tolist()) and ref[0][0, 1] > 0.9
    if kind == "anti-aligned":
        assert (ref[0][0] < 0).sum() >= k - 2
    else:
        assert ref[0][0, k - 1] > 0.1
    s, i, stats = _search(q, x16, None, k)
    _assert_equal((s, i), ref, stats)
    assert stats["path"] == "prefiltered"


@pytest.mark.parametrize("N", [2049, 2303, 4096])
def test_no_tile_reads_past_the_last_row(N):
    """The bank is the first N rows of one larger allocation whose next 256 rows are copies of the queries: a tile read past row N
    would score 1.0 and come back as an index >= N.  Everything stays inside one allocation."""
    rng = np.random.default_rng(N)
    Q, D, k = 40, 128, 10
    q = rng.standard_normal((Q, D), dtype=np.float32)
    big = rng.standard_normal((N + 256, D), dtype=np.float32).astype(np.float16)
    big[N:] = q[np.arange(256) % Q].astype(np.float16)
    w = rng.random(D, dtype=np.float32) + 0.1
    w /= w.sum()
    big_d = torch.from_numpy(big).cuda()
    bank = big_d[:N]
    assert bank.is_contiguous() and bank.data_ptr() == big_d.data_ptr()
    s, i, stats = _search(q, bank, w, k)
    assert int(i.max()) < N and int(i.min()) >= 0, stats
    _assert_equal((s, i), so.cosine_topk_np(q, big[:N].astype(np.float32), k, w), stats)
    assert stats["path"] == "prefiltered"


def test_sharded_fp16_bank_merge_equals_whole_bank():
    """Two PreparedBank(fp16) shards (ragged sizes, idx_offset) + ops.topk_merge == the whole bank == the oracle."""
    from sky_embeddings_amd import ops, search
    rng = np.random.default_rng(3)
    Q, N, D, k = 50, 12000, 128, 12
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x16 = rng.standard_normal((N, D), dtype=np.float32).astype(np.float16)
    x16[9000] = x16[100]
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x16).cuda()
    st = {}
    whole_s, whole_i = search.cosine_topk(qd, search.PreparedBank(xd), k, stats=st)
    assert st["path"] == "prefiltered"
    parts = []
    for lo, hi in ((0, 6100), (6100, N)):
        st = {}
        parts.append(search.cosine_topk(qd, search.PreparedBank(xd[lo:hi], None, idx_offset=lo), k, stats=st))
        assert st["path"] == "prefiltered"
    gs = torch.stack([p[0] for p in parts], dim=1).contiguous()
    gi = torch.stack([p[1] for p in parts], dim=1).contiguous()
    out_s, out_i = torch.empty(Q, k, device="cuda"), torch.empty(Q, k, device="cuda", dtype=torch.int64)
    ops.topk_merge(gs, gi, Q, 2, k, out_s, out_i)
    assert torch.equal(out_i, whole_i) and torch.equal(out_s, whole_s)
    _assert_equal((out_s.cpu().numpy(), out_i.cpu().numpy()), so.cosine_topk_np(q, x16.astype(np.float32), k, None))


def test_routes_and_refusals(monkeypatch):
    """Q = 16 and SKYEMB_TOPK_PREFILTER=0 take the token route with the bare tensor's bits; a bare fp16 tensor keeps that route at
    any Q; an fp32 PreparedBank on the widened rows returns the two-stage route's bits; bf16 and a misaligned bank are refused."""
    from sky_embeddings_amd import search
    rng = np.random.default_rng(23)
    Q, N, D, k = 40, 5000, 128, 9
    q = rng.standard_normal((Q, D), dtype=np.float32)
    x16 = rng.standard_normal((N, D), dtype=np.float32).astype(np.float16)
    w = rng.random(D, dtype=np.float32) + 0.1
    w /= w.sum()
    qd, xd, wd = torch.from_numpy(q).cuda(), torch.from_numpy(x16).cuda(), torch.from_numpy(w).cuda()
    pb = search.PreparedBank(xd, wd)
    assert pb.dtype == torch.float16 and pb.sample(64)[0].dtype == torch.float16

    st = {}
    s2, i2 = search.cosine_topk(qd, pb, k, stats=st)
    assert st["path"] == "prefiltered" and "redone" in st
    _assert_equal((s2.cpu().numpy(), i2.cpu().numpy()), so.cosine_topk_np(q, x16.astype(np.float32), k, w), st)

    st32 = {}
    s32, i32 = search.cosine_topk(qd, search.PreparedBank(xd.float(), wd), k, stats=st32)
    assert st32["path"] == "prefiltered" and torch.equal(s32, s2) and torch.equal(i32, i2)

    bare = {}
    sb, ib = search.cosine_topk(qd, xd, k, weights=wd, stats=bare)
    assert bare["path"] == "tokens"                          # a bare fp16 tensor keeps its route
    assert torch.equal(sb, s2) and torch.equal(ib, i2)

    st = {}
    s16, i16 = search.cosine_topk(qd[:16], pb, k, stats=st)
    assert st["path"] == "tokens"
    sb16, ib16 = search.cosine_topk(qd[:16], xd, k, weights=wd)
    assert torch.equal(s16, sb16) and torch.equal(i16, ib16)

    monkeypatch.setenv("SKYEMB_TOPK_PREFILTER", "0")
    st = {}
    s0, i0 = search.cosine_topk(qd, pb, k, stats=st)
    assert st["path"] == "tokens" and torch.equal(s0, sb) and torch.equal(i0, ib)
    monkeypatch.delenv("SKYEMB_TOPK_PREFILTER")

    with pytest.raises(ValueError, match="bfloat16"):
        search.PreparedBank(xd.to(torch.bfloat16), wd)
    odd = torch.empty(N * D + 8, device="cuda", dtype=torch.float16)[4:4 + N * D].view(N, D)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        search.PreparedBank(odd, wd)


def test_no_second_image_of_the_bank_is_kept():
    """PreparedBank(fp16) + half_image() allocate the norms (4 B per row), rowp (16 B per row) and one 256 x D tile: about 0.8 MB
    against a 30.7 MB bank.  A second fp16 image of the bank (what an fp32 PreparedBank builds) would be 100 %."""
    from sky_embeddings_amd import search
    N, D = 20000, 768
    bank = torch.randn(N, D, device="cuda").to(torch.float16)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    pb = search.PreparedBank(bank)
    bank16, rowp = pb.half_image()
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    print(f"grown {grown} bytes, bank {bank.numel() * 2} bytes")
    assert bank16.data_ptr() == bank.data_ptr() and pb.tail_tile.shape == (256, D)
    assert 0 < grown < 0.10 * bank.numel() * 2
