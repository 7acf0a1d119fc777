"""GPU parity of the exact similarity search, ELEMENT BY ELEMENT and route by route: skyemb_cosine_topk (the two streaming
instantiations and the three tiles), skyemb_cosine_scores, skyemb_cosine_sample_floor, skyemb_weighted_norms[_lp] and
skyemb_kth_largest_floor go through the C ABI (sky_embeddings_amd.ops) and every element the statement of
tests/exact_search_reference.py defines is held to the bits of the C oracle.  The cases are the smallest shapes that reach each
branch of the dispatch (tests/test_exact_search_reference_cpu.py pins the tables); each case prints the route it takes.

Every output lies inside a larger buffer: 64 guard elements on either side must come back unchanged, and the output itself
starts as a NaN payload (scores) or -7777 (indices), so that a slot the statement defines and the kernel skipped cannot pass.
The raw partial lists are checked before any merge (check_lists: the contract of include/skyemb.h for any cut of the bank;
check_ranges: each list against its own row range), then skyemb_topk_merge with and without `ws` against cosine_topk_np
restricted by the floor.  SKYEMB_TOPK_NW=4 and SKYEMB_TOPK_STREAM=0 are read once per process: two child processes run the
many-query rows on the 64 x 128 tile and the Q <= 16 rows on the 16-query tile."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import similarity_oracle as so
from tests import exact_search_reference as er
from tests.exact_search_reference import EPS, bits

DEV = "cuda"
PAD = 64
FILL_BITS, GUARD_BITS = 0x7FC01234, 0x7FC0BEEF           # two NaN payloads: the pre-fill of a score output, its guards
FILL_IDX, GUARD_IDX = -7777, 77
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    return load_ops()


def load_ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()
    return _ops


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(shape, dtype=torch.float32):
    """-> (pre-filled output of `shape`, its buffer with PAD guard elements on either side)."""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        raw = torch.full((n + 2 * PAD,), FILL_BITS, dtype=torch.int32, device=DEV)
        raw[:PAD] = GUARD_BITS
        raw[PAD + n:] = GUARD_BITS
        buf = raw.view(torch.float32)
    else:
        buf = torch.full((n + 2 * PAD,), FILL_IDX, dtype=dtype, device=DEV)
        buf[:PAD] = GUARD_IDX
        buf[PAD + n:] = GUARD_IDX
    return buf[PAD:PAD + n].view(*shape), buf


def raw_ints(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def guards_intact(*bufs):
    for buf in bufs:
        g = GUARD_BITS if buf.dtype == torch.float32 else GUARD_IDX
        r = raw_ints(buf)
        if not (bool((r[:PAD] == g).all()) and bool((r[-PAD:] == g).all())):
            return False
    return True


def untouched(*bufs):
    """Guards AND pre-fill as allocated: what a refused call must leave."""
    for buf in bufs:
        r = raw_ints(buf)[PAD:-PAD]
        if not bool((r == (FILL_BITS if buf.dtype == torch.float32 else FILL_IDX)).all()):
            return False
    return guards_intact(*bufs)


def same_bits(got, ref):
    g, r = bits(got.cpu().numpy()), bits(ref)
    if g.shape == r.shape and np.array_equal(g, r):
        return True
    at = np.argwhere(g != r) if g.shape == r.shape else []
    print(f"{len(at)} of {g.size} elements differ; first:", [(tuple(i), hex(g[tuple(i)] & 0xffffffff), hex(r[tuple(i)] & 0xffffffff)) for i in at[:8]])
    return False


def refused(ops, rc, text, *bufs):
    """A refusal: non-zero code, skyemb_last_error set by this call, nothing launched (the pre-filled outputs are as allocated)."""
    msg = ops.lib().skyemb_last_error()
    torch.cuda.synchronize()
    assert rc != 0 and msg and text in msg.decode(), (rc, msg)
    assert untouched(*bufs)


# ------------------------------------------------------------------------------------------------------------- top-k
def run_topk_case(ops, c, n, stream_on=True, nw4=False):
    name, lib_lists = er.route(c.Q, c.N, c.D, c.k, stream_on, nw4)
    assert name == c.route and lib_lists == ops.cosine_topk_chunks(c.N, c.Q, c.D, c.k), (c, name, lib_lists)
    L = c.nchunks if c.nchunks is not None else lib_lists
    q, x, w = er.search_data(c.Q, c.N, c.D, c.weighted, n)
    ref = so.cosine_scores_np(q, x, w, EPS)
    rs, ri = so.cosine_topk_np(q, x, c.k, w, EPS)
    tw, qn = so.prep_queries_np(q, w)
    tw_d, qn_d, x_d, xn_d = dev(tw), dev(qn), dev(x), dev(so.wnorms_np(x, w))
    thr, forms = er.make_floors(ref, c.k, n)
    ranges = er.list_ranges(name, c.N, L)
    print(f"{er.topk_id(c)}: route {name}, {L} lists ({sum(hi <= lo for lo, hi in ranges)} empty), floors {sorted(set(forms))}")
    for thr0 in (None, thr):
        ps, ps_b = guarded((c.Q, L, c.k))
        pi, pi_b = guarded((c.Q, L, c.k), torch.int64)
        ops.cosine_topk(tw_d, qn_d, x_d, xn_d, c.k, EPS, c.idx_offset, L, ps, pi, dev(thr0))
        torch.cuda.synchronize()
        assert guards_intact(ps_b, pi_b)
        hs, hi = ps.cpu().numpy(), pi.cpu().numpy()
        er.check_lists(hs, hi, ref, c.N, c.k, thr0, c.idx_offset)
        er.check_ranges(hs, hi, ref, c.k, thr0, c.idx_offset, ranges)
        es, ei = er.restrict_by_floor(rs, ri, thr0, c.idx_offset)
        for ws in (None, torch.zeros(c.Q, dtype=torch.int32, device=DEV)):
            ms, ms_b = guarded((c.Q, c.k))
            mi, mi_b = guarded((c.Q, c.k), torch.int64)
            ops.topk_merge(ps, pi, c.Q, L, c.k, ms, mi, ws)
            torch.cuda.synchronize()
            assert guards_intact(ms_b, mi_b) and same_bits(ms, es) and np.array_equal(mi.cpu().numpy(), ei), (er.topk_id(c), ws is not None)
    return name


@pytest.mark.parametrize("n", range(len(er.STREAM_CASES)), ids=[er.topk_id(c) for c in er.STREAM_CASES])
def test_streaming_topk(ops, n):
    assert run_topk_case(ops, er.STREAM_CASES[n], n) in ("stream8", "stream4")


@pytest.mark.parametrize("n", range(len(er.TILED_CASES)), ids=[er.topk_id(c) for c in er.TILED_CASES])
def test_tiled_topk(ops, n):
    assert run_topk_case(ops, er.TILED_CASES[n], n) in ("tile16", "tile64x256")


# ------------------------------------------------------------------------------------------------------------- refusals
def raw_topk(ops, tw, qn, x, xn, Q, N, D, k, nchunks, ps, pi):
    return ops.lib().skyemb_cosine_topk(tw.data_ptr(), qn.data_ptr(), x.data_ptr(), xn.data_ptr(), Q, N, D, k, EPS, 0, nchunks, None,
                                        ps.data_ptr(), pi.data_ptr(), torch.cuda.current_stream().cuda_stream)


def test_lds_cap_of_the_16_query_tile(ops):
    """launch_topk refuses what does not fit 160 KiB of LDS: the largest accepted k runs and is right, k + 1 launches nothing."""
    k = er.largest_k("tile16")
    assert run_topk_case(ops, er.TopkCase(1, 300, 4, k, True, 0, None, "tile16"), 0) == "tile16"
    tw, qn, x, xn = (torch.ones(s, device=DEV) for s in ((1, 4), (1,), (300, 4), (300,)))
    ps, ps_b = guarded((1, 1, k + 1))
    pi, pi_b = guarded((1, 1, k + 1), torch.int64)
    assert er.route(1, 300, 4, k + 1) == ("tile16", 1)
    refused(ops, raw_topk(ops, tw, qn, x, xn, 1, 300, 4, k + 1, 1, ps, pi), "of LDS", ps_b, pi_b)


def test_topk_refusals(ops):
    Q, N, D, k = 3, 300, 64, 5
    tw, qn, x, xn = (torch.ones(s, device=DEV) for s in ((Q, D), (Q,), (N, D), (N,)))
    lists = er.route(Q, N, D, k)[1]
    ps, ps_b = guarded((Q, lists + 1, k))
    pi, pi_b = guarded((Q, lists + 1, k), torch.int64)
    for bad in (1, lists - 1, lists + 1):                              # the streaming route takes the library's count only
        refused(ops, raw_topk(ops, tw, qn, x, xn, Q, N, D, k, bad, ps, pi), "nchunks must come from", ps_b, pi_b)
    refused(ops, raw_topk(ops, tw, qn, x, xn, Q, 2 ** 31, D, k, 1, ps, pi), "shard too large", ps_b, pi_b)
    refused(ops, raw_topk(ops, tw, qn, x, xn, 17, 2 ** 31, 100, k, 1, ps, pi), "shard too large", ps_b, pi_b)
    for D_bad in (6, 62, 1026):
        refused(ops, raw_topk(ops, tw, qn, x, xn, Q, 4, D_bad, k, 1, ps, pi), "bad shape", ps_b, pi_b)
    assert raw_topk(ops, tw, qn, x, xn, Q, N, D, k, lists, ps, pi) == 0    # and the same arguments with the right count run
    torch.cuda.synchronize()
    assert guards_intact(ps_b, pi_b) and not untouched(ps_b, pi_b)


# ------------------------------------------------------------------------------------------------------------- scores
def run_scores_case(ops, c, n, stream_on=True):
    assert er.scores_route(c.Q, c.N, c.D, stream_on) == c.route
    q, x, w = er.search_data(c.Q, c.N, c.D, c.weighted, 100 + n)
    ref = so.cosine_scores_np(q, x, w, EPS)
    tw, qn = so.prep_queries_np(q, w)
    out, out_b = guarded((c.Q, c.N))
    ops.cosine_scores(dev(tw), dev(qn), dev(x), dev(so.wnorms_np(x, w)), EPS, out)
    torch.cuda.synchronize()
    print(f"{er.score_id(c)}: route {c.route}")
    assert guards_intact(out_b) and same_bits(out, ref), er.score_id(c)
    return c.route


@pytest.mark.parametrize("n", range(len(er.SCORE_CASES)), ids=[er.score_id(c) for c in er.SCORE_CASES])
def test_cosine_scores(ops, n):
    run_scores_case(ops, er.SCORE_CASES[n], n)


# ------------------------------------------------------------------------------------------------------------- sample floor
@functools.lru_cache(maxsize=None)
def floor_data(Q, S):
    q, x, w = er.search_data(Q, S, er.FLOOR_D, True, S)
    tw, qn = so.prep_queries_np(q, w)
    return so.cosine_scores_np(q, x, w, EPS), dev(tw), dev(qn), dev(x), dev(so.wnorms_np(x, w))


@pytest.mark.parametrize("c", er.FLOOR_CASES, ids=er.floor_id)
def test_sample_floor(ops, c):
    Q, S, kk = c
    k, tiles = er.floor_k(S, kk), er.ceil_div(S, 16)
    ref, tw, qn, x, xn = floor_data(Q, S)
    assert ops.sample_floor_applicable(Q, S, er.FLOOR_D, k, tw, x)
    expect, _ = er.sample_floor_reference(ref, k)
    ws, ws_b = guarded((Q, tiles))
    out, out_b = guarded((Q,))
    ops.cosine_sample_floor(tw, qn, x, xn, k, EPS, ws, out)
    torch.cuda.synchronize()
    print(f"{er.floor_id(c)}: {tiles} tiles ({S % 16 or 16} rows in the last), k {k}")
    assert guards_intact(ws_b, out_b) and same_bits(out, expect), er.floor_id(c)


def raw_floor(ops, tw, qn, x, xn, Q, S, D, k, ws, out):
    return ops.lib().skyemb_cosine_sample_floor(tw.data_ptr(), qn.data_ptr(), x.data_ptr(), xn.data_ptr(), Q, S, D, k, EPS, ws.data_ptr(),
                                                out.data_ptr(), torch.cuda.current_stream().cuda_stream)


def test_sample_floor_refusals(ops):
    big = torch.ones(17 * (16 * 2048 + 1) * 4 + 8, device=DEV)             # room for every shape below; never read
    qn = xn = big
    ws, ws_b = guarded((17, 2049))
    out, out_b = guarded((17,))
    for Q, S, D, k in er.FLOOR_REFUSALS:
        assert not ops.sample_floor_applicable(Q, S, D, k, big)
        refused(ops, raw_floor(ops, big, qn, big, xn, Q, S, D, k, ws, out), "skyemb_cosine_sample_floor", ws_b, out_b)
    off4 = big[1:]                                                          # rows 4 bytes off a 16-byte boundary
    assert off4.data_ptr() % 16 == 4 and ops.sample_floor_applicable(4, 40, 64, 1, big) and not ops.sample_floor_applicable(4, 40, 64, 1, off4)
    refused(ops, raw_floor(ops, big, qn, off4, xn, 4, 40, 64, 1, ws, out), "16-byte aligned", ws_b, out_b)
    refused(ops, raw_floor(ops, off4, qn, big, xn, 4, 40, 64, 1, ws, out), "16-byte aligned", ws_b, out_b)


# ------------------------------------------------------------------------------------------------------------- weighted norms
def off4_copy(t):
    """The same values in storage that starts 4 bytes behind a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, device=DEV, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 4
    v.copy_(t)
    return v


@pytest.mark.parametrize("c", er.NORM_CASES, ids=er.norm_id)
def test_weighted_norms(ops, c):
    x, w = er.norm_data(c.N, c.D)
    w = w if c.has_w else None
    norms_ref, xw_ref = er.norms_reference(x, w)
    x_d = dev(x) if c.aligned else off4_copy(dev(x))
    norms, norms_b = guarded((c.N,))
    xw, xw_b = guarded((c.N, c.D))
    ops.weighted_norms(x_d, dev(w), norms, xw if c.has_out else None)
    torch.cuda.synchronize()
    print(f"{er.norm_id(c)}: route {c.route}")
    assert guards_intact(norms_b, xw_b) and same_bits(norms, norms_ref)
    assert same_bits(xw, xw_ref) if c.has_out else untouched(xw_b)


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=("f16", "bf16"))
@pytest.mark.parametrize("shape", er.NORM_SHAPES, ids=lambda s: "N%d-D%d" % s)
def test_weighted_norms_lp(ops, shape, dtype):
    """The 16-bit twin is the fp32 statement on the exactly widened rows (tests/test_lp_bank_cpu.py)."""
    x, w = er.norm_data(*shape)
    x16 = torch.from_numpy(x).to(dtype)
    for ww in (w, None):
        norms_ref = so.wnorms_np(x16.float().numpy(), ww)
        norms, norms_b = guarded((shape[0],))
        ops.weighted_norms_lp(x16.to(DEV), dev(ww), norms)
        torch.cuda.synchronize()
        assert guards_intact(norms_b) and same_bits(norms, norms_ref)


# ------------------------------------------------------------------------------------------------------------- k-th floor
@functools.lru_cache(maxsize=None)
def kth_inputs(S):
    x = er.kth_data(S)
    return x, dev(x)


@pytest.mark.parametrize("c", er.KTH_CASES, ids=er.kth_id)
def test_kth_largest_floor(ops, c):
    S, kk = c
    x, x_d = kth_inputs(S)
    k = er.kth_k(x, kk)
    out, out_b = guarded((len(er.KTH_ROWS),))
    ops.kth_largest_floor(x_d, k, out)
    torch.cuda.synchronize()
    print(f"{er.kth_id(c)}: route {er.kth_route(S)}, k {k}, rows {er.KTH_ROWS}")
    assert guards_intact(out_b) and same_bits(out, er.kth_reference(x, k)), er.kth_id(c)


# ------------------------------------------------------------------------------------------------------------- switches
def child_main(which):
    """Body of the two child processes; the first failing case ends the process with its traceback."""
    ops = load_ops()
    routes = set()
    if which == "nw4":
        for n, c in enumerate(er.NW4_CASES):
            routes.add(run_topk_case(ops, c, n, nw4=True))
    else:
        for n, c in enumerate(er.STREAM_OFF_CASES):
            routes.add(run_topk_case(ops, c, n, stream_on=False))
        for n, c in enumerate(er.SCORE_STREAM_OFF_CASES):
            routes.add(run_scores_case(ops, c, n, stream_on=False))
        Q, S, kk = er.FLOOR_CASES[2]                                        # the sample floor needs the streaming scorer: refused
        _, tw, qn, x, xn = floor_data(Q, S)
        ws, ws_b = guarded((Q, er.ceil_div(S, 16)))
        out, out_b = guarded((Q,))
        assert not ops.sample_floor_applicable(Q, S, er.FLOOR_D, 1, tw, x)
        refused(ops, raw_floor(ops, tw, qn, x, xn, Q, S, er.FLOOR_D, 1, ws, out), "SKYEMB_TOPK_STREAM", ws_b, out_b)
        routes.add("floor_refused")
    print("child ok:", which, " ".join(sorted(routes)))


def run_child(which, env):
    code = f"from tests import test_exact_search_elementwise_gpu as t; t.child_main({which!r})"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True,
                         text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    return out.stdout


def test_four_wave_many_query_tile_in_a_child_process():
    assert "child ok: nw4 tile64x128\n" in run_child("nw4", {"SKYEMB_TOPK_NW": "4"})


def test_streaming_kernels_switched_off_in_a_child_process():
    assert "child ok: stream_off floor_refused scores16 tile16\n" in run_child("stream_off", {"SKYEMB_TOPK_STREAM": "0"})
