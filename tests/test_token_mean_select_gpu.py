"""GPU: combine 'mean' under a selection of images on the two-stage route (Selection.prepare_mean: stage 1 over the compacted pooled
image, stage 2 through the map) is bit for bit the grouped route under the same flags; the gather kernel is bit for bit
tests/token_mean_select_reference.py; what was not asked for stays where it was."""
import functools

import numpy as np
import pytest
import torch

from sky_embeddings_amd import ops, search
from tests import prefilter_gpu_harness as h
from tests import token_mean_select_reference as ref
from tests import token_search_reference as tsr
from tests.test_token_mean_prefilter_gpu import no_staging_list_fills

pytestmark = pytest.mark.gpu
T16 = h.TORCH16
N, S_TAIL = 4400, 2048 + 37


@pytest.fixture(autouse=True)
def _small_q(monkeypatch):
    monkeypatch.setattr(search, "TOKEN_MEAN_SELECT_PREFILTER_MIN_Q", 17)
    monkeypatch.setattr(search, "TOKEN_MEAN_PREFILTER_MIN_Q", 17)
    monkeypatch.setattr(search, "TOKEN_PREFILTER_MIN_Q", 17)


def flags_of(n, s, seed=0):
    """Exactly s of n images, scattered."""
    f = torch.zeros(n, dtype=torch.bool)
    f[torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:s]] = True
    return f.to(h.DEV)


@functools.lru_cache(maxsize=4)
def random_case(fmt, n, P, D, Q=257, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * P + D)
    bank = torch.randn(n, P, D, generator=g).to(T16[fmt]).to(h.DEV)
    q = torch.randn(Q, D, generator=g).to(h.DEV)
    w = (torch.rand(D, generator=g) + 0.1).to(h.DEV)
    return bank, q, w


def both(q, bank, k, flags, w=None, idx_offset=0, tb=None, sel=None):
    """(two-stage result and stats, grouped result under the same flags) over the same bank."""
    tb = search.TokenBank.resident(bank, w, idx_offset) if tb is None else tb
    sel = search.Selection(flags).prepare_mean(tb) if sel is None else sel
    st, ref_st = {}, {}
    got = search.cosine_topk_tokens(q, tb, k, "mean", stats=st, select=sel)
    want = search.cosine_topk_tokens(q, search.TokenBank(bank, tb.weights, idx_offset), k, "mean", stats=ref_st, select=flags)
    assert ref_st["path"] == "tokens"
    return got, st, want


def assert_equal(got, want):
    assert torch.equal(got[1], want[1]), "image indices differ from the grouped route"
    assert torch.equal(got[0], want[0]), "scores differ from the grouped route"


@pytest.mark.parametrize("fmt", ("fp16", "bf16"))
@pytest.mark.parametrize("S", (S_TAIL, 2048))
def test_gather_per_element(fmt, S):
    """skyemb_token_mean_select_gather through the C ABI into guarded buffers: every bit of every output, nothing outside them."""
    D = 128
    rng = np.random.default_rng(S)
    bits = rng.integers(0, 1 << 16, (N, D), dtype=np.uint16)       # any bit pattern, NaN and inf among them: rows are copied, not read
    rows_n = ref.rowp_rows(N)
    rowp = rng.standard_normal((rows_n, 4)).astype(np.float32)
    rowp[N:] = ref.SENTINEL
    rowp[::97] = (0, np.inf, 1, 0)                                 # unboundable images keep their constants
    idx = np.sort(rng.choice(N, S, replace=False))
    idx[0], idx[-1] = 0, N - 1                                     # the bank's first and last image
    idx = np.unique(idx)
    idx = np.concatenate([idx, np.setdiff1d(np.arange(N), idx)[:S - idx.shape[0]]])
    idx = np.sort(idx)
    assert idx.shape[0] == S
    L = ops.lib()
    rows_s = L.skyemb_bank16_rowp_rows(S)
    assert rows_s == ref.rowp_rows(S)
    pooled_d = h.dev(bits.view(np.int16)).view(T16[fmt])
    rowp_d, idx_d = h.dev(rowp), h.dev(idx)
    ps, rs, tail, cmap = h.Guarded(S * D * 2), h.Guarded(rows_s * 16), h.Guarded(256 * D * 2), h.Guarded(S * 4)
    rc = L.skyemb_token_mean_select_gather(h.ptr(pooled_d), h.ptr(rowp_d), h.ptr(idx_d), N, S, D, ops.dtype_code(T16[fmt]), ps.ptr(), rs.ptr(),
                                           tail.ptr(), cmap.ptr(), h.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.skyemb_last_error()
    assert ps.intact() and rs.intact() and tail.intact() and cmap.intact()
    want_ps, want_rs, want_tail, want_map = ref.gather(bits, rowp, idx)
    assert np.array_equal(ps.np(np.uint16, S, D), want_ps)
    assert ref.same_bits(rs.np(np.float32, rows_s, 4), want_rs)
    assert np.array_equal(cmap.np(np.int32, S), want_map)
    if S % 256:
        assert np.array_equal(tail.np(np.uint16, 256, D), want_tail)
    else:
        assert want_tail is None and tail.untouched()
    # the wrapper returns the same
    got = ops.token_mean_select_gather(pooled_d, rowp_d, idx_d)
    assert np.array_equal(h.patterns16(got[0]), want_ps) and ref.same_bits(got[2].cpu().numpy(), want_rs)
    assert np.array_equal(got[3].cpu().numpy(), want_map) and (got[1] is None) == (S % 256 == 0)


@pytest.mark.parametrize("fmt", ("fp16", "bf16"))
@pytest.mark.parametrize("P", (1, 4, 16, 64))
def test_bit_equal_to_the_grouped_route(fmt, P):
    bank, q, w = random_case(fmt, N, P, 128)
    flags = flags_of(N, S_TAIL, seed=P)
    idx = torch.nonzero(flags).squeeze(1)
    # the CPU statement of stage 1 over the selected images' pooled rows (they are the bank stage 1 walks): no list can fill, so
    # redone == 0 is required below and a re-run cannot hide a failure
    fits, worst = no_staging_list_fills(bank.index_select(0, idx).contiguous(), q, w, fmt, 10)
    assert fits, f"the CPU statement lets a staging list fill ({worst} pairs in one item): pick other inputs"
    got, st, want = both(q, bank, 10, flags, w)
    assert st["path"] == "prefiltered" and st["combine"] == "mean" and st["redone"] == 0, st
    assert st["selected"] == S_TAIL and st["compacted"] == (S_TAIL, N) and "tiles" not in st
    assert_equal(got, want)
    assert bool(flags[got[1].flatten()].all())


def abi_search(bank, q, w, k, idx, eps=1e-6):
    """The route through the library calls alone, without a floor: (scores, indices, redo) as numpy."""
    tb = search.TokenBank(bank, w)
    tw, qn = search.prepare_queries(q, tb.weights)
    pooled, _, rowp = ops.token_mean_pool(bank, tb.norms)
    comp = ops.token_mean_select_gather(pooled, rowp, idx)
    Q = q.shape[0]
    out_s = torch.empty(Q, k, device=h.DEV)
    out_i = torch.empty(Q, k, device=h.DEV, dtype=torch.int64)
    redo = torch.empty(Q, device=h.DEV, dtype=torch.int32)
    ops.cosine_topk_tokens_mean_prefiltered_sel(tw, qn, bank, tb.norms, *comp, k, eps, 0, out_s, out_i, redo)
    return out_s.cpu().numpy(), out_i.cpu().numpy(), redo.cpu().numpy()


@pytest.mark.parametrize("fmt", ("fp16", "bf16"))
def test_d160_against_the_contract(fmt):
    """The grouped kernels take D % 64 == 0 only: at D = 160 the route runs through the library calls and is held to the contract
    the grouped route is itself pinned to bit for bit (tests/token_search_reference.py), restricted to the selected images."""
    bank, q, w = random_case(fmt, N, 4, 160)
    flags = flags_of(N, S_TAIL, seed=160)
    idx = torch.nonzero(flags).squeeze(1)
    sc = tsr.combined_scores(q.cpu().numpy(), bank.float().cpu().numpy(), "mean", w.cpu().numpy())[:, idx.cpu().numpy()]
    fits, worst = no_staging_list_fills(bank.index_select(0, idx).contiguous(), q, w, fmt, 1, contract=sc)
    assert fits, f"the CPU statement lets a staging list fill ({worst} pairs in one item): pick other inputs"
    for k in (1, 100, 256):
        want_s, pos = tsr.topk_of_scores(sc, k)
        want_i = idx.cpu().numpy()[pos]                            # (every query has k finite scores here: no -1)
        got_s, got_i, redo = abi_search(bank, q, w, k, idx)
        assert not redo.any()
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s)


@pytest.mark.parametrize("fmt", ("fp16", "bf16"))
def test_deselected_images_cannot_matter(fmt):
    bank, q, w = random_case(fmt, N, 4, 128, Q=40, seed=5)
    flags = flags_of(N, S_TAIL, seed=5)
    off = torch.nonzero(~flags).squeeze(1)
    dirty = bank.clone()
    dirty[off[0::3], 1, 3] = float("nan")
    dirty[off[1::3], 2] = float("inf")
    dirty[off[2::3]] = 6e4
    got_clean, st_clean, want = both(q, bank, 10, flags, w)
    assert st_clean["path"] == "prefiltered"
    assert_equal(got_clean, want)
    tb = search.TokenBank.resident(dirty, w)
    st = {}
    got = search.cosine_topk_tokens(q, tb, 10, "mean", stats=st, select=search.Selection(flags).prepare_mean(tb))
    assert st == st_clean, (st, st_clean)                          # the same route, the same number of re-runs
    assert_equal(got, got_clean)


@pytest.mark.parametrize("fmt", ("fp16", "bf16"))
def test_nan_and_unboundable_selected_images_and_idx_offset(fmt):
    P, D, Q, k = 4, 128, 33, 20
    bank, q, w = random_case(fmt, N, P, D, Q=Q, seed=9)
    bank = bank.clone()
    flags = flags_of(N, S_TAIL, seed=9)
    on = torch.nonzero(flags).squeeze(1).tolist()
    a, b = on[10], on[500]
    for j, i in enumerate((a, b)):                                 # images made of query j itself: its best by far
        bank[i] = (q[j] / w.sqrt()).to(T16[fmt])[None, :].expand(P, D)
    bank[a, 1, 3] = float("nan")                                   # a NaN token: the image scores -inf
    bank[b, 0] = 0                                                 # an all-zero token: norm 0, the image cannot be bounded
    tb = search.TokenBank.resident(bank, w, 1000)
    sel = search.Selection(flags).prepare_mean(tb)
    rowp_sel, cmap = sel.mean_prefilter(tb)[2].cpu().numpy(), sel.mean_prefilter(tb)[3].cpu().numpy()
    for i in (a, b):
        assert (rowp_sel[np.searchsorted(cmap, i)] == np.array([0, np.inf, 1, 0], np.float32)).all()
    got, st, want = both(q, bank, k, flags, w, idx_offset=1000, tb=tb, sel=sel)
    assert st["path"] == "prefiltered"
    assert_equal(got, want)
    assert 1000 + a not in got[1][0].tolist()                      # never returned
    assert 1000 + b in got[1][1].tolist()                          # decided exactly: still among query 1's best
    valid = got[1][got[1] >= 0]
    assert int(valid.min()) >= 1000 and bool(flags[valid - 1000].all())


@pytest.mark.parametrize("fmt", ("fp16", "bf16"))
def test_duplicates_on_both_sides_of_the_selection(fmt):
    P, D, Q = 4, 128, 40
    g = torch.Generator().manual_seed(3)
    base = torch.randn(300, P, D, generator=g).to(T16[fmt])
    bank = base.repeat(15, 1, 1)[:N].contiguous().to(h.DEV)        # image i comes back at 300 + i, 600 + i, ...: exact ties everywhere
    q = (base[:Q, 0].float() + 0.5 * torch.randn(Q, D, generator=g)).to(h.DEV)
    flags = flags_of(N, S_TAIL, seed=3)
    for k in (7, 100):
        got, st, want = both(q, bank, k, flags)
        assert st["path"] == "prefiltered"
        assert_equal(got, want)
        s, i = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert flags.cpu().numpy()[i].all()                        # deselected twins are absent
        tie = s[:, 1:] == s[:, :-1]
        assert tie.any() and (i[:, 1:][tie] > i[:, :-1][tie]).all()     # ties come out image-ascending


def test_a_full_list_is_rerun_and_still_equal():
    g = torch.Generator().manual_seed(4)
    one = torch.randn(1, 4, 128, generator=g).to(torch.float16)
    bank = one.repeat(6000, 1, 1).contiguous().to(h.DEV)           # identical images: every pair passes, every staging list fills
    q = torch.randn(40, 128, generator=g).to(h.DEV)
    got, st, want = both(q, bank, 10, flags_of(6000, 4352, seed=4))
    assert st["path"] == "prefiltered" and st["redone"] > 0, st
    assert_equal(got, want)


def test_set_weights_rebuilds_the_entry():
    bank, q, w = random_case("bf16", N, 4, 128, Q=40)
    flags = flags_of(N, S_TAIL, seed=1)
    tb = search.TokenBank.resident(bank, w)
    sel = search.Selection(flags)
    assert sel.prepare_mean(tb) is sel
    kept = sel._mean[tb]
    got, st, want = both(q, bank, 10, flags, tb=tb, sel=sel)
    assert st["path"] == "prefiltered" and sel._mean[tb] is kept   # repeated searches do not gather again
    assert_equal(got, want)
    w2 = torch.rand(128, device=h.DEV) + 0.1
    tb.set_weights(w2)
    assert tb in sel._mean                                         # stale, not dropped: the Selection was asked once
    got, st, want = both(q, bank, 10, flags, tb=tb, sel=sel)
    assert st["path"] == "prefiltered"
    assert sel._mean[tb] is not kept and sel._mean[tb][0] == tb._version and sel._mean[tb][1] is tb.stage1_mean()
    assert_equal(got, want)


def test_a_selection_never_prepared_keeps_the_grouped_route():
    bank, q, w = random_case("fp16", N, 4, 128, Q=40)
    flags = flags_of(N, S_TAIL, seed=2)
    tb = search.TokenBank.resident(bank, w)
    plain = search.TokenBank(bank, w)
    sel = search.Selection(flags)
    for select in (sel, flags):
        st = {}
        got = search.cosine_topk_tokens(q, tb, 10, "mean", stats=st, select=select)
        assert st["path"] == "tokens" and "compacted" not in st
        assert_equal(got, search.cosine_topk_tokens(q, plain, 10, "mean", select=flags))
    assert sel._mean is None and tb._stage1_mean is None           # nothing pooled, nothing gathered
    # prepared for ANOTHER bank: still the grouped route over this one
    sel.prepare_mean(search.TokenBank.resident(bank.clone(), w))
    st = {}
    search.cosine_topk_tokens(q, tb, 10, "mean", stats=st, select=sel)
    assert st["path"] == "tokens" and tb._stage1_mean is None
    with pytest.raises(ValueError, match="TokenBank.resident"):
        sel.prepare_mean(plain)


def test_neighbouring_routes_are_untouched():
    bank, q, w = random_case("fp16", N, 4, 128, Q=40)
    flags = flags_of(N, S_TAIL, seed=2)
    tb, plain = search.TokenBank.resident(bank, w), search.TokenBank(bank, w)
    st = {}
    got = search.cosine_topk_tokens(q, tb, 10, "mean", stats=st)   # the unselected mean search
    assert st["path"] == "prefiltered" and "compacted" not in st and "selected" not in st
    assert_equal(got, search.cosine_topk_tokens(q, plain, 10, "mean"))
    st = {}
    sel = search.Selection(flags).prepare_mean(tb)                 # holding the compacted image changes nothing for min / max
    got = search.cosine_topk_tokens(q, tb, 10, "min", stats=st, select=sel)
    assert st["path"] == "prefiltered" and "tiles" in st and "compacted" not in st
    assert_equal(got, search.cosine_topk_tokens(q, plain, 10, "min", select=flags))
