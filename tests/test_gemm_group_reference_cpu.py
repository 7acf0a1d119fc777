"""CPU: tests/gemm_group_reference.py -- the case table of tests/test_gemm_group_elementwise_gpu.py reaches what it claims, the header
model walks every tile once and equals what skyemb_gemm_group_plan writes (the plan fills a host blob only: no device), the plan
refuses what it should with a message, and subtly wrong grouped launches driven through gemm_reference.emulate exceed the bar."""
import ctypes
import math

import pytest
import torch

from tests import gemm_group_reference as gg
from tests import gemm_reference as gr
from tests.gemm_group_reference import GROUP_CASES, GROUPED_TILES, MASKS, MIXED_TILES, RING_TILES, gid
from tests.gemm_reference import BF, F16, KC, RC, T256, Case

ORDERS = (None, "0", "1")


# ------------------------------------------------------------------------------------------------------------- coverage
def test_the_table_is_small_and_its_problems_differ():
    for gc in GROUP_CASES:
        P = gc.problems
        assert len(P) <= 6 or len(P) == gg.GROUP_MAX, gid(gc)
        assert len({(c.M, c.N, c.K) for c in P}) == len(P), (gid(gc), "two problems share (M, N, K)")
        assert len({c.K for c in P}) >= min(len(P), 3), (gid(gc), "per-problem K")
        for c in P:
            assert c.M <= 768 and c.N <= 768 and c.K <= 384 and c.split == 0 and not c.ws and c.tile == gc.tile and c.dtype == gc.dtype
    assert len(GROUP_CASES) <= 50


def test_the_table_reaches_every_tile_class_epilogue_and_order():
    seen = {(gc.dtype, gc.tile, gg.class_mask(gc.problems)) for gc in GROUP_CASES}
    for dt in (BF, F16):
        for tile in GROUPED_TILES:
            for mask in MASKS[tile]:
                assert (dt, tile, mask) in seen, (dt, tile, mask)
    assert all(gg.class_mask(gc.problems) in MASKS[gc.tile] for gc in GROUP_CASES)
    epis = {c.epi for gc in GROUP_CASES for c in gc.problems}
    assert epis >= {"plain", "colsum", "colsum16", "gelu", "full", "dgelu", "resid"}
    # outputs of the weight-gradient groups: out_f32 with ldo32 > N + colsum_a, colsum16, plain out_f32
    for gc in GROUP_CASES:
        if gc.name == "wgrad":
            assert {c.epi for c in gc.problems} == {"plain", "colsum", "colsum16"}
            assert all(gg.lds(c)["ldo32"] > c.N and gg.lds(c)["ldo"] > c.N for c in gc.problems)
    # both tile orders per tile family, in both formats
    for dt in (BF, F16):
        ring = {gg.order_on(gc.tile, gc.order) for gc in GROUP_CASES if gc.dtype == dt and gc.tile != T256}
        big = {gg.order_on(gc.tile, gc.order) for gc in GROUP_CASES if gc.dtype == dt and gc.tile == T256}
        assert ring == {False, True} and big == {False, True}
        for tile in GROUPED_TILES:
            assert {gg.order_on(tile, gc.order) for gc in GROUP_CASES if (gc.dtype, gc.tile, gc.name) == (dt, tile, "wgrad")} == {False, True}
    assert any(len(gc.problems) == gg.GROUP_MAX for gc in GROUP_CASES)
    hints = [gc for gc in GROUP_CASES if gc.hint]
    assert hints and all(gc.hint % 16 != 0 and gc.hint % 4 == 0 for gc in hints)


def test_weight_gradient_groups_hold_the_four_hostile_shapes():
    for gc in GROUP_CASES:
        if gc.name != "wgrad":
            continue
        bm, bn = gr.TILES[gc.tile][:2]
        nt = [gg.ntiles(c, gc.tile) for c in gc.problems]
        assert max(nt) >= 9 and any(n % 8 for n in nt), gid(gc)
        assert any(c.M % bm == 0 and c.N % bn == 0 for c in gc.problems)
        if gc.tile != T256:
            assert any(c.M < bm and c.N < bn for c in gc.problems)
            assert any(c.M % bm and c.N % bn and c.M > bm for c in gc.problems)
            ks = [c.K for c in gc.problems]
            assert all(k % 128 == 0 for k in ks) if gc.tile == 9128128 else sorted(ks) == [64, 128, 192, 320]
        else:
            assert all(c.M % 256 == 0 and c.N % 256 == 0 and c.K >= 128 for c in gc.problems)


def test_padding_and_eighths_that_cross_a_problem_border():
    """Groups with padding workgroups; groups (order on) whose total / 8 is a multiple of no problem's tile count (problems of one tile
    aside: 1 divides everything); and what that is for: an XCD's eighth of the slots that holds slots / real tiles of two problems."""
    padded = literal = slots = real = 0
    for gc in GROUP_CASES:
        h = gg.header(gc.tile, gc.problems, gc.order)
        nt = [gg.ntiles(c, gc.tile) for c in gc.problems]
        padded += sum(nt) < h["total"]
        if not h["on"]:
            continue
        e = h["total"] >> 3
        literal += all(e % n for n in nt if n > 1)
        for x in range(8):
            owners = [gg.lookup(g, h["starts"], h["n"]) for g in range(x * e, (x + 1) * e)]
            slots += len({p for p, _ in owners}) > 1
            real += len({p for p, tb in owners if tb < nt[p]}) > 1
    print("padded", padded, "total / 8 multiple of no tile count", literal, "eighths over two problems' slots", slots, "... real tiles", real)
    assert padded >= 10 and literal >= 4 and slots >= 10 and real >= 4


# ------------------------------------------------------------------------------------------------------------- the walk
@pytest.mark.parametrize("gc", GROUP_CASES, ids=gid)
def test_the_walk_visits_every_real_tile_once_and_no_padding_slot(gc):
    want = sorted((p, tb) for p, c in enumerate(gc.problems) for tb in range(gg.ntiles(c, gc.tile)))
    h = gg.header(gc.tile, gc.problems, None)
    assert h["total"] % 8 == 0 and all(s % 8 == 0 for s in h["starts"])
    for on in (False, True):
        w = gg.walk(gc.tile, gc.problems, on)
        assert len(w) == h["total"]
        assert sorted(x for x in w if x is not None) == want, (gid(gc), on)
        assert sorted(gg.slot_to_tile(b, h["total"], on) for b in range(h["total"])) == list(range(h["total"]))
        # ... and a padding slot is one: it lies between a problem's last tile and the next problem's first slot
        for b, x in enumerate(w):
            if x is None:
                p, tb = gg.lookup(gg.slot_to_tile(b, h["total"], on), h["starts"], h["n"])
                assert gg.ntiles(gc.problems[p], gc.tile) <= tb < h["starts"][p + 1] - h["starts"][p]


# ------------------------------------------------------------------------------------------------------------- the plan
def _lib():
    from sky_embeddings_amd import _lib as L
    return L, L.lib()


def plan_args(L, c, ptr=0x10000, **over):
    """skyemb_gemm_args of problem c with dummy 16-byte-aligned pointers (the plan reads no memory behind them)."""
    ld = gg.lds(c)
    g = L.GemmArgs()
    g.A, g.B, g.lda, g.ldb = ptr, ptr + 0x100, ld["lda"], ld["ldb"]
    g.a_layout, g.b_layout = (L.KC if c.al == KC else L.RC), (L.KC if c.bl == KC else L.RC)
    g.M, g.N, g.K = c.M, c.N, c.K
    g.dtype = L.BF16 if c.dtype == BF else L.F16
    g.alpha = 0.5 if gg.has(c, "alpha") else 1.0
    g.ldo32, g.ldo, g.ldo2 = c.N, c.N, c.N
    for name, field, ldf in (("bias", "bias", None), ("table", "table", "ldt"), ("table", "tab_row", None), ("dst", "dst_row", None),
                             ("resid", "resid", "ldr"), ("aux", "aux", "ldaux"), ("out_f32", "out_f32", "ldo32"), ("out", "out", "ldo"),
                             ("out2", "out2", "ldo2"), ("colsum", "colsum_a", None)):
        if gg.has(c, name):
            setattr(g, field, ptr + 0x200)
            if ldf:
                setattr(g, ldf, ld[ldf])
    g.act = {"gelu": L.ACT_GELU, "dgelu": L.ACT_DGELU}.get(c.epi, L.ACT_NONE)
    for k, v in over.items():
        setattr(g, k, v)
    return g


def plan(L, lib, args, tile, short=0):
    n = len(args)
    arr = (L.GemmArgs * max(n, 1))(*args)
    nbytes = lib.skyemb_gemm_group_blob_bytes(n)
    blob = (ctypes.c_int32 * ((nbytes + 3) // 4 + 64))()
    info = L.GemmGroupInfo()
    rc = lib.skyemb_gemm_group_plan(arr, n, tile, ctypes.cast(blob, ctypes.c_void_p), nbytes - short, ctypes.byref(info))
    msg = lib.skyemb_last_error()
    return rc, info, list(blob), (msg.decode() if msg else "")


def check_header(L, lib, tile_arg, tile, problems, order):
    rc, info, words, msg = plan(L, lib, [plan_args(L, c) for c in problems], tile_arg)
    assert rc == 0, msg
    h = gg.header(tile, problems, order)
    n = h["n"]
    assert words[0] == n and words[1] == h["word1"], (words[:2], h)
    assert words[8:8 + n + 1] == h["starts"] and not any(words[8 + n + 1:8 + gg.GROUP_MAX + 1])
    assert (info.total_blocks, info.tile, info.class_mask, info.reserved & 4) == (h["total"], tile, h["mask"], 4 if h["f16"] else 0)
    assert info.reserved & 3 == 0 and words[2] == 0 and words[3] == 0 and words[41] == 0          # no side jobs, no optimiser


@pytest.fixture(scope="module")
def planner():
    try:
        L, lib = _lib()
    except Exception as e:   # the library is not built / cannot be loaded on this machine
        pytest.skip(f"libskyemb cannot be loaded here: {e}")
    return L, lib


def test_the_plan_writes_the_modelled_header(planner, monkeypatch):
    L, lib = planner
    for gc in GROUP_CASES:
        for order in ORDERS:
            if order is None:
                monkeypatch.delenv("SKYEMB_GROUP_XCD_ORDER", raising=False)
            else:
                monkeypatch.setenv("SKYEMB_GROUP_XCD_ORDER", order)
            check_header(L, lib, gc.tile, gc.tile, gc.problems, order)
    monkeypatch.delenv("SKYEMB_GROUP_XCD_ORDER", raising=False)
    # tile = 0: either side of group_tile's thresholds (320 tiles of 128 x 64, 400 of 128 x 128; 160..256 whole 256 x 256 tiles at K >= 2048)
    wg = lambda m, n, k=128: Case(BF, 0, RC, RC, m, n, k, "plain")
    sweep = (([wg(128 * 11, 64 * 29)], 64064), ([wg(128 * 16, 64 * 20)], 128064), ([wg(128 * 8, 64 * 20), wg(128 * 8 - 8, 64 * 20 - 8, 64)], 128064),
             ([wg(128 * 8, 64 * 20), wg(128 * 7, 64 * 20, 64)], 64064), ([wg(128 * 21, 128 * 19)], 128064), ([wg(128 * 20, 128 * 20)], 128128),
             ([wg(128 * 20, 128 * 20 - 8)], 128128), ([wg(128 * 19, 128 * 21 - 8, 64), wg(8, 8)], 128128),
             ([wg(256 * 13, 256 * 13, 2048)], T256), ([wg(256 * 16, 256 * 16, 2048)], T256), ([wg(256 * 16, 256 * 16, 2048), wg(256, 256, 2048)], 128128),
             ([wg(256 * 12, 256 * 13, 2048), wg(256, 768, 4096)], 128128), ([wg(256 * 12, 256 * 13, 2048), wg(512, 512, 4096)], T256),
             ([wg(256 * 13, 256 * 13, 1984)], 128128), ([wg(256 * 13, 256 * 13 + 8, 2048)], 128128))
    for problems, want in sweep:
        assert gg.chosen_tile(problems) == want, (problems, want)
        check_header(L, lib, 0, want, problems, None)


def test_the_plan_refuses_with_a_message(planner, monkeypatch):
    L, lib = planner
    monkeypatch.delenv("SKYEMB_GROUP_XCD_ORDER", raising=False)
    ok = Case(BF, 64064, RC, RC, 72, 56, 128, "colsum")
    P = lambda al, bl, **kw: Case(BF, 64064, al, bl, 72, 56, 128, "plain")._replace(**kw)
    a = lambda c, **over: plan_args(L, c, **over)
    assert plan(L, lib, [a(ok)], 64064)[0] == 0
    refusals = {
        "n = 0": ([], 64064, 0, "problems"),
        "n = 33": ([a(ok)] * 33, 64064, 0, "problems"),
        "a blob one byte short": ([a(ok)], 64064, 1, "blob too small"),
        "mask 3": ([a(P(KC, KC)), a(P(KC, RC))], 64064, 0, "mix 3"),
        "mask 5": ([a(P(KC, KC)), a(P(RC, RC))], 64064, 0, "mix 5"),
        "mask 8": ([a(P(RC, KC))], 64064, 0, "mix 8"),
        "mask 12": ([a(P(RC, RC)), a(P(RC, KC))], 64064, 0, "mix 12"),
        "bf16 with fp16": ([a(ok), a(ok._replace(dtype=F16, M=80))], 64064, 0, "problem 1"),
        "K % 64": ([a(ok), a(ok), a(ok._replace(K=96))], 64064, 0, "problem 2"),
        "N % 8": ([a(P(KC, KC, N=60))], 64064, 0, "problem 0"),
        "odd k-tiles on 9128128": ([a(ok._replace(K=128)), a(ok._replace(K=192))], 9128128, 0, "K % 128"),
        "ragged on 256256": ([a(ok._replace(M=256, N=256)), a(ok._replace(M=264, N=256))], T256, 0, "whole tiles"),
        "K = 64 on 256256": ([a(ok._replace(M=256, N=256, K=64))], T256, 0, "whole tiles"),
        "a tile without GROUPED": ([a(ok)], 2256128, 0, "not built for grouped"),
        "an unknown tile": ([a(ok)], 777, 0, "not built for grouped"),
        "mask 6 on 9128128": ([a(P(KC, RC)), a(P(RC, RC, M=80))], 9128128, 0, "mix KC.RC with RC.RC"),
    }
    for what, (args, tile, short, text) in refusals.items():
        rc, info, _, msg = plan(L, lib, args, tile, short)
        assert rc != 0, what
        assert msg.startswith("skyemb_gemm_group_plan") and text in msg, (what, msg)


def test_a_plan_that_answers_0_names_a_built_launch(planner):
    """Every (tile, class mask) the plan accepts is one group_launch_tile has an instance for (gemm_pipe.hip: masks 1, 2, 4 with
    GROUPED, mask 6 with MIXED only); the GPU test launches each of them.  Mask 6 on 9128128 planned with rc 0 before and then failed
    to launch: the plan refuses it now."""
    L, lib = planner
    by_mask = {1: [(KC, KC)], 2: [(KC, RC)], 4: [(RC, RC)], 6: [(KC, RC), (RC, RC)]}
    for tile in GROUPED_TILES:
        for mask, classes in by_mask.items():
            m = 256 if tile == T256 else 72
            args = [plan_args(L, Case(BF, tile, al, bl, m + 256 * i, 256, 128, "plain")) for i, (al, bl) in enumerate(classes)]
            rc, info, _, msg = plan(L, lib, args, tile)
            assert (rc == 0) == (mask in MASKS[tile]), (tile, mask, rc, msg)
            if rc == 0:
                assert info.class_mask == mask and info.tile == tile
    assert set(MIXED_TILES) == {t for t in GROUPED_TILES if 6 in MASKS[t]} and set(RING_TILES) == {t for t in GROUPED_TILES if 1 in MASKS[t]}


# ------------------------------------------------------------------------------------------------------------- mutants
@pytest.fixture(scope="module")
def emulated():
    """Per case: operands, fp64 statement, emulated problems (shared by the tests below; not modified)."""
    out = {}
    for gc in GROUP_CASES:
        ts = [gg.inputs(gc, j) for j in range(len(gc.problems))]
        sts = [gg.reference(c, t) for c, t in zip(gc.problems, ts)]
        full = [gg.emulate(c, t) for c, t in zip(gc.problems, ts)]
        out[gid(gc)] = (ts, sts, full)
    return out


def test_the_emulated_launch_is_inside_the_bar_under_both_orders(emulated):
    for gc in GROUP_CASES:
        ts, sts, full = emulated[gid(gc)]
        a = gg.run_group(gc, ts, False, full=full)
        b = gg.run_group(gc, ts, True, full=full)
        r = gg.worst_ratio(gc, a, sts)
        assert r <= 1.0, (gid(gc), r)
        for ma, mb in zip(a, b):
            for name in ma:
                assert torch.equal(torch.nan_to_num(ma[name], nan=-7.0), torch.nan_to_num(mb[name], nan=-7.0)), (gid(gc), name)


@pytest.mark.parametrize("mutant", gg.GROUP_MUTANTS)
def test_a_subtly_wrong_launch_exceeds_the_bar(emulated, mutant):
    caught = []
    for gc in GROUP_CASES:
        ts, sts, full = emulated[gid(gc)]
        r = gg.worst_ratio(gc, gg.run_group(gc, ts, gg.order_on(gc.tile, gc.order), mutant, full=full), sts)
        if not r <= 1.0:
            caught.append((gid(gc), r))
    print(mutant, len(caught), "of", len(GROUP_CASES), caught[:4])
    assert caught, mutant
    if mutant in ("prev_args", "other_k"):
        # one wrong tile lands orders of magnitude off its bar (the contrast between problems), not a few bars
        assert max(r for _, r in caught) > 100.0 or any(math.isinf(r) for _, r in caught)
        assert len(caught) >= len(GROUP_CASES) // 2


def test_the_slot_map_applied_twice_is_a_permutation():
    """Why xcd_twice is defined on the tile index inside a problem: on the launch's slots the map is a bijection, so is its square,
    and every tile is still computed once -- no result can tell."""
    for total in (8, 40, 64, 256):
        twice = sorted(gg.slot_to_tile(gg.slot_to_tile(b, total, True), total, True) for b in range(total))
        assert twice == list(range(total))


# ------------------------------------------------------------------------------------------------------------- single launches
def test_few_problems_lack_a_single_launch_of_the_same_tile():
    refused = [(gid(gc), j) for gc in GROUP_CASES for j in gg.single_refused(gc)]
    total = sum(len(gc.problems) for gc in GROUP_CASES)
    print("no single launch of the group's tile:", refused)
    assert len(refused) * 4 <= total, (len(refused), total)
    for gc in GROUP_CASES:
        for j, c in enumerate(gc.problems):
            if j not in gg.single_refused(gc):
                counts = gr.planned(gg.base(c))["counts"]
                assert counts == {"fallback": 0, "pipe": int(gc.tile != T256), "tile256": int(gc.tile == T256), "splitk": 0}
