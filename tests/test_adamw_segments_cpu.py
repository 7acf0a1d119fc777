"""CPU: the host side of the segmented AdamW launch -- skyemb_adamw_segments_plan against its restatement in
tests/adamw_segments_reference.py (byte for byte), the partition property of every table, every refusal with its text, the launch's
argument checks, the pure launch splitter beside PredictorOptimizer, and the mutants of the emulation (each must change the result
of every kernel case of tests/test_adamw_segments_gpu.py).  Shapes come from skyemb_adamw_segments_limits."""
import ctypes

import numpy as np
import pytest
import torch

from sky_embeddings_amd import _lib, ops
from sky_embeddings_amd.optim import segmented_launches
from tests import adamw_segments_reference as ar

MAX_GROUPS, CHUNK, MAX_GRID = ops.adamw_segments_limits()


def test_limits_and_struct_layouts():
    assert MAX_GROUPS >= 64 and MAX_GROUPS * ctypes.sizeof(_lib.AdamwGroup) + 128 <= 4096     # by value in HIP's 4 KB of arguments
    assert CHUNK > 0 and CHUNK % 4 == 0 and MAX_GRID > 0
    assert ctypes.sizeof(_lib.AdamwGroup) == 32 and _lib.AdamwGroup.decayed.offset == 28
    assert ctypes.sizeof(_lib.AdamwSegment) == 24 and _lib.AdamwSegment.group.offset == 16
    assert ops.ADAMW_WORK_DTYPE == ar.WORK and ar.WORK.itemsize == 16


def lengths_layout(lengths, groups, gap_after=()):
    segs, off = [], 0
    for k, n in enumerate(lengths):
        segs.append((off, n, groups[k % len(groups)]))
        off += n + (8 if k in gap_after else 0)
    return segs, off


VITB = ar.vitb_finetune_segments()
LAYOUTS = {
    "one-of-8": ([(0, 8, 0)], 1, 8),
    "reversed": (list(reversed(lengths_layout([8, 12, CHUNK, 16], [0, 1])[0])), 2, CHUNK + 36),
    "touching-same-group": ([(8, 12, 0), (20, CHUNK - 4, 0), (CHUNK + 16, 8, 0)], 1, CHUNK + 24),
    "touching-other-group": ([(8, 12, 0), (20, CHUNK - 4, 1), (CHUNK + 16, 8, 0)], 2, CHUNK + 24),
    "gaps": lengths_layout([8, 16, 24, 8], [2, 2, 0], gap_after=(0, 2))[:1] + (3, 80),
    "chunk-edges": lengths_layout([CHUNK - 4, CHUNK, CHUNK + 4, 3 * CHUNK + 8], [0, 1, 2, 3], gap_after=(0, 1, 2))[:1] + (4, 6 * CHUNK + 40),
    "chunk-edges-joined": lengths_layout([CHUNK - 4, CHUNK, CHUNK + 4, 3 * CHUNK + 8], [0])[:1] + (1, 6 * CHUNK + 8),
    "kernel-case": ar.kernel_layout(CHUNK)[:1] + (len(ar.GROUPS), ar.kernel_layout(CHUNK)[1]),
    "vit-b-finetune": (VITB[0], len(VITB[1]), VITB[2]),
}


def test_the_vitb_layout_is_the_one_meant():
    segs, groups, buffer_n = VITB
    assert len(segs) >= 150 and len(groups) == 28 and buffer_n > 100_000_000
    assert sum(n for _, n, _ in segs) < buffer_n                      # holes: pos_embed is not there, the MAE decoder is


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_table_equals_the_restatement_and_partitions_the_segments(name):
    segs, n_groups, buffer_n = LAYOUTS[name]
    table, n_work = ops.adamw_segments_plan(segs, n_groups, buffer_n)
    want = ar.plan_reference(segs, CHUNK)
    assert n_work == len(want) == len(table) and table.tobytes() == want.tobytes()
    assert int(table["n"].max()) <= CHUNK and int(table["n"].min()) >= 4
    # every element of a segment is in exactly one item, no element outside is in any; an item has its segment's group
    assert np.array_equal(ar.table_mask(table, buffer_n), ar.union_mask(segs, buffer_n))
    group_at = np.full(buffer_n, -1, dtype=np.int32)
    for off, n, g in segs:
        group_at[off:off + n] = g
    for it in table:
        assert (group_at[it["offset"]:it["offset"] + it["n"]] == it["group"]).all()


def test_the_table_does_not_depend_on_the_input_order():
    segs, n_groups, buffer_n = LAYOUTS["kernel-case"]
    want = ops.adamw_segments_plan(sorted(segs), n_groups, buffer_n)[0].tobytes()
    rng = np.random.default_rng(0)
    for _ in range(5):
        assert ops.adamw_segments_plan([segs[i] for i in rng.permutation(len(segs))], n_groups, buffer_n)[0].tobytes() == want


def test_need_bytes_without_a_table_and_a_small_table():
    L = _lib.lib()
    segs = (_lib.AdamwSegment * 2)()
    segs[0].offset, segs[0].n, segs[0].group = 0, CHUNK + 4, 0
    segs[1].offset, segs[1].n, segs[1].group = CHUNK + 12, 8, 0
    need, n_work = ctypes.c_int64(-1), ctypes.c_int32(-1)
    args = (ctypes.addressof(segs), 2, 1, 2 * CHUNK)
    assert L.skyemb_adamw_segments_plan(*args, None, 0, ctypes.addressof(need), ctypes.addressof(n_work)) == 0
    assert (need.value, n_work.value) == (48, 3)
    buf = (ctypes.c_char * 48)()
    assert L.skyemb_adamw_segments_plan(*args, ctypes.addressof(buf), 32, ctypes.addressof(need), ctypes.addressof(n_work)) != 0
    assert b"table of 32 bytes: 3 work items need 48" in L.skyemb_last_error()
    assert L.skyemb_adamw_segments_plan(*args, ctypes.addressof(buf), 48, ctypes.addressof(need), ctypes.addressof(n_work)) == 0
    assert bytes(buf) == ar.plan_reference([(0, CHUNK + 4, 0), (CHUNK + 12, 8, 0)], CHUNK).tobytes()


@pytest.mark.parametrize("segs, n_groups, buffer_n, text", [
    ([], 1, 64, "n_segs = 0"),
    ([(0, 8, 0)], 0, 64, "n_groups = 0: expected 1 .. %d" % MAX_GROUPS),
    ([(0, 8, 0)], MAX_GROUPS + 1, 64, "n_groups = %d: expected 1 .. %d" % (MAX_GROUPS + 1, MAX_GROUPS)),
    ([(0, 8, 0), (10, 8, 0)], 1, 64, "segment 1: offset 10 is not"),
    ([(0, 8, 0), (-4, 8, 0)], 1, 64, "segment 1: offset -4 is not"),
    ([(0, 8, 0), (8, 6, 0)], 1, 64, "segment 1: length 6 is not"),
    ([(0, 0, 0)], 1, 64, "segment 0: length 0 is not"),
    ([(0, 8, 0), (16, -8, 0)], 1, 64, "segment 1: length -8 is not"),
    ([(0, 8, 0), (60, 8, 0)], 1, 64, "segment 1: [60, 68) leaves the buffer [0, 64)"),
    ([(64, 8, 0)], 1, 64, "segment 0: [64, 72) leaves the buffer [0, 64)"),
    ([(0, 16, 0), (8, 16, 0)], 1, 64, "segment 1: [8, 24) overlaps segment 0: [0, 16)"),
    ([(8, 16, 0), (32, 8, 0), (0, 16, 0)], 1, 64, "segment 0: [8, 24) overlaps segment 2: [0, 16)"),
    ([(0, 32, 0), (40, 8, 0), (8, 8, 0)], 1, 64, "segment 2: [8, 16) overlaps segment 0: [0, 32)"),
    ([(0, 8, 0), (0, 8, 0)], 1, 64, "segment 1: [0, 8) overlaps segment 0: [0, 8)"),
    ([(0, 8, 0), (8, 8, 2)], 2, 64, "segment 1: group 2 outside [0, 2)"),
    ([(0, 8, -1)], 2, 64, "segment 0: group -1 outside [0, 2)"),
])
def test_plan_refusals(segs, n_groups, buffer_n, text):
    with pytest.raises(ValueError) as e:
        ops.adamw_segments_plan(segs, n_groups, buffer_n)
    assert "skyemb_adamw_segments_plan" in str(e.value) and text in str(e.value), str(e.value)


def test_launch_refusals_come_before_any_device_work():
    L = _lib.lib()
    buf = (ctypes.c_char * 256)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    groups = ops.adamw_groups([(1e-3, 0.1, 0.05, 0.9, 0.95, 1e-8, 0.05, True)])
    g = ctypes.addressof(groups)

    def call(p=a, gr=a, m=a, v=a, lp=a, dtype=_lib.F32, table=a, n_work=1, grp=g, n_groups=1, skip=None):
        rc = L.skyemb_adamw_segments(p, gr, m, v, lp, dtype, table, n_work, grp, n_groups, 1.0, skip, None)
        return rc, L.skyemb_last_error().decode()
    for kw in (dict(p=None), dict(gr=None), dict(m=None), dict(v=None), dict(lp=None), dict(table=None), dict(grp=None)):
        rc, msg = call(**kw)
        assert rc != 0 and "skyemb_adamw_segments: null pointer" in msg, (kw, msg)
    for kw in (dict(p=a + 4), dict(gr=a + 8), dict(m=a + 4), dict(v=a + 12), dict(lp=a + 8), dict(lp=a + 4, dtype=_lib.BF16),
               dict(table=a + 8), dict(skip=a + 2)):
        rc, msg = call(**kw)
        assert rc != 0 and "skyemb_adamw_segments: unaligned buffers" in msg, (kw, msg)
    for n_work in (0, -3):
        rc, msg = call(n_work=n_work)
        assert rc != 0 and f"n_work = {n_work}" in msg
    for n_groups in (0, MAX_GROUPS + 1):
        rc, msg = call(n_groups=n_groups)
        assert rc != 0 and f"n_groups = {n_groups}: expected 1 .. {MAX_GROUPS}" in msg
    rc, msg = call(dtype=7)
    assert rc != 0 and "bad dtype 7" in msg


# ---- the launch splitter ---------------------------------------------------------------------------------------------------------
def synthetic(n_groups, empty=()):
    """Two stores: every group not in `empty` has two segments in store 'a'; every third group also one in store 'b'."""
    segs, off = [], {"a": 0, "b": 0}
    for g in range(n_groups):
        if g in empty:
            continue
        for store in ("a", "a") + (("b",) if g % 3 == 0 else ()):
            segs.append((store, off[store], 8 + 4 * (g % 5), g))
            off[store] += 8 + 4 * (g % 5) + 8 * (g % 2)
    return segs


@pytest.mark.parametrize("n_groups", [1, MAX_GROUPS, MAX_GROUPS + 1, 2 * MAX_GROUPS, 200, 3 * MAX_GROUPS + 1])
@pytest.mark.parametrize("with_empty", [False, True])
def test_launch_splitter(n_groups, with_empty):
    empty = set(range(1, n_groups, 7)) if with_empty else set()
    segs = synthetic(n_groups, empty)
    launches = segmented_launches(segs, MAX_GROUPS)
    seen = []
    for store, group_ids, local in launches:
        assert 1 <= len(group_ids) <= MAX_GROUPS and group_ids == sorted(set(group_ids)) and not set(group_ids) & empty
        assert {k for _, _, k in local} == set(range(len(group_ids)))          # renumbered per launch, every listed group used
        seen += [(store, off, n, group_ids[k]) for off, n, k in local]
    assert sorted(seen) == sorted(segs) and len(seen) == len(set(seen))        # every (store, segment) exactly once
    touching = {s: len({g for st, _, _, g in segs if st == s}) for s in ("a", "b")}
    assert len(launches) == sum(-(-t // MAX_GROUPS) for t in touching.values() if t)      # minimal
    for s, t in touching.items():
        if 0 < t <= MAX_GROUPS:
            assert sum(1 for st, _, _ in launches if st == s) == 1             # one launch per store when the groups fit
    # consecutive launches of a store walk its groups in ascending order
    for s in ("a", "b"):
        ids = [g for st, gids, _ in launches if st == s for g in gids]
        assert ids == sorted(ids)


def test_launch_splitter_on_nothing_and_on_the_linear_probe():
    assert segmented_launches([], MAX_GROUPS) == []
    # the linear probe's groups: norm. (engine), fc_norm. (empty), head. (head store)
    segs = [("engine", 800, 64, 0), ("engine", 864, 64, 0), ("head", 0, 192, 2), ("head", 192, 8, 2)]
    assert segmented_launches(segs, MAX_GROUPS) == [("engine", [0], [(800, 64, 0), (864, 64, 0)]), ("head", [2], [(0, 192, 0), (192, 8, 0)])]


# ---- the mutants -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernel_case():
    segs, buffer_n, canary = ar.kernel_layout(CHUNK)
    table, _ = ops.adamw_segments_plan(segs, len(ar.GROUPS), buffer_n)
    return segs, buffer_n, canary, table


def test_kernel_layout_is_the_one_meant(kernel_case):
    segs, buffer_n, canary, table = kernel_case
    assert sorted(n for _, n, _ in segs) == [8, 12, CHUNK - 4, CHUNK, CHUNK + 4, 2 * CHUNK + 8]
    assert segs != sorted(segs) and 3 <= len(ar.GROUPS) <= 5
    assert canary[:8].all() and canary[-8:].all() and int(canary.sum()) == 5 * ar.GAP
    assert np.array_equal(ar.union_mask(segs, buffer_n) == 0, canary)
    gs = ar.GROUPS
    assert len({g["lr"] for g in gs}) == len(gs) and len({(g["beta1"], g["beta2"]) for g in gs}) == len(gs)
    assert any(g["wd"] == 0 for g in gs) and {g["decayed"] for g in gs} == {True, False}
    assert any(g["wd"] != 0 and not g["decayed"] for g in gs)                  # the flag, not wd, decides
    assert len(table) > len(segs)


@pytest.mark.parametrize("c", ar.KERNEL_CASES, ids=ar.kcase_id)
def test_every_mutant_changes_every_kernel_case(kernel_case, c):
    segs, buffer_n, canary, table = kernel_case
    t = ar.kernel_inputs(c, buffer_n, canary)
    true = ar.emulate(t, table, segs, ar.GROUPS, c, CHUNK)
    assert ar.differs(true, ar.emulate(t, table, segs, ar.GROUPS, c, CHUNK)) == 0
    # the emulation itself: outside the segments nothing moves, inside p_lp is written everywhere
    outside = torch.from_numpy(canary)
    for k in ("p", "m", "v", "p_lp"):
        assert torch.equal(ar.as_int(true[k])[outside], ar.as_int(t[k])[outside])
    assert not bool(torch.isnan(true["p_lp"][~outside].float()).any())
    for mutant in ar.MUTANTS:
        n = ar.differs(true, ar.emulate(t, table, segs, ar.GROUPS, c, CHUNK, mutant))
        print(ar.kcase_id(c), mutant, n)
        assert n >= 1, mutant


def test_the_emulation_meets_the_fp64_bar_per_segment(kernel_case):
    """The emulation is held to rowwise_reference's own statement under each group's scalars: the swap of its scalars works."""
    from tests import rowwise_reference as rr
    segs, buffer_n, canary, table = kernel_case
    c = ar.KCase(ar.BF, 2.0 ** -10)
    t = ar.kernel_inputs(c, buffer_n, canary)
    true = ar.emulate(t, table, segs, ar.GROUPS, c, CHUNK)
    saved = dict(rr.ADAM)
    for off, n, gi in segs:
        sl = slice(off, off + n)
        case = ar.aw_case(n, ar.GROUPS[gi]["decayed"], c.lp, c.grad_scale)
        with ar.group_scalars(ar.GROUPS[gi]):
            ref, err = rr.aw_reference({k: t[k][sl] for k in ("p", "g", "m", "v")}, case)
            bars = rr.aw_bars(ref, err, case)
        for k in bars:
            assert rr.ratio(true[k][sl], ref["p" if k == "p_lp" else k], bars[k]) <= 1.0, (off, k)
    assert rr.ADAM == saved                                                    # the shared reference is left as it was
