"""GPU parity of the grouped GEMM launches (skyemb_gemm_group_plan / _launch: gemm_pipe_group_kernel on the ring tiles,
gemm256_group_kernel on 256 x 256), ELEMENT BY ELEMENT: each case of tests/gemm_group_reference.py GROUP_CASES -- every grouped
tile, class mask 1 / 2 / 4 / 6, both 16-bit formats, both tile orders, per-problem K and epilogues, the 16-bit gradient mirror, 32
problems, a prefetch hint of a ragged size -- is planned once with ops.GemmGroup and launched twice, and every element of every
output of every problem is held to the fp64 statement and the bar of tests/gemm_reference.py (ratio <= 1, the one tolerance; the
table and the bar are pinned on the CPU by tests/test_gemm_group_reference_cpu.py, which also shows that one tile computed with a
neighbour's arguments or K, a dropped last tile, a padding workgroup that stores, and a truncating mirror store exceed the bar).

What a case checks besides the bar:
- guards, as tests/test_gemm_elementwise_gpu.py (tests/helpers.py): operands, bias, table, resid and aux sit in NaN buffers, row maps
  have guard entries naming NaN rows; outputs are NaN views inside sentinel buffers: every element must be written, nothing outside
  may change -- the columns [N, ld), the rows before and after, the rows of dst_row = -1 and the unmapped rows of a scatter;
- contrast between problems (gemm_group_reference.inputs): seeds and powers of two per problem;
- repeatability: the second launch of the same blob gives the same bits;
- the same tile body: each problem's bits equal those of ops.gemm(tile = the group's code, split_k = 1) into fresh outputs
  (gemm_group_reference.single_refused lists the problems without such a launch: none in the present table);
- path: one `group` (ring tiles) or one `group256` launch per launch() in ops.gemm_launch_counts(), nothing else;
- the plan: info.tile is the code asked for, total_blocks the model's and a multiple of 8, class_mask the model's.
The two tile orders of a weight-gradient group give identical bits; a KC.RC + RC.RC group on 9128128 is refused by the plan.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_group_reference as gg
from tests import gemm_reference as gr
from tests.gemm_group_reference import GROUP_CASES, GROUPED_TILES, gid
from tests.gemm_reference import BF, F16, F32, KC, RC, T256, Case
from tests.helpers import DEV, NAN, Out, gemm_device_inputs, record_parity

COUNTS = ("fallback", "pipe", "tile256", "splitk", "group", "group256")


def fresh_outputs(c):
    """-> ({name: Out}, the output arguments of ops.gemm / ops.gemm_args)."""
    ld = gg.lds(c)
    Mo = gg.out_rows(c)
    outs, kw = {}, {}
    if gg.has(c, "out_f32"):
        outs["out_f32"] = Out(Mo, c.N, F32, ld["ldo32"])
        kw.update(out_f32=outs["out_f32"].view, ldo32=ld["ldo32"])
    if gg.has(c, "out"):
        outs["out"] = Out(Mo, c.N, c.dtype, ld["ldo"])
        kw.update(out=outs["out"].view, ldo=ld["ldo"])
    if gg.has(c, "out2"):
        outs["out2"] = Out(Mo, c.N, c.dtype, ld["ldo2"])
        kw.update(out2=outs["out2"].view, ldo2=ld["ldo2"])
    if gg.has(c, "colsum"):
        outs["colsum"] = Out(1, c.M, F32, c.M + 8)
        kw.update(colsum_a=outs["colsum"].view)
    return outs, kw


def call_kw(ops, c, t, dev_in, out_kw, tile):
    ld = gg.lds(c)
    act = {"gelu": ops.ACT_GELU, "dgelu": ops.ACT_DGELU}.get(c.epi, ops.ACT_NONE)
    return dict(M=c.M, N=c.N, K=c.K, a_layout=c.al, b_layout=c.bl, lda=ld["lda"], ldb=ld["ldb"], alpha=t["alpha"], act=act, tile=tile,
                **dev_in["kw"], **out_kw)


def set_order(monkeypatch, order):
    if order is None:
        monkeypatch.delenv("SKYEMB_GROUP_XCD_ORDER", raising=False)
    else:
        monkeypatch.setenv("SKYEMB_GROUP_XCD_ORDER", order)


class Prepared:
    """Operands of a grouped case on the device (behind guards) and its fp64 statement: built once per case, not modified."""

    def __init__(self, gc):
        self.ts = [gg.inputs(gc, j) for j in range(len(gc.problems))]
        self.dev = [gemm_device_inputs(gg.base(c), t) for c, t in zip(gc.problems, self.ts)]
        self.sts = [gg.reference(c, t) for c, t in zip(gc.problems, self.ts)]
        self.bars = [gg.bars(c, st) for c, st in zip(gc.problems, self.sts)]
        self.hint = None
        if gc.hint:                                          # `hint` bytes in the middle of a larger buffer
            self.hint = torch.zeros(gc.hint // 4 + 64, device=DEV)[32:32 + gc.hint // 4]


def run_group(ops, monkeypatch, gc, prep, order):
    """Plan gc under `order`, launch twice -> ([{name: Out}] per problem, bits of the first launch, the plan)."""
    set_order(monkeypatch, order)
    outs, args = [], []
    for j, (c, t, d) in enumerate(zip(gc.problems, prep.ts, prep.dev)):
        o, kw = fresh_outputs(c)
        outs.append(o)
        args.append(ops.gemm_args(d["A"], d["B"], prefetch=prep.hint if j == 0 else None, **call_kw(ops, c, t, d, kw, gc.tile)))
    if gc.hint:
        assert args[0].prefetch_bytes == gc.hint and gc.hint % 16
    grp = ops.GemmGroup(args, DEV, tile=gc.tile)
    name = gid(gc)
    assert grp.ok, (name, ops.lib().skyemb_last_error())
    h = gg.header(gc.tile, gc.problems, order)
    assert grp.info.tile == gc.tile and grp.info.total_blocks == h["total"] and h["total"] % 8 == 0, (name, grp.info.tile, grp.info.total_blocks)
    assert grp.info.class_mask == h["mask"] and grp.total_blocks == h["total"]
    want = dict.fromkeys(COUNTS, 0)
    want["group256" if gc.tile == T256 else "group"] = 1
    first = None
    for launch in range(2):
        before = ops.gemm_launch_counts()
        grp.launch()
        after = ops.gemm_launch_counts()
        torch.cuda.synchronize()
        assert {k: after[k] - before[k] for k in COUNTS} == want, (name, "path")
        bits = [{n: o.bits().clone() for n, o in po.items()} for po in outs]
        if first is None:
            first = bits
            for po in outs:
                for o in po.values():
                    o.view.fill_(NAN)
        else:
            for j, (b1, b2) in enumerate(zip(first, bits)):
                for n in b1:
                    assert torch.equal(b1[n], b2[n]), (name, j, n, "the second launch gave other bits")
    return outs, first, grp


def check_group(ops, monkeypatch, gc, worst=None):
    name = gid(gc)
    prep = Prepared(gc)
    outs, bits, grp = run_group(ops, monkeypatch, gc, prep, gc.order)
    mask = grp.info.class_mask
    fam = f"{gr.DT[gc.dtype]}/{'tile256' if gc.tile == T256 else 'ring'}/mask{mask}"
    bad = {}
    for j, (c, po) in enumerate(zip(gc.problems, outs)):
        ratios = {}
        for n, o in po.items():
            assert o.outside_intact(), (name, j, n, "written outside the output")
            got = o.view.double().cpu()
            got = got[0] if n == "colsum" else got
            ratios[n] = gr.ratio(got, prep.sts[j]["ref"][n], prep.bars[j][n])
            if worst is not None:
                worst[f"{fam}/{n}"] = max(worst.get(f"{fam}/{n}", 0.0), ratios[n])
        if len(gc.problems) <= 6:
            print(f"{name} problem {j} {gr.cid(c)} err/bar {ratios}")
        bad.update({(j, n): r for n, r in ratios.items() if not r <= 1.0})
    if worst is not None:
        worst[fam + "/cases"] = worst.get(fam + "/cases", 0) + 1
    assert not bad, (name, bad)
    # the same tile body as a single launch: the same bits
    refused = gg.single_refused(gc)
    for j, (c, t, d) in enumerate(zip(gc.problems, prep.ts, prep.dev)):
        if j in refused:
            continue
        o, kw = fresh_outputs(c)
        before = ops.gemm_launch_counts()
        ops.gemm(d["A"], d["B"], split_k=1, **call_kw(ops, c, t, d, kw, gc.tile))
        after = ops.gemm_launch_counts()
        want = dict.fromkeys(COUNTS, 0)
        want["tile256" if gc.tile == T256 else "pipe"] = 1
        assert {k: after[k] - before[k] for k in COUNTS} == want, (name, j, "the single launch took another path")
        for n in o:
            assert torch.equal(o[n].bits(), bits[j][n]), (name, j, n, "the group and the single launch of the same tile differ")
    return prep, bits


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    record_parity("gemm_group_elementwise", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in sorted(w.items())})


@pytest.mark.parametrize("gc", GROUP_CASES, ids=gid)
def test_gemm_group_elementwise(ops, worst, monkeypatch, gc):
    check_group(ops, monkeypatch, gc, worst)


@pytest.mark.parametrize("dtype", (BF, F16), ids=("bf16", "f16"))
@pytest.mark.parametrize("tile", GROUPED_TILES)
def test_both_tile_orders_give_the_same_bits(ops, monkeypatch, dtype, tile):
    pair = [gc for gc in GROUP_CASES if (gc.name, gc.dtype, gc.tile) == ("wgrad", dtype, tile)]
    assert len(pair) == 2 and gg.order_on(tile, pair[0].order) != gg.order_on(tile, pair[1].order)
    prep = Prepared(pair[0])
    _, b0, _ = run_group(ops, monkeypatch, pair[0], prep, pair[0].order)
    _, b1, _ = run_group(ops, monkeypatch, pair[1], prep, pair[1].order)
    for j, (x, y) in enumerate(zip(b0, b1)):
        for n in x:
            assert torch.equal(x[n], y[n]), (dtype, tile, j, n)


@pytest.mark.parametrize("dtype", (BF, F16), ids=("bf16", "f16"))
def test_a_mixed_group_on_the_two_k_group_tile_is_refused_by_the_plan(ops, dtype):
    """9128128 has no KC.RC + RC.RC instance: the plan answers -1 with a message (it used to answer 0, and the launch then failed);
    nothing is launched.  The same group on 128128 plans and launches (test_gemm_group_elementwise, "mixed")."""
    problems = [Case(dtype, 9128128, KC, RC, 72, 136, 128, "plain"), Case(dtype, 9128128, RC, RC, 136, 72, 128, "plain")]
    args = []
    keep = []
    for c in problems:
        t = gr.inputs(c)
        d = gemm_device_inputs(c, t)
        o, kw = fresh_outputs(c)
        keep.append((d, o))
        args.append(ops.gemm_args(d["A"], d["B"], **call_kw(ops, c, t, d, kw, 9128128)))
    before = ops.gemm_launch_counts()
    grp = ops.GemmGroup(args, DEV, tile=9128128)
    msg = ops.lib().skyemb_last_error()
    assert not grp.ok and grp.blob is None and msg and b"9128128" in msg and b"mix" in msg, msg
    assert ops.gemm_launch_counts() == before
    for _, o in keep:
        assert all(x.outside_intact() and bool(torch.isnan(x.view).all()) for x in o.values())
