"""GPU parity of skyemb_gemm, every product tile, operand-layout class, epilogue and dtype, ELEMENT BY ELEMENT: each case of
tests/gemm_reference.py CASES goes through ops.gemm and every element of every output is held to the fp64 statement and the
derived bar of that module (pinned on the CPU by tests/test_gemm_reference_cpu.py, which also checks that CASES reaches every tile
code in every layout class it is built for, every epilogue, split-K and the fallback kernel, and that subtly wrong kernels -- a
truncating store, GELU of the rounded pre-activation, a swapped k-tile ... -- exceed the bar).

What a case checks besides the bar (a NaN, e.g. an element never written, fails it):
- guards: A and B are views into larger buffers with ld beyond the contiguous extent; the padding columns and the rows before and
  after are NaN, so a read outside the operand poisons a result.  The same for resid, aux, table and bias; tab_row and dst_row
  have guard entries around them that name a valid but wrong row whose table / residual row is NaN.  The split-K workspace starts
  as NaN.  Outputs are views with ld beyond N that start as NaN inside and carry a sentinel outside: every element must be
  written, nothing outside may change -- the columns [N, ld) of every row, the rows of dst_row = -1 and the unmapped rows of a
  scatter (which must still be NaN) included;
- contrast (gemm_reference.inputs): rows of A per 16-row fragment and rows of B per 8-wide piece carry different powers of two;
- repeatability: a second call gives the same bits, split-K included;
- path: the change in ops.gemm_launch_counts() is what gemm_reference.planned says (pipe / 256 x 256 / fallback, the split-K
  reduce exactly when S > 1, two launches for the row tail): a case that falls to another kernel fails;
- signed bias (the "pos" cases, one per 16-bit dtype and kernel family): mean signed error over mean bar below BIAS = 0.1 --
  rounding to nearest is unbiased (sampling noise ~0.4 bar / sqrt(n)), a truncating store is pulled by ~0.35 of the bar
  (test_signed_bias_separates_rne_from_truncation shows the separation on the CPU).

The row tail: plan_single emits two launches only past a whole round of 128x128 / 256x128 / 256x256 tiles (>= 8.3 M outputs); the
case here has the fewest rows for which it does (1025 x 8072, K = 128: test_row_tail_case_has_the_fewest_rows) and is the one case
that allocates more than a few MB (two 16-bit outputs of 16.6 MB).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_reference as gr
from tests.gemm_reference import CASES, F16, F32, KC, RC, cid, has
from tests.helpers import DEV, NAN, Out, record_parity
from tests.helpers import gemm_device_inputs as device_inputs

BIAS = 0.1


def launch(ops, c, t, dev_in):
    """One ops.gemm call of case c into fresh guarded outputs: {name: Out}."""
    ld = gr.lds(c)
    Mo = gr.out_rows(c)
    outs, kw = {}, {}
    if has(c, "out_f32"):
        outs["out_f32"] = Out(Mo, c.N, F32, ld["ldo32"])
        kw.update(out_f32=outs["out_f32"].view, ldo32=ld["ldo32"])
    if has(c, "out"):
        outs["out"] = Out(Mo, c.N, c.dtype, ld["ldo"])
        kw.update(out=outs["out"].view, ldo=ld["ldo"])
    if has(c, "out2"):
        outs["out2"] = Out(Mo, c.N, c.dtype, ld["ldo2"])
        kw.update(out2=outs["out2"].view, ldo2=ld["ldo2"])
    if has(c, "colsum"):
        outs["colsum"] = Out(1, c.M, F32, c.M + 8)
        kw.update(colsum_a=outs["colsum"].view)
    if c.ws:
        kw.update(ws=torch.full((gr.ws_floats(c),), NAN, device=DEV))
    act = {"gelu": ops.ACT_GELU, "dgelu": ops.ACT_DGELU}.get(c.epi, ops.ACT_NONE)
    ops.gemm(dev_in["A"], dev_in["B"], M=c.M, N=c.N, K=c.K, a_layout=c.al, b_layout=c.bl, lda=ld["lda"], ldb=ld["ldb"],
             alpha=t["alpha"], act=act, tile=c.tile, split_k=c.split, **dev_in["kw"], **kw)
    return outs


def check_case(ops, c, worst=None):
    t = gr.inputs(c)
    name = cid(c)
    plan = gr.planned(c)
    dev_in = device_inputs(c, t)
    before = ops.gemm_launch_counts()
    o1 = launch(ops, c, t, dev_in)
    after = ops.gemm_launch_counts()
    o2 = launch(ops, c, t, dev_in)
    torch.cuda.synchronize()
    delta = {k: after[k] - before[k] for k in ("fallback", "pipe", "tile256", "splitk", "group", "group256")}
    assert delta == dict(plan["counts"], group=0, group256=0), (name, "path", delta, plan)
    st = gr.reference(c, t)
    bars = gr.bars(c, st)
    ratios = {}
    for n, o in o1.items():
        assert o.outside_intact(), (name, n, "written outside the output")
        assert torch.equal(o.bits(), o2[n].bits()), (name, n, "a second call gave other bits")
        got = o.view.double().cpu()
        got = got[0] if n == "colsum" else got
        ratios[n] = gr.ratio(got, st["ref"][n], bars[n])
        if c.kind == "pos" and n == "out":
            bias = float((got - st["ref"][n]).mean() / bars[n].mean())
            print(f"{name} signed bias {bias:.4f}")
            assert abs(bias) < BIAS, (name, "signed bias", bias)
    print(f"{name} [{plan['family']} {plan['tile']} S={plan['split']}] err/bar {ratios}")
    if worst is not None:
        fam = f"{gr.DT[c.dtype]}/{plan['family']}"
        worst[fam + "/cases"] = worst.get(fam + "/cases", 0) + 1
        for n, r in ratios.items():
            worst[f"{fam}/{n}"] = max(worst.get(f"{fam}/{n}", 0.0), r)
    bad = {n: r for n, r in ratios.items() if not r <= 1.0}
    assert not bad, (name, plan["family"], plan["tile"], ratios)
    return ratios


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
    record_parity("gemm_elementwise", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in sorted(w.items())})


@pytest.mark.parametrize("c", CASES, ids=cid)
def test_gemm_elementwise(ops, worst, c):
    check_case(ops, c, worst)


def test_refusals_are_reported(ops):
    """Where refusal is the documented behaviour (gemm_reference.planned: "refused"): a named tile outside its subset raises instead
    of running something else -- the 144-row tiles with a row-contiguous A, the two-k-group tiles at an odd number of k-tiles, the
    256 x 256 tile below two k-tiles, with row maps, or with a row-contiguous A that is not a whole-tile weight gradient."""
    for c in (gr.Case(torch.bfloat16, 9144064, RC, RC, 136, 72, 128, "plain"), gr.Case(F16, 13144256, RC, KC, 136, 264, 128, "plain"),
              gr.Case(torch.bfloat16, 9064064, KC, KC, 70, 72, 192, "plain"), gr.Case(F16, 9128128, KC, RC, 70, 72, 64, "plain"),
              gr.Case(torch.bfloat16, 256256, KC, KC, 264, 264, 64, "plain"), gr.Case(F16, 256256, KC, KC, 264, 264, 128, "full"),
              gr.Case(torch.bfloat16, 256256, RC, KC, 264, 264, 128, "plain")):
        assert gr.planned(c)["family"] == "refused"
        t = gr.inputs(c)
        before = ops.gemm_launch_counts()
        with pytest.raises(Exception):
            launch(ops, c, t, device_inputs(c, t))
        assert ops.gemm_launch_counts() == before, cid(c)
