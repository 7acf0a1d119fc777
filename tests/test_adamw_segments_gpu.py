"""GPU: the segmented AdamW launch (ops.adamw_segments, csrc/adamw_segments.hip) against the per-tensor launches it replaces, BIT
FOR BIT -- the kernel on a canaried buffer (and held to the fp64 bar of tests/rowwise_reference.py), the grid-stride wrap, the
overflow guard -- and the downstream predictor end to end: PredictorOptimizer(segmented=True) against segmented=False after every
training step, in fp32, bf16 and fp16 under a dynamic loss scale, an injected overflow included.  Shapes come from
ops.adamw_segments_limits(); the layout, inputs and groups from tests/adamw_segments_reference.py."""
import os
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import adamw_segments_reference as ar
from tests import rowwise_reference as rr
from tests.rowwise_reference import BF, F16, F32
from tests.test_predictor_f16_gpu import CASES, build, optimiser_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BUFS = ("p", "g", "m", "v", "p_lp")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "predictor.npz"))


def upload(table):
    return torch.from_numpy(table.view(np.int32)).to(DEV)


def per_tensor(ops, t, segments, groups, grad_scale):
    """ops.adamw over each segment with its group's scalars, on a copy of the device buffers t."""
    e = {k: x.clone() for k, x in t.items()}
    for off, n, gi in segments:
        lr, bc1, bc2, b1, b2, eps, wd, decayed = ar.group_struct(groups[gi])
        sl = slice(off, off + n)
        ops.adamw(e["p"][sl], e["g"][sl], e["m"][sl], e["v"][sl], e["p_lp"][sl], n, n if decayed else 0, None, b1, b2, eps, wd,
                  grad_scale=grad_scale, lr=lr, bc1=bc1, bc2=bc2)
    return e


def same_bits(a, b, names=BUFS):
    return {k: int((ar.as_int(a[k]) != ar.as_int(b[k])).sum()) for k in names}


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ar.KERNEL_CASES, ids=ar.kcase_id)
def test_segments_match_the_per_tensor_launches_bit_for_bit(ops, c):
    _, chunk, _ = ops.adamw_segments_limits()
    segments, buffer_n, canary = ar.kernel_layout(chunk)
    host = ar.kernel_inputs(c, buffer_n, canary)
    t = {k: x.to(DEV) for k, x in host.items()}
    want = per_tensor(ops, t, segments, ar.GROUPS, c.grad_scale)
    table, n_work = ops.adamw_segments_plan(segments, len(ar.GROUPS), buffer_n)
    ops.adamw_segments(t["p"], t["g"], t["m"], t["v"], t["p_lp"], upload(table), n_work, [ar.group_struct(g) for g in ar.GROUPS],
                       grad_scale=c.grad_scale)
    torch.cuda.synchronize()
    diff = same_bits(t, want)
    print(ar.kcase_id(c), "elements differing from the per-tensor launches", diff)
    assert not any(diff.values()), diff
    # nothing outside the segments moved (the canaries among it), g moved nowhere, and every segment element of p_lp was written
    outside = torch.from_numpy(ar.union_mask(segments, buffer_n) == 0).to(DEV)
    assert bool(outside[torch.from_numpy(canary).to(DEV)].all()) and int(outside.sum()) == int(canary.sum())
    for k in BUFS:
        assert torch.equal(ar.as_int(t[k])[outside], ar.as_int(host[k]).to(DEV)[outside]), k
    assert torch.equal(ar.as_int(t["g"]), ar.as_int(host["g"]).to(DEV))
    assert not bool(torch.isnan(t["p_lp"][~outside].float()).any())
    moved = same_bits(t, {k: x.to(DEV) for k, x in host.items()}, ("p", "m", "v"))
    assert all(n > 0 for n in moved.values()), moved
    # the fp64 bar of the flat-buffer kernel, segment by segment
    worst = defaultdict(float)
    for off, n, gi in segments:
        sl = slice(off, off + n)
        case = ar.aw_case(n, ar.GROUPS[gi]["decayed"], c.lp, c.grad_scale)
        with ar.group_scalars(ar.GROUPS[gi]):
            ref, err = rr.aw_reference({k: host[k][sl].to(DEV) for k in ("p", "g", "m", "v")}, case)
            bars = rr.aw_bars(ref, err, case)
        for k in bars:
            worst[k] = max(worst[k], rr.ratio(t[k][sl], ref["p" if k == "p_lp" else k], bars[k]))
    print(ar.kcase_id(c), "err/bar", dict(worst))
    assert all(r <= 1.0 for r in worst.values()), dict(worst)


def test_grid_stride_wrap(ops):
    """More work items than workgroups: max_grid + 3 items of one chunk each, against ONE ops.adamw launch over the range."""
    _, chunk, max_grid = ops.adamw_segments_limits()
    n = (max_grid + 3) * chunk
    gen = torch.Generator(device=DEV).manual_seed(11)
    t = {"p": torch.randn(n, device=DEV, generator=gen), "g": torch.randn(n, device=DEV, generator=gen) * 0.1,
         "m": torch.randn(n, device=DEV, generator=gen) * 0.01, "v": torch.rand(n, device=DEV, generator=gen) * 0.01,
         "p_lp": torch.full((n,), float("nan"), device=DEV, dtype=BF)}
    g = ar.GROUPS[0]
    want = per_tensor(ops, t, [(0, n, 0)], [g], 1.0)
    table, n_work = ops.adamw_segments_plan([(0, n, 0)], 1, n)
    assert n_work == max_grid + 3 and set(table["n"].tolist()) == {chunk}
    ops.adamw_segments(t["p"], t["g"], t["m"], t["v"], t["p_lp"], upload(table), n_work, [ar.group_struct(g)])
    torch.cuda.synchronize()
    diff = same_bits(t, want)
    assert not any(diff.values()), diff
    assert not bool(torch.isnan(t["p_lp"].float()).any())


def test_guard(ops):
    _, chunk, _ = ops.adamw_segments_limits()
    c = ar.KCase(F16, 2.0 ** -10)
    segments, buffer_n, canary = ar.kernel_layout(chunk)
    host = ar.kernel_inputs(c, buffer_n, canary)
    table, n_work = ops.adamw_segments_plan(segments, len(ar.GROUPS), buffer_n)
    table, groups = upload(table), [ar.group_struct(g) for g in ar.GROUPS]
    runs = {}
    for tag, skip in (("none", None), ("zero", [0, 77]), ("set", [1, 0])):
        t = {k: x.to(DEV) for k, x in host.items()}
        state = None if skip is None else torch.tensor(skip, dtype=torch.int32, device=DEV)
        ops.adamw_segments(t["p"], t["g"], t["m"], t["v"], t["p_lp"], table, n_work, groups, grad_scale=c.grad_scale, skip=state)
        torch.cuda.synchronize()
        runs[tag] = t
        if state is not None:
            assert state.tolist() == skip                      # the guard word is only read
    start = {k: x.to(DEV) for k, x in host.items()}
    assert not any(same_bits(runs["set"], start).values())     # skip[0] != 0: nothing written anywhere
    assert not any(same_bits(runs["zero"], runs["none"]).values())
    assert any(same_bits(runs["none"], start, ("p", "m", "v", "p_lp")).values())


# ---- 2. the predictor, end to end ------------------------------------------------------------------------------------------------
DTYPES = {"f32": (torch.float32, None), "bf16": (torch.bfloat16, None), "f16": (torch.float16, "dynamic")}


def pair(z, case, dtype, loss_scale):
    """The same model and optimiser twice: [segmented, per tensor]."""
    from sky_embeddings_amd.utils.vit import LinearLR, build_optimizer
    init_lr, wd, layer_decay, total, flf = [float(v) for v in z[f"{case}/hyper"]]
    out = []
    for segmented in (True, False):
        model, m = build(z, case, dtype, loss_scale=loss_scale)
        opt = build_optimizer(m, CASES[case][0], init_lr, wd, layer_decay, segmented=segmented)
        assert opt.segmented is segmented
        out.append((model, m, opt, LinearLR(opt, start_factor=1.0, end_factor=1 / flf, total_iters=int(total))))
    return out


def same_state(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same_state(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_state(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    return a == b


def assert_same(ma, mb, oa, ob, what):
    sa, sb = optimiser_state(ma), optimiser_state(mb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, k)
    assert same_state(oa.state_dict(), ob.state_dict()), what


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", ["ft_map_mse", "ft_avg_mse", "lp_token_ce"])
def test_predictor_steps_are_bit_identical(z, case, dt):
    from sky_embeddings_amd.utils.predictor_training_fns import run_iter
    dtype, loss_scale = DTYPES[dt]
    (model_s, m_s, opt_s, sch_s), (model_t, m_t, opt_t, sch_t) = pair(z, case, dtype, loss_scale)
    x, labels = torch.from_numpy(z[f"{case}/x"]), torch.from_numpy(z[f"{case}/labels"])
    cp_s, cp_t = defaultdict(list), defaultdict(list)
    assert_same(m_s, m_t, opt_s, opt_t, "start")
    start = optimiser_state(m_s)
    for it in range(3):
        run_iter(model_s, x[it].cuda(), None, None, labels[it].cuda(), opt_s, sch_s, cp_s, loss_fn=CASES[case][2], mode="train")
        run_iter(model_t, x[it].cuda(), None, None, labels[it].cuda(), opt_t, sch_t, cp_t, loss_fn=CASES[case][2], mode="train")
        assert_same(m_s, m_t, opt_s, opt_t, it)
        assert cp_s["train_loss"] == cp_t["train_loss"], (it, cp_s["train_loss"], cp_t["train_loss"])
        assert opt_s.step_count == opt_t.step_count
        assert 1 <= opt_s.last_step_launches <= 2
        assert opt_t.last_step_launches == len(opt_t._names()) > 2
    assert opt_s.step_count >= 1
    end = optimiser_state(m_s)
    assert not torch.equal(start["head.p"], end["head.p"]) and not torch.equal(start["engine.p"], end["engine.p"])


def test_injected_overflow_is_skipped_in_both_modes(z):
    """fp16, dynamic scale: an inf written into the gradient buffer from the host before step() -- the step is skipped, step_count
    stays, no buffer changes; the next clean step is bit-identical between the modes again."""
    case = "ft_map_mse"
    runs = pair(z, case, torch.float16, "dynamic")
    x, labels = torch.from_numpy(z[f"{case}/x"]), torch.from_numpy(z[f"{case}/labels"])

    def backward(model, m, it):
        model.train(True)
        loss = torch.nn.MSELoss()(model(x[it].cuda()), m.normalize_labels(labels[it].cuda()))
        loss.backward()
        return float(loss.detach())

    for model, m, opt, sched in runs:
        backward(model, m, 0)
        name = opt.param_groups[0]["params"][0]
        (_, gr, _, _, _), _ = opt._buffers(name)
        gr[:1].copy_(torch.tensor([float("inf")]))                     # a host-side write into the flat gradient buffer
        before, skipped, scale = optimiser_state(m), m.scaler.skipped_steps, m.scaler.scale
        opt.step()
        sched.step()
        after = optimiser_state(m)
        for k in before:
            assert torch.equal(before[k], after[k]), (opt.segmented, k)
        assert opt.step_count == 0 and m.scaler.skipped_steps == skipped + 1 and m.scaler.scale == scale / 2
    (_, m_s, opt_s, _), (_, m_t, opt_t, _) = runs
    assert_same(m_s, m_t, opt_s, opt_t, "after the skipped step")
    # clean steps until one is taken (the dynamic scale may still have to come down): the same in both modes
    for it in (1, 2, 0):
        losses = []
        for model, m, opt, sched in runs:
            losses.append(backward(model, m, it))
            opt.step()
            sched.step()
        assert losses[0] == losses[1]
        assert_same(m_s, m_t, opt_s, opt_t, it)
        assert opt_s.step_count == opt_t.step_count
    assert opt_s.step_count >= 1
