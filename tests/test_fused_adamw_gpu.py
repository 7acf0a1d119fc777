"""The AdamW step fused into the grouped weight-gradient launches (csrc/gemm_pipe.hip, csrc/gemm_pipe256.h), through ops.GemmGroup
and through TrainStep.

Two forms carry the step of a transformer block's weight matrices: the EPILOGUE form (skyemb_gemm_group_plan_adamw: a launch steps
its own tiles instead of storing their gradients) and the SIDE form (skyemb_gemm_group_plan_side_adamw: extra workgroups behind the
tiles step the flat slice [lo, hi) whose gradients an earlier launch stored; own_step says whether the launch's own tiles are
stepped in their epilogue too or stored).  Every kernel case puts its problems in ONE flat fp32 buffer, as the engine does: 8-aligned
offsets with gaps between them, and a sentinel pattern in the gaps and in every element of g, p, m, v and the 16-bit shadow p_lp
the launch must not touch.  Each case has two references:

- bit-exact: the same problems planned WITHOUT the optimiser store their gradients into a separate flat buffer, then ops.adamw
  steps each updated range with the same scalars (adamw_math.h pins every rounding, so the fused forms must give the same bits in
  p, m, v and p_lp), and every buffer outside the updated ranges keeps its sentinels;
- float64: the AdamW statement of oracle/mae_oracle.adamw_step, evaluated in fp64 from the fp32 inputs and the gradient the
  kernel used (the plain group's), within the bar below; p_lp equals p rounded to the shadow format.

Bar of the fp64 comparison (u = 2^-24, the unit roundoff of fp32; the scalars are the fp32 values the kernel receives, and the
gradient scale s is a power of two, so g s is exact).  First-order bounds of the fp32 statement's rounding errors:
- m' = fma(m, b1, (g s)(1 - b1)): the rounding of 1 - b1, of the product and of the fma: |dm| <= 3u (|b1 m| + |(1 - b1) g s|).
- v' = fma(v, b2, (g s)^2 (1 - b2)): four roundings: |dv| <= 4u (b2 v + (1 - b2) (g s)^2).
- d = sqrt(v') / sqrt(bc2) + eps: relative error <= |dv| / (2 v') + 4u (sqrt, sqrt(bc2), the division, the sum).
- q = m' / d: |dq| <= |dm| / d + |q| (rel(d) + u).
- p' = fma(-lr / bc1, q, p (1 - lr wd)): the decayed p carries <= 3u |p| (two roundings in 1 - lr wd, one in the product), the
  step size u, the fma u |p'|: |dp| <= 3u |p| + (lr / bc1) (|dq| + 2u |q|) + u |p'|.
The worst error over the bar of each form and format is recorded (tests/helpers.record_parity).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import record_parity

DEV = "cuda"
NAN = float("nan")
BF, FH = torch.bfloat16, torch.float16
DT = {BF: "bf16", FH: "f16"}
TILES = [64064, 128064, 128128, 256256]
B1, B2, EPS, WD, GS = 0.9, 0.95, 1e-8, 0.05, 2.0 ** -4
U = 2.0 ** -24
_WORST = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()  # fail loudly if libskyemb.so is missing
    return _ops


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def sentinel(n, salt, dtype=torch.float32):
    """A finite pattern no kernel produces by accident (integers, exact in fp32, bf16 and fp16)."""
    return (-(torch.arange(n, device=DEV) % 61 + 100 + salt)).to(dtype)


def hyper_for(step, lr=1e-3):
    return torch.tensor([lr, 1 - B1 ** step, 1 - B2 ** step, 0.0], device=DEV, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------------ case setup
class Case:
    """Problems [(n_out, k_in, with_bias)] over T token rows in one flat buffer; optionally a side slice of `side_len` elements placed
    after the first problem.  Gaps of 16, 24, 32, ... elements before every region."""

    def __init__(self, ops, tile, dtype, shapes, T, seed, side_len=0, n_decay=None):
        self.ops, self.tile, self.dtype, self.shapes, self.T = ops, tile, dtype, shapes, T
        g = torch.Generator().manual_seed(seed)
        cur, self.offs, self.side = 24, [], None
        for j, (o, i, _) in enumerate(shapes):
            if side_len and j == 1:
                self.side = (cur, cur + side_len)
                cur += side_len + 8 * (j + 2)
            self.offs.append(cur)
            cur += o * i + 8 * (j + 2)
        self.n = cur + 40
        self.ranges = [(s, s + o * i) for s, (o, i, _) in zip(self.offs, shapes)]
        self.n_decay = n_decay
        self.dys = [torch.randn(T, o, generator=g).to(DEV, dtype) for o, _, _ in shapes]
        self.xs = [torch.randn(T, i, generator=g).to(DEV, dtype) for _, i, _ in shapes]
        n = self.n
        self.p0 = (torch.randn(n, generator=g) * 0.5).to(DEV)
        self.m0 = (torch.randn(n, generator=g) * 0.05).to(DEV)
        self.v0 = (torch.rand(n, generator=g) * 1e-2).to(DEV)
        self.g0 = sentinel(n, 0)
        if self.side is not None:                                 # the gradients an earlier launch stored for the side slice
            lo, hi = self.side
            self.g0[lo:hi] = (torch.randn(hi - lo, generator=g) * 8).to(DEV)
        self.plp0 = sentinel(n, 7, dtype)

    def problems(self, flat, dbs):
        RC = 1
        return [self.ops.gemm_args(self.dys[j], self.xs[j], M=o, N=i, K=self.T, a_layout=RC, b_layout=RC, lda=o, ldb=i,
                                   out_f32=flat[self.offs[j]:self.offs[j] + o * i].view(o, i), colsum_a=dbs[j])
                for j, (o, i, _) in enumerate(self.shapes)]

    def bias_bufs(self):
        return [torch.full((o,), NAN, device=DEV) if b else None for o, _, b in self.shapes]

    def plain(self):
        """The reference gradients: the same problems planned without the optimiser, stored into a separate flat buffer."""
        gref, dbs = sentinel(self.n, 0), self.bias_bufs()
        grp = self.ops.GemmGroup(self.problems(gref, dbs), DEV, tile=self.tile)
        assert grp.ok and grp.info.tile == self.tile
        grp.launch()
        if self.side is not None:
            lo, hi = self.side
            gref[lo:hi] = self.g0[lo:hi]
        return gref, dbs

    def state(self):
        return self.g0.clone(), self.p0.clone(), self.m0.clone(), self.v0.clone(), self.plp0.clone()

    def desc(self, bufs, hyper, grad_scale=GS):
        from sky_embeddings_amd._lib import AdamwDesc
        g, p, m, v, plp = bufs
        d = AdamwDesc()
        d.g_base, d.p, d.m, d.v, d.p_lp, d.hyper = (t.data_ptr() for t in (g, p, m, v, plp, hyper))
        d.n_decay, d.beta1, d.beta2, d.eps, d.weight_decay, d.grad_scale = self.n_decay, B1, B2, EPS, WD, grad_scale
        return d

    def reference(self, bufs, stepped, gsrc, hyper, grad_scale=GS):
        """ops.adamw over every range of `stepped` (in place on bufs = (g, p, m, v, p_lp)), gradients from gsrc."""
        _, p, m, v, plp = bufs
        for s, e in stepped:
            self.ops.adamw(p[s:e], gsrc[s:e], m[s:e], v[s:e], plp[s:e], e - s, min(max(self.n_decay - s, 0), e - s), hyper, B1, B2, EPS,
                           WD, grad_scale=grad_scale)


def fp64_check(case, got, stepped, gsrc, hyper, key, grad_scale=GS):
    """The fp64 AdamW statement from the fp32 inputs over `stepped`; records and returns the worst error over the bar (module docstring)."""
    _, p, m, v, plp = got
    lr, bc1, bc2 = (float(x) for x in hyper[:3].cpu())
    b1, b2, eps, wd = f32(B1), f32(B2), f32(EPS), f32(WD)
    worst = 0.0
    for s, e in stepped:
        gs = gsrc[s:e].double().cpu() * grad_scale
        p0, m0, v0 = (t[s:e].double().cpu() for t in (case.p0, case.m0, case.v0))
        idx = torch.arange(s, e, dtype=torch.float64)
        pd = torch.where(idx < case.n_decay, p0 * (1 - lr * wd), p0)
        m1 = b1 * m0 + (1 - b1) * gs
        v1 = b2 * v0 + (1 - b2) * gs * gs
        den = v1.sqrt() / math.sqrt(bc2) + eps
        q = m1 / den
        p1 = pd - (lr / bc1) * q
        bar_m = 3 * U * ((b1 * m0).abs() + ((1 - b1) * gs).abs())
        bar_v = 4 * U * (b2 * v0 + (1 - b2) * gs * gs)
        rel_d = torch.where(v1 > 0, bar_v / (2 * v1), torch.zeros_like(v1)) + 4 * U
        bar_q = bar_m / den + q.abs() * (rel_d + U)
        bar_p = 3 * U * p0.abs() + (lr / bc1) * (bar_q + 2 * U * q.abs()) + U * p1.abs()
        for t, ref, bar in ((p, p1, bar_p), (m, m1, bar_m), (v, v1, bar_v)):
            err = (t[s:e].double().cpu() - ref).abs()
            worst = max(worst, float((err / (bar + 1e-300)).max()))
        assert torch.equal(plp[s:e], p[s:e].to(plp.dtype)), "p_lp is not p rounded to the shadow format"
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    record_parity(f"fused_adamw_fp64_over_bar_{key}", round(_WORST[key], 4))
    assert worst <= 1.0, f"fp64 error {worst:.3f} x the bar"
    return worst


def assert_bufs_equal(a, b, names=("g", "p", "m", "v", "p_lp")):
    for x, y, nm in zip(a, b, names):
        if not torch.equal(x, y):
            bad = (x != y).nonzero().flatten()
            raise AssertionError(f"{nm} differs at {bad.numel()} elements, first {bad[:8].tolist()}")


def shapes_for(tile, seed):
    """Three or four weight-gradient problems (n_out, k_in, bias gradient?) for a tile: ragged edges on the ring tiles (multiples of 8,
    not of the tile's height or width), whole tiles on 256 x 256."""
    if tile == 256256:
        return [(512, 256, True), (256, 768, False), (256, 256, True)], 192
    return [(200, 136, True), (72, 264, False), (136, 48, True), (328, 96 if seed % 2 else 104, False)], 192


def decay_inside(case, j):
    """n_decay inside problem j: off a row boundary and off an 8-element boundary."""
    o, i, _ = case.shapes[j]
    return case.offs[j] + (o // 2) * i + i // 2 + 3


# ---------------------------------------------------------------------------------------------------------- epilogue form
@pytest.mark.parametrize("dtype", [BF, FH], ids=DT.get)
@pytest.mark.parametrize("tile", TILES)
def test_epilogue_form_equals_the_separate_launch_and_fp64(ops, tile, dtype):
    """skyemb_gemm_group_plan_adamw on every tile and format: p, m, v, p_lp bit for bit equal to the plain group + ops.adamw, within
    the fp64 bar; bias gradients equal the plain group's; g_base is neither read nor written for the problems (sentinels stay)."""
    shapes, T = shapes_for(tile, 1)
    c = Case(ops, tile, dtype, shapes, T, seed=tile % 997 + (dtype == FH))
    c.n_decay = decay_inside(c, 1)
    hyper = hyper_for(3)
    gref, dbs_ref = c.plain()
    ref = c.state()
    c.reference(ref, c.ranges, gref, hyper)
    got = c.state()
    dbs = c.bias_bufs()
    grp = ops.GemmGroup(c.problems(got[0], dbs), DEV, tile=tile, adamw=c.desc(got, hyper))
    assert grp.ok and grp.info.tile == tile and grp.total_blocks == grp.tile_blocks
    grp.launch()
    torch.cuda.synchronize()
    assert_bufs_equal(got, ref)
    assert torch.equal(got[0], c.g0)                                  # the gradient buffer is untouched
    for a, b in zip(dbs, dbs_ref):
        assert (a is None and b is None) or torch.equal(a, b)
    fp64_check(c, got, c.ranges, gref, hyper, f"epilogue_{DT[dtype]}")


@pytest.mark.parametrize("dtype", [BF, FH], ids=DT.get)
@pytest.mark.parametrize("tile", TILES)
def test_epilogue_form_replay_reads_the_step_scalars_from_the_device(ops, tile, dtype):
    """One planned group launched twice with ops.set_scalars changing lr, bc1, bc2 in between (how a graph replay reads the step's
    scalars) == two ops.adamw steps with those scalars."""
    shapes, T = shapes_for(tile, 2)
    c = Case(ops, tile, dtype, shapes, T, seed=31 + tile % 991)
    c.n_decay = decay_inside(c, 0)
    hyper = hyper_for(1)
    gref, _ = c.plain()
    ref = c.state()
    got = c.state()
    dbs = c.bias_bufs()                                  # (the planned blob holds raw pointers: the buffers must outlive the launches)
    grp = ops.GemmGroup(c.problems(got[0], dbs), DEV, tile=tile, adamw=c.desc(got, hyper))
    assert grp.ok
    steps = [(2e-3, 1 - B1, 1 - B2), (7e-4, 1 - B1 ** 2, 1 - B2 ** 2)]
    for lr, bc1, bc2 in steps:
        ops.set_scalars(hyper, lr, bc1, bc2)
        c.reference(ref, c.ranges, gref, hyper)
        ops.set_scalars(hyper, lr, bc1, bc2)
        grp.launch()
    torch.cuda.synchronize()
    assert_bufs_equal(got, ref)
    assert not torch.equal(got[1], c.p0)


# -------------------------------------------------------------------------------------------------------------- side form
# (side length in 8-element pieces, side workgroups): one piece; shorter than one pass of 256 workgroups; not a multiple of
# blocks x threads x U pieces; a few million elements; a single workgroup
SIDE_CASES = [(1, 7), (1000, 256), (7 * 512 * 4 * 3 + 123, 7), (375_001, 256), (5003, 1)]


@pytest.mark.parametrize("side_case", SIDE_CASES, ids=lambda s: f"{s[0]}x8_on{s[1]}")
@pytest.mark.parametrize("own", [0, 1])
@pytest.mark.parametrize("dtype", [BF, FH], ids=DT.get)
@pytest.mark.parametrize("tile", TILES)
def test_side_form_equals_the_separate_launch_and_fp64(ops, tile, dtype, own, side_case):
    """skyemb_gemm_group_plan_side_adamw: the side slice [lo, hi) (gradients pre-stored in g_base, n_decay inside it) is stepped
    bit for bit as ops.adamw steps it; own_step = 1: the tiles too, g untouched for them; own_step = 0: the tiles' gradients are
    stored equal to the plain group's and their p / m / v / p_lp stay untouched.  Gaps keep their sentinels."""
    pieces, blocks = side_case
    shapes, T = shapes_for(tile, 3)
    c = Case(ops, tile, dtype, shapes, T, seed=pieces % 1009 + tile % 13 + 5 * own, side_len=8 * pieces)
    lo, hi = c.side
    c.n_decay = lo + 8 * (pieces // 2) + (5 if pieces > 1 else 3)
    hyper = hyper_for(4)
    gref, dbs_ref = c.plain()
    ref = c.state()
    stepped = [(lo, hi)] + (c.ranges if own else [])
    c.reference(ref, stepped, gref, hyper)
    if not own:
        for s, e in c.ranges:
            ref[0][s:e] = gref[s:e]                                   # stored, not stepped
    got = c.state()
    dbs = c.bias_bufs()
    grp = ops.GemmGroup(c.problems(got[0], dbs), DEV, tile=tile, adamw=c.desc(got, hyper), side=(own, lo, hi, blocks))
    assert grp.ok and grp.info.tile == tile and grp.total_blocks == grp.tile_blocks + blocks
    grp.launch()
    torch.cuda.synchronize()
    assert_bufs_equal(got, ref)
    for a, b in zip(dbs, dbs_ref):
        assert (a is None and b is None) or torch.equal(a, b)
    fp64_check(c, got, stepped, gref, hyper, f"side_{DT[dtype]}")


def test_side_form_with_an_empty_range(ops):
    """side = (own_step, lo, lo, 0) is allowed: with own_step = 1 it is the epilogue form, nothing else moves."""
    shapes, T = shapes_for(128064, 0)
    c = Case(ops, 128064, BF, shapes, T, seed=77)
    c.n_decay = decay_inside(c, 2)
    hyper = hyper_for(2)
    gref, _ = c.plain()
    ref = c.state()
    c.reference(ref, c.ranges, gref, hyper)
    got = c.state()
    dbs = c.bias_bufs()
    grp = ops.GemmGroup(c.problems(got[0], dbs), DEV, tile=128064, adamw=c.desc(got, hyper), side=(1, 64, 64, 0))
    assert grp.ok and grp.total_blocks == grp.tile_blocks
    grp.launch()
    torch.cuda.synchronize()
    assert_bufs_equal(got, ref)


# -------------------------------------------------------------------------------------------- both side jobs in one launch
@pytest.mark.parametrize("own", [0, 1])
@pytest.mark.parametrize("dtype", [BF, FH], ids=DT.get)
@pytest.mark.parametrize("tile", TILES)
def test_layernorm_and_optimiser_side_jobs_share_one_launch(ops, tile, dtype, own):
    """A side-form group with a LayerNorm backward attached (the engine's normal combination: the first n_ln side workgroups take
    LayerNorm rows, the rest the optimiser's slice).  Row count 337: 85 four-wave blocks, so a side workgroup of two blocks is half
    used.  LayerNorm outputs and partial table == ops.layernorm_bwd, the side slice == ops.adamw, the tiles stepped or stored."""
    from sky_embeddings_amd._lib import BF16, F16
    code = BF16 if dtype == BF else F16
    M, D = 337, 192
    g = torch.Generator().manual_seed(tile % 1000 + own)
    x = torch.randn(M, D, generator=g).to(DEV)
    dy = torch.randn(M, D, generator=g).to(DEV, dtype)
    gam = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    g_in = torch.randn(M, D, generator=g).to(DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.layernorm_fwd(x, gam, torch.zeros(D, device=DEV), torch.empty(M, D, device=DEV, dtype=dtype), mean, rstd, M, D, 1e-6)
    nb = ops.layernorm_bwd_blocks(M)
    go_a, glp_a, part_a = g_in.clone(), torch.empty(M, D, device=DEV, dtype=dtype), torch.full((2, nb, D), NAN, device=DEV)
    ops.layernorm_bwd(dy, x, gam, mean, rstd, go_a, go_a, glp_a, part_a, None, None, M, D, code)
    shapes, T = shapes_for(tile, 4)
    c = Case(ops, tile, dtype, shapes, T, seed=91 + own, side_len=8 * 20011)
    lo, hi = c.side
    c.n_decay = lo + 8 * 777 + 1
    hyper = hyper_for(5)
    gref, dbs_ref = c.plain()
    ref = c.state()
    stepped = [(lo, hi)] + (c.ranges if own else [])
    c.reference(ref, stepped, gref, hyper)
    if not own:
        for s, e in c.ranges:
            ref[0][s:e] = gref[s:e]
    got = c.state()
    dbs = c.bias_bufs()
    go_b, glp_b, part_b = g_in.clone(), torch.full((M, D), -3.0, device=DEV, dtype=dtype), torch.full((2, nb, D), NAN, device=DEV)
    blocks = 256
    grp = ops.GemmGroup(c.problems(got[0], dbs), DEV, tile=tile, adamw=c.desc(got, hyper), side=(own, lo, hi, blocks),
                        ln_bwd=dict(dy=dy, x=x, gamma=gam, mean=mean, rstd=rstd, g_in=go_b, g_out=go_b, g_lp=glp_b, part=part_b, M=M, D=D))
    per_wg = 1 if tile == 64064 else 2
    assert grp.ok and grp.ln_side and grp.total_blocks == grp.tile_blocks + blocks + (nb + per_wg - 1) // per_wg
    grp.launch()
    torch.cuda.synchronize()
    assert torch.equal(go_a, go_b) and torch.equal(glp_a, glp_b) and torch.equal(part_a, part_b)
    assert_bufs_equal(got, ref)
    for a, b in zip(dbs, dbs_ref):
        assert (a is None and b is None) or torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("tile", TILES)
def test_fused_plans_refuse_what_they_cannot_step(ops, tile):
    """plan_adamw and plan_side_adamw (own_step 0 and 1) refuse -- ok False or an error -- and launch nothing for: a side range of
    partial 8-element pieces, a non-empty range with no workgroups (or an empty one with some), a problem with bias / out / act /
    alpha != 1, an out_f32 below g_base or at an offset from it not divisible by 8, a k-contiguous operand."""
    from sky_embeddings_amd._lib import ACT_GELU, KC, RC
    shapes, T = shapes_for(tile, 5)
    c = Case(ops, tile, BF, shapes, T, seed=3)
    c.n_decay = 0
    o, i, _ = shapes[0]
    dy, xx = c.dys[0], c.xs[0]
    hyper = hyper_for(1)
    bufs = c.state()
    base = bufs[0][8:]                                   # g_base 8 elements into the buffer: element 0 lies below it
    desc = c.desc(bufs, hyper)
    desc.g_base = base.data_ptr()

    def wgrad(out_f32, **kw):
        return ops.gemm_args(dy, xx, M=o, N=i, K=T, a_layout=RC, b_layout=RC, lda=o, ldb=i, out_f32=out_f32, **kw)

    def refused(args, side):
        before = ops.gemm_launch_counts()["group"]
        try:
            ok = ops.GemmGroup(args, DEV, tile=tile, adamw=desc, side=side).ok
        except Exception:
            ok = False
        return not ok and ops.gemm_launch_counts()["group"] == before

    at = base[64:64 + o * i].view(o, i)
    flawed = {
        "bias": [wgrad(at, bias=torch.zeros(i, device=DEV))],
        "out": [wgrad(at, out=torch.empty(o, i, device=DEV, dtype=BF))],
        "act": [wgrad(at, act=ACT_GELU)],
        "alpha": [wgrad(at, alpha=0.5)],
        "below_g_base": [wgrad(bufs[0][:o * i].view(o, i))],
        "offset_not_8": [wgrad(base[4:4 + o * i].view(o, i))],
        # a data-gradient (KC.RC) problem beside a weight gradient
        "kc": [wgrad(at), ops.gemm_args(xx, dy, M=T, N=o, K=64, a_layout=KC, b_layout=RC, lda=i, ldb=o,
                                       out_f32=base[o * i + 64:o * i + 64 + T * o].view(T, o))],
    }
    sides = [None, (0, 1024, 2048, 7), (1, 1024, 2048, 7)]
    for side in sides:                                   # the well-formed group is taken: the refusals below are the flaws'
        assert ops.GemmGroup([wgrad(at)], DEV, tile=tile, adamw=desc, side=side).ok, side
    fails = [(label, side) for side in sides for label, args in flawed.items() if not refused(args, side)]
    for own in (0, 1):
        for bad in ((own, 1024, 1028, 7), (own, 1020, 2048, 7), (own, 1024, 2048, 0), (own, 1024, 1024, 3)):
            if not refused([wgrad(at)], bad):
                fails.append(("range", bad))
    assert not fails, fails
    torch.cuda.synchronize()
    assert_bufs_equal(bufs, c.state())                  # nothing touched the flat buffers


# ------------------------------------------------------------------------------------------------------ engine-level placement
_TINY = dict(img_size=64, patch_size=16, in_chans=5, embed_dim=192)


def _run_steps(dtype, fused, policy, steps=3, B=64):
    from sky_embeddings_amd.engine import MAEEngine
    from sky_embeddings_amd.model_config import config_for
    from sky_embeddings_amd.optim import CosineLR, FusedAdamW
    from sky_embeddings_amd.train_step import TrainStep
    cfg = config_for("tiny", **_TINY)
    g = torch.Generator().manual_seed(0)
    imgs = torch.randn(B, 5, 64, 64, generator=g).to(DEV)
    noise = torch.rand(steps, B, cfg.num_patches, generator=g).to(DEV)
    eng = MAEEngine(cfg, compute_dtype=dtype, seed=1)
    opt = FusedAdamW(eng, lr=1e-3, weight_decay=0.05)
    step = TrainStep(eng, opt, CosineLR(opt, 100), B, external_noise=True, fused_adamw=fused, adamw_side=policy)
    assert step.fused_adamw == fused and step.graphs is not None
    losses = []
    for t in range(steps):
        step.noise.copy_(noise[t])
        losses.append(step(imgs).clone())
    torch.cuda.synchronize()
    st = eng.store
    return step, eng, [float(x) for x in losses], [t.clone() for t in (st.p, st.m, st.v, st.p_lp)]


@pytest.fixture(scope="module")
def separate_runs():
    return {dt: _run_steps(dt, False, None)[2:] for dt in (BF, FH)}


@pytest.mark.parametrize("policy", ["0", "1", "auto", "dec", "enc"])
@pytest.mark.parametrize("dtype", [BF, FH], ids=DT.get)
def test_every_placement_policy_equals_the_separate_optimiser_launch(separate_runs, dtype, policy):
    """Graph-mode TrainStep(fused_adamw=True, adamw_side=policy) on the tiny config: losses, p, m, v and p_lp bit-identical to the
    separate optimiser launch; the side jobs are placed as the policy says; the fused ranges and _rest() split [0, n) exactly."""
    step, eng, losses, state = _run_steps(dtype, True, policy)
    ref_losses, ref_state = separate_runs[dtype]
    assert step.adamw_side == policy
    w = eng._ws[step._ws_key]
    n_groups = sum(1 for grp in w["wgrad_groups"].values() if grp is not None)
    assert n_groups >= 4 and len(w["wgrad_groups_adamw"]) == n_groups
    launches = w["adamw_side_launches"]
    if policy == "0":
        assert launches == 0
    elif policy == "1":
        assert launches == n_groups - 1
    elif policy in ("dec", "enc"):
        assert launches > 0
    # which launch carries which block: launch k carries the step of launch k - 1's block (header words 3 = side workgroups and
    # 4-7 = the slice [lo, hi) of the planned blob) exactly where the policy says -- "auto": where the launch's tiles leave a quarter
    # of the device's workgroup slots free
    order = [p for p in eng._wgrad_launch_order(w) if w["wgrad_groups"].get(p) is not None]
    ncu = torch.cuda.get_device_properties(DEV).multi_processor_count
    per_cu = {256256: 1, 128128: 2, 9128128: 1, 128064: 2, 64064: 3}
    for k, prefix in enumerate(order):
        grp0 = w["wgrad_groups"][prefix]
        want = k > 0 and (policy == "1" or (policy == "dec" and prefix.startswith("decoder_blocks")) or
                          (policy == "enc" and prefix.startswith("blocks")) or
                          (policy == "auto" and grp0.tile_blocks <= 0.76 * ncu * per_cu[grp0.info.tile]))
        blob = w["wgrad_groups_adamw"][prefix].blob.cpu()
        side_wgs, rng = int(blob[:16].view(torch.int32)[3]), tuple(blob[16:32].view(torch.int64).tolist())
        assert (side_wgs > 0) == want, (prefix, side_wgs)
        if want:
            assert rng == eng._block_weight_span(order[k - 1]), (prefix, rng)
    assert launches == sum(int(w["wgrad_groups_adamw"][p].blob[12:16].view(torch.int32).item() > 0) for p in order)
    if policy == "auto":
        record_parity(f"fused_adamw_auto_side_launches_tiny_{DT[dtype]}", dict(side_launches=launches, groups=n_groups))
    # every parameter is stepped exactly once: fused ranges + the ordinary launch's ranges tile [0, n)
    parts = sorted(list(eng.fused_adamw_ranges(w)) + list(step._rest()))
    assert parts[0][0] == 0 and parts[-1][1] == eng.store.n
    assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(parts, parts[1:])), parts
    assert losses == ref_losses
    for k, (a, b) in enumerate(zip(state, ref_state)):
        assert torch.equal(a, b), ("p", "m", "v", "p_lp")[k]


# --------------------------------------------------------------------------------------------------------- loss-scale pinning
@pytest.mark.parametrize("graph", [True, False])
def test_an_eager_forward_between_steps_leaves_the_baked_loss_scale_alone(graph):
    """fp16: a fused TrainStep at B = 64 pins the loss scale it bakes into the loss kernel and the fused launches' grad_scale.  An
    eager forward_train on 20 images between two steps (a validation pass on a ragged batch) must not re-plan it: the next step
    runs, the scale and the optimiser's grad_scale are unchanged, and the parameters equal those of a run without the forward."""
    from sky_embeddings_amd.engine import MAEEngine
    from sky_embeddings_amd.model_config import config_for
    from sky_embeddings_amd.optim import CosineLR, FusedAdamW
    from sky_embeddings_amd.train_step import TrainStep
    cfg = config_for("tiny", **_TINY)
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(64, 5, 64, 64, generator=g).to(DEV)
    val = torch.randn(20, 5, 64, 64, generator=g).to(DEV)
    noise = torch.rand(2, 64, cfg.num_patches, generator=g).to(DEV)
    out = []
    for eager_forward in (False, True):
        eng = MAEEngine(cfg, compute_dtype=FH, seed=1)
        opt = FusedAdamW(eng, lr=1e-3, weight_decay=0.05)
        step = TrainStep(eng, opt, CosineLR(opt, 100), 64, use_graph=graph, external_noise=True, fused_adamw=True)
        assert step.fused_adamw
        scale, gscale = eng.loss_scale, opt.grad_scale
        step.noise.copy_(noise[0])
        step(imgs)
        if eager_forward:
            loss, _, _ = eng.forward_train(val, 0.75, torch.rand(20, cfg.num_patches, device=DEV))
            torch.cuda.synchronize()
            assert math.isfinite(float(loss))
        step.noise.copy_(noise[1])
        step(imgs)
        torch.cuda.synchronize()
        assert eng.loss_scale == scale and opt.grad_scale == gscale
        st = eng.store
        out.append([t.clone() for t in (st.p, st.m, st.v, st.p_lp)])
    for a, b in zip(*out):
        assert torch.equal(a, b)
