"""GPU parity of the row-wise kernels around the GEMMs, ELEMENT BY ELEMENT: LayerNorm forward / backward / reduce, the flat-buffer
AdamW, the masked per-patch loss and the reductions and copies of frontend.hip go through the C ABI wrappers of
sky_embeddings_amd/ops.py, and every element of every output -- mean, rstd, the partial-sum table, the zero rows and the zeroed
gradients included -- is held to the fp64 statement and the derived bar of tests/rowwise_reference.py (pinned on the CPU by
tests/test_rowwise_reference_cpu.py, which also shows that subtly wrong kernels exceed the bar).  The cases are the smallest
shapes at which each instantiation and branch is live; the case ids name them.

Outputs start as NaN where the kernel promises to write everywhere (a NaN left behind fails the bar) and carry a sentinel where it
must not write: the rows of unmasked patches under fill_mask_tokens, the padding columns of colsum's operand are NaN (a read there
poisons a sum).  Each test records its worst err/bar (helpers.record_parity "rowwise_elementwise").
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import rowwise_reference as rr
from tests.helpers import record_parity
from tests.rowwise_reference import BF, F16, F32

DEV = "cuda"
NAN = float("nan")
SENT = 12.5


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
    record_parity("rowwise_elementwise", {k: round(v, 4) for k, v in sorted(w.items())})


def dev(t, dtype=None):
    return None if t is None else (t.to(DEV) if dtype is None else t.to(DEV, dtype))


def nans(*shape, dtype=F32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def hold(worst, family, name, ratios):
    """Print and record the ratios of one case; all must be <= 1."""
    print(f"{name} err/bar {ratios}")
    for k, r in ratios.items():
        worst[f"{family}/{k}"] = max(worst.get(f"{family}/{k}", 0.0), r)
    bad = {k: r for k, r in ratios.items() if not r <= 1.0}
    assert not bad, (name, ratios)


def report(got, ref, bar, n=5):
    """The worst elements of a failing output: (index, got, ref, err / bar)."""
    r = ((got.double() - ref).abs() / bar).nan_to_num(nan=float("inf")).flatten()
    top = torch.topk(r, min(n, r.numel()))
    return [(tuple(int(v) for v in torch.unravel_index(i, ref.shape)), float(got.flatten()[i]), float(ref.flatten()[i]), float(x))
            for x, i in zip(top.values, top.indices)]


# ------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.fixture(scope="module")
def ln_data():
    cache = {}

    def get(c):
        if c not in cache:
            cache[c] = rr.ln_inputs(c)
        return cache[c]
    return get


@pytest.mark.parametrize("c,variant", rr.ln_fwd_cases(), ids=lambda v: rr.ln_id(v) if isinstance(v, rr.LN) else v)
def test_layernorm_forward(ops, worst, ln_data, c, variant):
    t = ln_data(c)
    ref, err = rr.ln_fwd_reference(t)
    bars = rr.ln_fwd_bars(ref, err, c.dtype)
    M, D = c.M, c.D
    y = nans(M, D, dtype=c.dtype) if variant == "y+y32" else None
    y32, mean, rstd = nans(M, D), nans(M), nans(M)
    ops.layernorm_fwd(dev(t["x"]), dev(t["gamma"]), dev(t["beta"]), y, mean, rstd, M, D, rr.LN_EPS, y32=y32, dtype=ops.dtype_code(c.dtype))
    torch.cuda.synchronize()
    got = {"mean": mean, "rstd": rstd, "y32": y32}
    if y is not None:
        got["y"] = y
    ratios = {n: rr.ratio(g.cpu(), ref["y" if n == "y32" else n], bars[n]) for n, g in got.items()}
    for n, r in ratios.items():
        if not r <= 1.0:
            print(n, report(got[n].cpu(), ref["y" if n == "y32" else n], bars[n]))
    hold(worst, "ln_fwd/" + rr.DT[c.dtype], f"{rr.ln_id(c)} {variant}", ratios)


def run_ln_bwd(ops, t, c, variant, nblk):
    M, D = c.M, c.D
    dy = dev(t["dy32"]) if variant.startswith("dy32") else dev(t["dy"], c.dtype)
    gin = "nogin" not in variant
    g_out = dev(t["g_in"].clone()) if gin else nans(M, D)              # (with an incoming gradient: in place, as the engine runs it)
    g_lp = None if "noglp" in variant else nans(M, D, dtype=c.dtype)
    part, dgam, dbet = nans(2, nblk, D), nans(D), nans(D)
    ops.layernorm_bwd(dy, dev(t["x"]), dev(t["gamma"]), dev(t["mean"]), dev(t["rstd"]), g_out if gin else None, g_out, g_lp, part, dgam,
                      dbet, M, D, ops.dtype_code(c.dtype))
    torch.cuda.synchronize()
    got = {"g_out": g_out, "part": part, "dgamma": dgam, "dbeta": dbet}
    if g_lp is not None:
        got["g_lp"] = g_lp
    return got


@pytest.mark.parametrize("c,variant", rr.ln_bwd_cases(), ids=lambda v: rr.ln_id(v) if isinstance(v, rr.LN) else v)
def test_layernorm_backward(ops, worst, ln_data, c, variant):
    t = ln_data(c)
    nblk = rr.ln_bwd_blocks(c.M)
    assert ops.layernorm_bwd_blocks(c.M) == nblk
    ref, err = rr.ln_bwd_reference(t, variant, nblk)
    bars = rr.ln_bwd_bars(ref, err, c.dtype)
    got = run_ln_bwd(ops, t, c, variant, nblk)
    ratios = {n: rr.ratio(g.cpu(), ref["g_out" if n == "g_lp" else n], bars[n]) for n, g in got.items()}
    for n, r in ratios.items():
        if not r <= 1.0:
            print(n, report(got[n].cpu(), ref["g_out" if n == "g_lp" else n], bars[n]))
    hold(worst, "ln_bwd/" + rr.DT[c.dtype], f"{rr.ln_id(c)} {variant}", ratios)


def test_layernorm_reduce_batch_past_32_blocks(ops, worst):
    """skyemb_layernorm_bwd_reduce_batch on a [70, 100] table: 70 blocks over 32 row groups (6 of them hold 3 rows), 100 columns
    over four 32-wide workgroups (the last one ragged), against the fp64 column sums; a second, single-vector item of another
    width in the same launch."""
    part = rr.ln_reduce_inputs()
    nblk, D = part.shape
    pd = dev(torch.stack([part, -2.0 * part]))                          # [2, nblk, D]: dgamma and dbeta halves
    dgam, dbet, vec = nans(D), nans(D), nans(36)
    other = torch.randn(5, 36, generator=torch.Generator().manual_seed(3))
    od = dev(other)
    table = ops.ln_reduce_items([(pd, dgam, dbet, nblk, D), (od, vec, None, 5, 36)], DEV)
    ops.layernorm_bwd_reduce_batch(table, 0, 2)
    torch.cuda.synchronize()
    ref, bar = rr.colsum_reference(part)
    oref, obar = rr.colsum_reference(other)
    hold(worst, "ln_reduce", "reduce_batch 70x100", {"dgamma": rr.ratio(dgam.cpu(), ref, bar), "dbeta": rr.ratio(dbet.cpu(), -2.0 * ref, 2.0 * bar),
                                                     "vector": rr.ratio(vec.cpu(), oref, obar)})


@pytest.mark.parametrize("D", rr.LN_REFUSED_D)
def test_layernorm_refuses_widths_it_has_no_kernel_for(ops, D):
    M = 4
    x, gam = torch.zeros(M, D, device=DEV), torch.ones(D, device=DEV)
    y, mean, rstd = torch.full((M, D), SENT, device=DEV), nans(M), nans(M)
    with pytest.raises(Exception):
        ops.layernorm_fwd(x, gam, gam, y, mean, rstd, M, D, rr.LN_EPS)
    g_out, part = torch.full((M, D), SENT, device=DEV), nans(2, 1, D)
    with pytest.raises(Exception):
        ops.layernorm_bwd(x, x, gam, mean, rstd, None, g_out, None, part, None, None, M, D, ops.F32)
    torch.cuda.synchronize()
    assert bool((y == SENT).all()) and bool((g_out == SENT).all()) and bool(torch.isnan(mean).all())


def test_layernorm_backward_side_job_at_a_ragged_width(ops, worst):
    """A LayerNorm backward of D = 260 (two float4 slots, one live lane in the second) riding in a grouped weight-gradient launch
    (skyemb_gemm_group_attach_ln_bwd, gamma read from LDS) against the fp64 statement per element -- the stand-alone kernel and
    the side job share their text and would be wrong together -- and, bit for bit, against the stand-alone kernel."""
    from sky_embeddings_amd._lib import RC
    c = rr.LN(326, 260, BF, "std", "side job")
    t = rr.ln_inputs(c)
    M, D, n_out, k_in = c.M, c.D, 768, 192
    nblk = rr.ln_bwd_blocks(M)
    ref, err = rr.ln_bwd_reference(t, "gin-glp", nblk)
    bars = rr.ln_bwd_bars(ref, err, BF)
    alone = run_ln_bwd(ops, t, c, "gin-glp", nblk)
    g = torch.Generator().manual_seed(326)
    T = (M + 63) // 64 * 64
    dyw, xw = dev(torch.randn(T, n_out, generator=g), BF), dev(torch.randn(T, k_in, generator=g), BF)
    dW, db = torch.empty(n_out, k_in, device=DEV), torch.empty(n_out, device=DEV)
    g_out, g_lp, part = dev(t["g_in"].clone()), nans(M, D, dtype=BF), nans(2, nblk, D)
    rec = dict(dy=dev(t["dy"], BF), x=dev(t["x"]), gamma=dev(t["gamma"]), mean=dev(t["mean"]), rstd=dev(t["rstd"]), g_in=g_out, g_out=g_out,
               g_lp=g_lp, part=part, M=M, D=D)
    grp = ops.GemmGroup([ops.gemm_args(dyw, xw, M=n_out, N=k_in, K=T, a_layout=RC, b_layout=RC, lda=n_out, ldb=k_in, out_f32=dW, colsum_a=db)],
                        DEV, tile=0, ln_bwd=rec)
    assert grp.ok and grp.ln_side and grp.total_blocks > grp.tile_blocks          # (the plan accepts rows up to 768 wide)
    grp.launch()
    torch.cuda.synchronize()
    got = {"g_out": g_out, "g_lp": g_lp, "part": part}
    hold(worst, "ln_bwd/side", "side job 326x260", {n: rr.ratio(x.cpu(), ref["g_out" if n == "g_lp" else n], bars[n]) for n, x in got.items()})
    for n, x in got.items():
        assert torch.equal(x, alone[n]), n


# ------------------------------------------------------------------------------------------------------------- AdamW
@pytest.mark.parametrize("c", rr.AW_CASES, ids=rr.aw_id)
def test_adamw(ops, worst, c):
    """The reference and the comparison run on the device in fp64 (the capped-grid case holds 50 MB per buffer): only the worst
    ratio and the indices of failures come back."""
    t = {k: dev(v) for k, v in rr.aw_inputs(c).items()}
    ref, err = rr.aw_reference(t, c)
    bars = rr.aw_bars(ref, err, c)
    s = rr.aw_scalars()
    p, m, v = t["p"].clone(), t["m"].clone(), t["v"].clone()
    g = t["g"].to(c.gdt)
    p_lp = nans(c.n, dtype=c.lp) if c.lp is not None else None
    kw = dict(grad_scale=c.grad_scale, zero_grad=c.zero_grad)
    if c.hyper:
        hyper = dev(torch.tensor([s["lr"], s["bc1"], s["bc2"], 0.0]))
        ops.adamw(p, g, m, v, p_lp, c.n, c.n_decay, hyper, s["beta1"], s["beta2"], s["eps"], s["wd"], **kw)
    else:
        ops.adamw(p, g, m, v, p_lp, c.n, c.n_decay, None, s["beta1"], s["beta2"], s["eps"], s["wd"], lr=s["lr"], bc1=s["bc1"], bc2=s["bc2"], **kw)
    torch.cuda.synchronize()
    got = {"p": p, "m": m, "v": v}
    if p_lp is not None:
        got["p_lp"] = p_lp
        assert torch.equal(p_lp, p.to(c.lp)), "the shadow is not the rounded parameter"
    ratios = {}
    for n, x in got.items():
        r = (x.double() - ref["p" if n == "p_lp" else n]).abs() / bars[n]
        r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
        ratios[n] = float(r.max())
        if ratios[n] > 1.0:
            print(n, "failing indices", torch.nonzero(r > 1.0).flatten()[:16].tolist())
    assert torch.equal(g, torch.zeros_like(g) if c.zero_grad else t["g"].to(c.gdt)), "gradient buffer"
    hold(worst, "adamw", rr.aw_id(c), ratios)


# ------------------------------------------------------------------------------------------------------------- masked patch loss
@pytest.mark.parametrize("c", rr.LS_CASES, ids=rr.ls_id)
def test_masked_patch_loss(ops, worst, c):
    t = rr.ls_inputs(c)
    ref, err, ill = rr.ls_reference(t, c)
    bars = rr.ls_bars(ref, err, c)
    assert int(ill.sum()) == 0
    B, L, pv = c.B, (c.H // c.p) ** 2, c.C * c.p * c.p
    loss, ws = nans(1), nans(4 * B * L + 4)
    if c.lp is None:                                                   # `dtype` F32: the fp32 gradient goes to dpred, dpred32 = NULL
        dlp, d32, code = nans(B, L + c.extra, pv), None, ops.F32
    else:
        dlp, d32, code = nans(B, L + c.extra, pv, dtype=c.lp), nans(B, L + c.extra, pv), ops.dtype_code(c.lp)
    ops.masked_patch_loss(dev(t["imgs"]), dev(t["pred"]), dev(t["mask"]), loss, dlp, d32, code, ws, c.p, c.extra, rr.PIXEL_MEAN,
                          rr.PIXEL_STD, True, c.l1, dscale=c.dscale)
    torch.cuda.synchronize()
    got = {"loss": (loss.cpu(), ref["loss"]), "ws": (ws[:4 * B * L].reshape(B * L, 4).cpu(), ref["ws"])}
    if c.lp is None:
        got["dpred32"] = (dlp.cpu(), ref["dpred"])
    else:
        got["dpred32"], got["dpred"] = (d32.cpu(), ref["dpred"]), (dlp.cpu(), ref["dpred"])
    ratios = {n: rr.ratio(x, r, bars[n]) for n, (x, r) in got.items()}
    for n, r in ratios.items():
        if not r <= 1.0:
            print(n, report(got[n][0], got[n][1], bars[n]))
    assert float(ws[4 * B * L].cpu()) == float(loss.cpu())             # (the loss once more behind the per-patch records)
    hold(worst, "loss", rr.ls_id(c), ratios)


# ------------------------------------------------------------------------------------------------------------- reductions, copies
@pytest.mark.parametrize("c", rr.CS_CASES, ids=rr.cs_id)
def test_colsum(ops, worst, c):
    X = rr.cs_inputs(c)
    buf = nans(c.M, c.ldx, dtype=c.dtype)                               # padding columns beyond N: NaN
    buf[:, :c.N] = dev(X, c.dtype)
    out = torch.full((c.N + 8,), SENT, device=DEV)
    out[:c.N] = NAN
    ops.colsum(buf, c.M, c.N, out, ldx=c.ldx)
    torch.cuda.synchronize()
    ref, bar = rr.colsum_reference(X)
    assert bool((out[c.N:] == SENT).all())
    hold(worst, "colsum/" + rr.DT[c.dtype], rr.cs_id(c), {"out": rr.ratio(out[:c.N].cpu(), ref, bar)})


@pytest.mark.parametrize("c", rr.RS_CASES, ids=rr.rs_id)
def test_rowsum_select(ops, worst, c):
    x, sel = rr.rs_inputs(c)
    ld = c.D + 4
    buf = nans(c.B * (c.L + 1), ld)                                     # padding columns: NaN
    buf[:, :c.D] = dev(x.reshape(-1, c.D))
    part, out = nans(256, c.D), nans(c.D)
    ops.rowsum_select(buf, ld, dev(sel), 1, c.L, c.L + 1, c.B * c.L, c.D, part, out)
    torch.cuda.synchronize()
    ref, bars = rr.rs_reference(x, sel)
    hold(worst, "rowsum_select", rr.rs_id(c), {"partial": rr.ratio(part.cpu(), ref["partial"], bars["partial"]),
                                               "out": rr.ratio(out.cpu(), ref["out"], bars["out"])})


@pytest.mark.parametrize("name,lp,with32", rr.GATHER_CASES, ids=[g[0] for g in rr.GATHER_CASES])
def test_gather_rows(ops, name, lp, with32):
    D, n_src, n = rr.GATHER_D, 9, 13
    g = torch.Generator().manual_seed(D)
    src = torch.randn(n_src, D, generator=g) * torch.logspace(-6, 4, D)[None, :]
    idx = torch.tensor([3, 3, 0, 8, 5, 3, 8, 1, 0, 7, 7, 2, 8], dtype=torch.int32)          # repeated rows, first and last
    o32 = nans(n, D) if with32 else None
    olp = nans(n, D, dtype=lp) if lp is not None else None
    ops.gather_rows(dev(src), dev(idx), o32, olp, n, D)
    torch.cuda.synchronize()
    want = src[idx.long()]
    if with32:
        assert torch.equal(o32.cpu(), want)
    if lp is not None:
        assert torch.equal(olp.cpu(), want.to(lp))


def test_fill_mask_tokens(ops):
    B, L, Dd, E = 3, 7, rr.FILL_D, 2
    g = torch.Generator().manual_seed(Dd)
    mask = (torch.rand(B, L, generator=g) > 0.4).float()
    mask[0, 0], mask[B - 1, L - 1] = 1.0, 0.0
    mt, pos = torch.randn(Dd, generator=g), torch.randn(L + E, Dd, generator=g)
    x = torch.full((B, L + E, Dd), SENT, device=DEV)
    ops.fill_mask_tokens(x, dev(mask), dev(mt), dev(pos), B, L, Dd, n_extra=E)
    torch.cuda.synchronize()
    want = torch.full((B, L + E, Dd), SENT)
    want[:, E:][mask.bool()] = (mt + pos[E:]).expand(B, -1, -1)[mask.bool()]
    assert torch.equal(x.cpu(), want)                                   # the extra rows and the unmasked rows keep the sentinel


@pytest.mark.parametrize("n", rr.CAST_N)
@pytest.mark.parametrize("dtype", [BF, F16, F32], ids=["bf16", "f16", "f32"])
def test_cast(ops, dtype, n):
    x = dev(rr.cast_inputs(n))
    dst = torch.full((n + 8,), 1.0, device=DEV, dtype=dtype)
    ops.cast(x, dst, n)
    torch.cuda.synchronize()
    bits = torch.int32 if dtype == F32 else torch.int16
    want = x.cpu().to(dtype)                                            # (the host's conversion: to nearest even, subnormals kept)
    assert torch.equal(dst[:n].cpu().view(bits), want.view(bits))
    assert bool((dst[n:] == 1.0).all())
