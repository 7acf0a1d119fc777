"""CPU checks of tests/rowwise_reference.py: for every case of the GPU tables the fp32 emulation of the kernel stays under the
derived bar and above a floor (a bar ten thousand times too loose fails), subtly wrong kernels (the mutants) exceed it, and the fp64
statements agree with the committed oracle and with torch where they overlap.

FLOORS: one tenth of the smallest worst err/bar the emulation reaches in a family, measured on the CPU (the ranges are in the
reference module's docstring).  16-bit outputs, dominated by h |r|, land near 1; fp32 sums far lower (worst-case n u bounds).
"""
import math

import pytest
import torch

from oracle import mae_oracle as mo
from tests import rowwise_reference as rr
from tests.rowwise_reference import BF, F16, F32

FLOORS = {"ln_fwd/mean": 9.9e-6, "ln_fwd/rstd": 1.0e-6, "ln_fwd/y32": 2.3e-4, "ln_fwd/y": 0.074,
          "ln_bwd/g_out": 5.2e-4, "ln_bwd/g_lp": 0.057, "ln_bwd/g_lp/f32": 5.2e-4, "ln_bwd/part": 0.011, "ln_bwd/dgamma": 6.4e-5,
          "ln_bwd/dbeta": 2.2e-5, "ln_reduce/out": 9.6e-4,
          "adamw/p": 0.049, "adamw/m": 0.042, "adamw/v": 0.029, "adamw/p_lp": 0.097, "adamw/p_lp/f32": 0.097,
          "loss/loss": 1.1e-7, "loss/ws": 7.0e-3, "loss/dpred32": 8.8e-4, "loss/dpred": 0.019,
          "colsum/out": 8.4e-6, "rowsum/partial": 0.037, "rowsum/out": 7.3e-5}


def held(family, ratios, lp32=()):
    """Every ratio <= 1 and above its family's floor (names in lp32: a shadow / copy stored in fp32, with the fp32 floor)."""
    for name, x in ratios.items():
        key = f"{family}/{name}" + ("/f32" if name in lp32 else "")
        print(f"{key} {x:.4g}")
        assert x <= 1.0, (key, ratios)
        assert x >= FLOORS[key], (key, x, FLOORS[key])


# ------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_fwd_ratios(c, mutant=None):
    t = rr.ln_inputs(c)
    ref, err = rr.ln_fwd_reference(t)
    bars = rr.ln_fwd_bars(ref, err, c.dtype)
    e = rr.ln_fwd_emulate(t, c.dtype, mutant=mutant)
    return {n: rr.ratio(e[n], ref["y" if n == "y32" else n], bars[n]) for n in ("mean", "rstd", "y32", "y")}


def ln_bwd_ratios(c, variant, mutant=None):
    t = rr.ln_inputs(c)
    nblk = rr.ln_bwd_blocks(c.M)
    ref, err = rr.ln_bwd_reference(t, variant, nblk)
    bars = rr.ln_bwd_bars(ref, err, c.dtype)
    e = rr.ln_bwd_emulate(t, variant, nblk, c.dtype, mutant=mutant)
    return {n: rr.ratio(e[n], ref["g_out" if n == "g_lp" else n], bars[n]) for n in ("g_out", "g_lp", "part", "dgamma", "dbeta")}


@pytest.mark.parametrize("c", [c for c in rr.LN_CASES if c.kind != "bwd"], ids=rr.ln_id)
def test_layernorm_forward_emulation_meets_the_bar(c):
    r = ln_fwd_ratios(c)
    if c.dtype == F32:
        r.pop("y")                                   # (an fp32 y is y32)
    held("ln_fwd", r)


@pytest.mark.parametrize("c,variant", rr.ln_bwd_cases(), ids=lambda v: rr.ln_id(v) if isinstance(v, rr.LN) else v)
def test_layernorm_backward_emulation_meets_the_bar(c, variant):
    r = ln_bwd_ratios(c, variant)
    if c.dtype != F32 and not variant.startswith("dy32") and c.M < 16 and r["dbeta"] == 0.0:
        r.pop("dbeta")                               # (a handful of 16-bit values: their fp32 sum is often exact)
    held("ln_bwd", r, lp32=("g_lp",) if c.dtype == F32 else ())


def test_layernorm_offset_rows_widen_the_bar_by_their_mean():
    """The cancellation term: x = 300 + randn against x = randn at the same shape, gamma and beta -- the bar of y is wider by
    about the ratio of the rows' magnitudes (|x| + |mean| ~ 600 against ~ 1), and the emulation still stays under it while its
    error really is two orders larger than a centred row's."""
    c = next(c for c in rr.LN_CASES if c.kind == "offset")
    t = rr.ln_inputs(c)
    t0 = dict(t, x=t["x"] - 300.0)
    out = {}
    for name, tt in (("offset", t), ("centred", t0)):
        ref, err = rr.ln_fwd_reference(tt)
        e = rr.ln_fwd_emulate(tt, F32)
        out[name] = (float(err["y"].median()), float((e["y32"] - ref["y"]).abs().max()))
    assert 100 < out["offset"][0] / out["centred"][0] < 1000, out
    assert out["offset"][1] > 30 * out["centred"][1], out


def test_layernorm_mutants_exceed_the_bar():
    for mutant in rr.LN_FWD_MUTANTS:
        cases = [c for c in rr.LN_CASES if c.kind != "bwd" and (mutant != "ragged" or (c.D // 4) % 64)]
        over = [rr.ln_id(c) for c in cases if max(ln_fwd_ratios(c, mutant).values()) > 1.0]
        print(mutant, over)
        assert over, mutant
    for mutant in rr.LN_BWD_MUTANTS:
        over = [rr.ln_id(c) for c in rr.LN_CASES if max(ln_bwd_ratios(c, "gin-glp", mutant).values()) > 1.0]
        print(mutant, over)
        assert over, mutant
    # the contiguous assignment differs only where a block walks more than one round of rows, and only in `part`
    big = next(c for c in rr.LN_CASES if c.kind == "bwd")
    r = ln_bwd_ratios(big, "gin-glp", "contiguous")
    assert r["part"] > 1.0 and r["dgamma"] <= 1.0 and r["g_out"] <= 1.0, r


def test_layernorm_cases_reach_the_paths_they_name():
    nv = lambda D: (D + 255) // 256
    ds = {c.D for c in rr.LN_CASES}
    assert {nv(D) for D in ds} >= {1, 2, 6, 7, 8} and 2048 in ds
    assert any((D // 4) % 64 == 1 and nv(D) > 1 for D in ds)            # one live lane in the last slot (260, 1284)
    assert any(c.M % 4 for c in rr.LN_CASES)
    big = next(c for c in rr.LN_CASES if c.kind == "bwd")
    nblk = rr.ln_bwd_blocks(big.M)
    rows = torch.bincount(rr.ln_block_of_row(big.M, nblk), minlength=nblk)
    assert nblk == 289 and (big.M + 3) // 4 > rr.LN_BWD_CAP and set(rows.tolist()) >= {8, 5}     # waves with 2 and with 3 rows
    assert rr.ln_bwd_blocks(4352) == 544 and rr.ln_bwd_blocks(8320) == 520 and rr.ln_bwd_blocks(37) == 10      # (layernorm.hip)
    nb, D = rr.LN_REDUCE_SHAPE
    assert nb > 64 and nb % 32 == 6 and D % 32
    assert all(D % 4 or D > 2048 for D in rr.LN_REFUSED_D)


def test_layernorm_reduce_emulation_meets_the_bar():
    part = rr.ln_reduce_inputs()
    ref, bar = rr.colsum_reference(part)
    held("ln_reduce", {"out": rr.ratio(part.sum(0), ref, bar)})


def test_layernorm_statement_is_torch_layer_norm():
    for c in rr.LN_CASES:
        if c.kind == "bwd":
            continue
        t = rr.ln_inputs(c)
        ref, _ = rr.ln_fwd_reference(t)
        x = t["x"].double().requires_grad_(True)
        gam, bet = t["gamma"].double().requires_grad_(True), t["beta"].double().requires_grad_(True)
        y = torch.nn.functional.layer_norm(x, (c.D,), gam, bet, rr.f32(rr.LN_EPS))
        scale = float(y.detach().abs().max())
        assert float((ref["y"] - y.detach()).abs().max()) <= 1e-12 * scale, rr.ln_id(c)
        # the backward, from the statement's own fp64 mean / rstd
        y.backward(t["dy"].double())
        nblk = rr.ln_bwd_blocks(c.M)
        b, _ = rr.ln_bwd_reference(dict(t, mean=ref["mean"], rstd=ref["rstd"]), "nogin-glp", nblk)
        for got, want in ((b["g_out"], x.grad), (b["dgamma"], gam.grad), (b["dbeta"], bet.grad)):
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), rr.ln_id(c)


# ------------------------------------------------------------------------------------------------------------- AdamW
def aw_ratios(c, mutant=None):
    t = rr.aw_inputs(c)
    ref, err = rr.aw_reference(t, c)
    bars = rr.aw_bars(ref, err, c)
    e = rr.aw_emulate(t, c, mutant)
    return {n: rr.ratio(e[n], ref["p" if n == "p_lp" else n], bars[n]) for n in bars}


@pytest.mark.parametrize("c", rr.AW_CASES, ids=rr.aw_id)
def test_adamw_emulation_meets_the_bar(c):
    r = aw_ratios(c)
    if c.n < 100:
        assert max(r.values()) <= 1.0, r             # (eight elements: no floor)
    else:
        held("adamw", r, lp32=("p_lp",) if c.lp == F32 else ())


def test_adamw_mutants_exceed_the_bar():
    small = [c for c in rr.AW_CASES if c.n < 1 << 20]
    for mutant in rr.AW_MUTANTS:
        over = [rr.aw_id(c) for c in small if max(aw_ratios(c, mutant).values()) > 1.0]
        print(mutant, over)
        assert over, mutant
    # the boundary mutant is caught by the two cases whose boundary is inside a float4, not by the aligned ones
    q = {rr.aw_id(c): max(aw_ratios(c, "decay_quad").values()) > 1.0 for c in small}
    assert [c.n_decay % 4 != 0 for c in small] == list(q.values()), q


def test_adamw_cases_reach_the_paths_they_name():
    stride = 4096 * 256
    big = max(rr.AW_CASES, key=lambda c: c.n)
    n4 = big.n // 4
    assert n4 > 3 * stride and n4 - 3 * stride == 37                   # second trip, u = 1 live for 37 threads
    assert big.n_decay % 4 == 2 and 2 * stride <= big.n_decay // 4     # the boundary inside a float4 of the second trip
    assert all(c.n // 4 <= stride for c in rr.AW_CASES if c is not big)
    assert {c.n_decay for c in rr.AW_CASES} >= {0} and any(c.n_decay == c.n for c in rr.AW_CASES)
    assert any(c.lp is None for c in rr.AW_CASES) and any(c.lp == F32 and c.gdt == BF for c in rr.AW_CASES)
    assert any(c.gdt == F16 and c.zero_grad for c in rr.AW_CASES) and any(c.hyper for c in rr.AW_CASES)
    for c in rr.AW_CASES[:4]:
        t = rr.aw_inputs(c)
        ref, _ = rr.aw_reference(t, c)
        assert bool((ref["v"] == 0).any()) and bool((t["g"] == 0).any()), rr.aw_id(c)      # denom = eps somewhere
        assert bool(((t["g"] != 0) & (t["g"].abs() * c.grad_scale < 1e-19)).any()) or c.gdt == F16


def test_adamw_statement_is_the_oracle_step():
    c = rr.AW_CASES[1]
    t = rr.aw_inputs(c)
    ref, _ = rr.aw_reference(t, c)
    p, m, v = t["p"].clone(), t["m"].clone(), t["v"].clone()
    nd, a = c.n_decay, rr.ADAM
    mo.adamw_step(p[:nd], t["g"][:nd], m[:nd], v[:nd], a["step"], a["lr"], a["wd"])
    mo.adamw_step(p[nd:], t["g"][nd:], m[nd:], v[nd:], a["step"], a["lr"], 0.0)
    for got, want in ((ref["p"], p), (ref["m"], m), (ref["v"], v)):
        assert float((got - want.double()).abs().max()) <= 1e-6 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------------------- loss
def ls_ratios(c, mutant=None):
    t = rr.ls_inputs(c)
    ref, err, ill = rr.ls_reference(t, c)
    bars = rr.ls_bars(ref, err, c)
    e = rr.ls_emulate(t, c, mutant)
    out = {"loss": rr.ratio(e["loss"], ref["loss"], bars["loss"]), "ws": rr.ratio(e["ws"], ref["ws"], bars["ws"]),
           "dpred32": rr.ratio(e["dpred32"], ref["dpred"], bars["dpred32"], skip=ill)}
    if c.lp is not None:
        out["dpred"] = rr.ratio(e["dpred"], ref["dpred"], bars["dpred"], skip=ill)
    return out


@pytest.mark.parametrize("c", rr.LS_CASES, ids=rr.ls_id)
def test_loss_emulation_meets_the_bar(c):
    held("loss", ls_ratios(c))


@pytest.mark.parametrize("c", [c for c in rr.LS_CASES if c.l1], ids=rr.ls_id)
def test_l1_cases_have_no_ill_conditioned_sign(c):
    """From the statement alone: no masked, finite element of an L1 case has 0 < |tn - pred| <= its error bound; the only exact
    zeros are the two equal pixels under a zero prediction."""
    t = rr.ls_inputs(c)
    ref, err, ill = rr.ls_reference(t, c)
    assert int(ill.sum()) == 0
    L = (c.H // c.p) ** 2
    live = (t["mask"][..., None] != 0) & ~torch.isnan(rr.patchify(t["imgs"], c.p))
    zeros = live & (ref["dpred"][:, c.extra:] == 0)
    assert int(zeros.sum()) == (2 if c.mask == "rand" else 0) and (c.mask != "rand" or int(zeros[1, L - 1].sum()) == 2)


def test_loss_mutants_exceed_the_bar():
    for mutant in rr.LS_MUTANTS:
        cases = [c for c in rr.LS_CASES if c.l1 or mutant != "sign0"]
        over = [rr.ls_id(c) for c in cases if max(ls_ratios(c, mutant).values()) > 1.0]
        print(mutant, over)
        assert over, mutant


def test_loss_cases_reach_the_paths_they_name():
    pv = {c.C * c.p * c.p for c in rr.LS_CASES}
    assert 3072 in pv and any(x > 3072 for x in pv)
    assert any(c.B * (c.H // c.p) ** 2 > 256 for c in rr.LS_CASES)
    assert {c.extra for c in rr.LS_CASES} >= {0, 1, 2} and {c.lp for c in rr.LS_CASES} >= {BF, F16, None}
    assert any(c.dscale != 1 for c in rr.LS_CASES)
    for c in rr.LS_CASES:
        t = rr.ls_inputs(c)
        L = (c.H // c.p) ** 2
        ok = ~torch.isnan(rr.patchify(t["imgs"], c.p))
        assert int(ok[0, L - 1].sum()) == 2 and float(t["mask"][0, L - 1]) == 1.0            # two finite pixels, masked
        assert int(ok.sum(-1).min()) >= 2                                                    # no patch without a finite pixel
        assert bool((t["mask"] == 0).any())


def test_loss_statement_is_the_oracle_loss():
    """mo.forward_loss (fp32) on the geometry of test_masked_patch_loss, loss and gradient, to 1e-6 relative."""
    for l1 in (False, True):
        for C, H, p in ((5, 64, 16), (9, 32, 8)):
            c = rr.LS(4, C, H, p, 1, BF, l1)
            t = rr.ls_inputs(c)
            cfg = mo.MAEConfig(img_size=H, patch_size=p, in_chans=C, pixel_mean=rr.PIXEL_MEAN, pixel_std=rr.PIXEL_STD, norm_pix_loss=True,
                               loss_fn="L1" if l1 else "mse")
            pr = t["pred"][:, 1:].clone().requires_grad_(True)
            loss = mo.forward_loss(mo.norm_inputs(t["imgs"], cfg), pr, t["mask"], cfg, nan_safe=True)
            loss.backward()
            loss = loss.detach()
            ref, _, ill = rr.ls_reference(t, c)
            assert abs(float(ref["loss"]) - float(loss)) <= 1e-6 * abs(float(loss))
            keep = ~ill[:, 1:]
            d = (ref["dpred"][:, 1:] - pr.grad.double()).abs()[keep]
            assert float(d.max()) <= 1e-6 * float(pr.grad.abs().max()) * (30 if not l1 else 1), (l1, C, float(d.max()))


# ------------------------------------------------------------------------------------------------------------- reductions, copies
@pytest.mark.parametrize("c", rr.CS_CASES, ids=rr.cs_id)
def test_colsum_emulation_meets_the_bar(c):
    X = rr.cs_inputs(c)
    ref, bar = rr.colsum_reference(X)
    r = rr.ratio(X.sum(0), ref, bar)
    if c.M < 4:
        assert r <= 1.0                              # (three terms: the sum is often exact)
    else:
        held("colsum", {"out": r})


@pytest.mark.parametrize("c", rr.RS_CASES, ids=rr.rs_id)
def test_rowsum_select_emulation_meets_the_bar(c):
    x, sel = rr.rs_inputs(c)
    ref, bars = rr.rs_reference(x, sel)
    e = rr.rs_emulate(x, sel)
    r = {n: rr.ratio(e[n], ref[n], bars[n]) for n in ref}
    if c.sel == "zero":
        assert r == {"partial": 0.0, "out": 0.0} and float(bars["out"].max()) == 0.0
    elif c.B * c.L < 256:
        assert r["partial"] == 0.0                   # (one row per block: a copy)
        held("rowsum", {"out": r["out"]})
    else:
        held("rowsum", r)


def test_reduction_cases_reach_the_paths_they_name():
    assert any(c.ldx > c.N for c in rr.CS_CASES) and any(c.M < 4 for c in rr.CS_CASES) and any(c.N % 64 for c in rr.CS_CASES)
    n = sorted({c.B * c.L for c in rr.RS_CASES})
    assert n[0] < 256 < n[1] < 1024 < n[2] and any(c.D > 256 for c in rr.RS_CASES)
    assert rr.GATHER_D > 1024 and rr.FILL_D > 1024 and max(rr.CAST_N) // 4 - 4096 * 256 == 5
    x = rr.cast_inputs(max(rr.CAST_N))
    h, b = x.to(F16), x.to(BF)
    assert bool(torch.isinf(h).any()) and bool(torch.isinf(b).any()) and not bool(torch.isinf(x).any())
    sub = (h.float().abs() > 0) & (h.float().abs() < 2.0 ** -14)
    assert int(sub.sum()) > 100 and bool(((h == 0) & (x != 0)).any())
