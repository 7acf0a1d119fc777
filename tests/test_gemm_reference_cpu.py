"""CPU checks of tests/gemm_reference.py: the bar against the emulated kernel arithmetic for every case of the GPU table, E_CDF
against the emulated gelu_parts, the mutants (subtly wrong kernels, each of which must exceed the bar), and the case table against the
launch plan.

Worst err/bar of the round-to-nearest emulation, per case and output: 16-bit outputs within [0.05, 1] (bf16 0.83-1.00, fp16
0.26-0.99: the stored rounding h |r| is the bar's own leading term); fp32 outputs 0.0005-0.47 and column sums 0.0001-0.07 (the
fp32 terms are worst-case gamma_K bounds while real sums err like sqrt(K) u; highest at K = 20).
"""
import math

import pytest
import torch

from tests import gemm_reference as gr
from tests.gemm_reference import BF, F16, F32, KC, RC, CASES, Case, cid

BIAS = 0.1                    # the signed-bias threshold of tests/test_gemm_elementwise_gpu.py (as tests/test_attention_core_gpu.py)
SMALL = [c for c in CASES if c.M * c.N <= 1 << 20]
LARGE = [c for c in CASES if c.M * c.N > 1 << 20]


def ratios(c, mutant=None, t=None):
    t = t if t is not None else gr.inputs(c)
    st = gr.reference(c, t)
    b = gr.bars(c, st)
    e = gr.emulate(c, t, mutant)
    return {n: gr.ratio(e[n], st["ref"][n], b[n]) for n in st["ref"]}, st, b, e


@pytest.mark.parametrize("c", SMALL + LARGE, ids=cid)
def test_rne_emulation_meets_the_bar(c):
    r, *_ = ratios(c)
    for name, x in r.items():
        assert x <= 1.0, (name, r)
        if gr.stored_dtype(c, name) != F32:
            assert x >= 0.05, (name, r)


def test_e_cdf_bounds_the_emulated_gelu_parts():
    """Dense grid over [-9, 9]: the fp32 emulation of gelu_parts reaches about a third of E_CDF (cdf and dGELU factor), the erf form
    of gemm.hip about a quarter of its own."""
    x = torch.linspace(-9.0, 9.0, 1 << 21, dtype=torch.float64).float()
    xd = x.double()
    cdf, _ = gr.gelu_parts32(x)
    e_cdf = float((cdf.double() - gr.phi_cdf(xd)).abs().max())
    e_dg = float((gr.dgelu32(x, True).double() - gr.dgelu64(xd)).abs().max())
    print(f"gelu_parts emulation: cdf {e_cdf:.3g}, dgelu {e_dg:.3g}, E_CDF {gr.E_CDF_PIPE:.3g}")
    assert gr.E_CDF_PIPE / 8 < e_cdf < gr.E_CDF_PIPE / 2 and gr.E_CDF_PIPE / 8 < e_dg < gr.E_CDF_PIPE / 2
    # the gelu itself, relative to |x|: the contract of the absolute term
    assert float(((gr.gelu32(x, True).double() - gr.gelu64(xd)).abs() / xd.abs().clamp_min(1e-3)).max()) < gr.E_CDF_PIPE
    c32 = 0.5 * (1.0 + torch.erf(x * torch.tensor(0.70710678118654752440)))
    f_cdf = float((c32.double() - gr.phi_cdf(xd)).abs().max())
    f_dg = float((gr.dgelu32(x, False).double() - gr.dgelu64(xd)).abs().max())
    print(f"erf form: cdf {f_cdf:.3g}, dgelu {f_dg:.3g}, E_CDF {gr.E_CDF_ERFF:.3g}")
    assert gr.E_CDF_ERFF / 16 < f_cdf < gr.E_CDF_ERFF and gr.E_CDF_ERFF / 16 < f_dg < gr.E_CDF_ERFF
    # what the absolute term means below -4: the relative error of gelu(x) there is above fp16's unit roundoff
    far = (xd < -4) & (xd > -6)
    rel = ((gr.gelu32(x, True).double() - gr.gelu64(xd)).abs() / gr.gelu64(xd).abs())[far]
    assert float(rel.max()) > 2.0 ** -11


def smallest(pred):
    cs = [c for c in CASES if pred(c)]
    assert cs
    return min(cs, key=lambda c: (c.M * c.N * c.K, cid(c)))


lp = lambda c: c.dtype != F32 and c.kind == "randn" and gr.planned(c)["family"] in ("pipe", "splitk", "tile256")
MUTANT_CASE = {
    "gelu_rounded": lambda c: lp(c) and c.epi == "gelu",
    "tanh": lambda c: lp(c) and c.epi == "gelu",
    "bias_after": lambda c: lp(c) and c.epi == "gelu",
    "alpha_bias": lambda c: lp(c) and c.epi in ("full", "resid"),
    "resid_m": lambda c: lp(c) and c.epi == "full",
    "tab_dst": lambda c: lp(c) and c.epi == "full",
    "swap_k": lambda c: lp(c) and c.K >= 128,
}


@pytest.mark.parametrize("mutant", sorted(MUTANT_CASE))
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "f16"])
def test_mutant_exceeds_the_bar(mutant, dtype):
    c = smallest(lambda c: c.dtype == dtype and MUTANT_CASE[mutant](c))
    good, *_ = ratios(c)
    assert max(good.values()) <= 1.0
    bad, *_ = ratios(c, mutant)
    names = [n for n in bad if n != "out2"] if mutant in ("gelu_rounded", "tanh", "bias_after") else list(bad)
    assert max(bad[n] for n in names) > 1.0, (cid(c), bad)
    if mutant == "gelu_rounded":                  # ... by the margin the docstring states: ~ h |v| |gelu'| against fp32 terms
        assert bad["out"] > 1.5 and bad["out2"] <= 1.0, bad


@pytest.mark.parametrize("dtype", [F32, BF, F16], ids=["f32", "bf16", "f16"])
def test_mutants_of_the_fallback_kernel_exceed_the_bar(dtype):
    for mutant, epi in (("tanh", "gelu"), ("bias_after", "gelu"), ("alpha_bias", "full"), ("resid_m", "full"), ("tab_dst", "full"),
                        ("swap_k", "full")):
        if mutant == "swap_k" and dtype == F32:
            continue                               # (the fp32 cases have fewer than two whole 64-wide k-tiles)
        c = smallest(lambda c: c.dtype == dtype and c.epi == epi and gr.planned(c)["family"] == "fallback" and
                     (mutant != "swap_k" or c.K >= 128))
        bad, *_ = ratios(c, mutant)
        assert max(bad.values()) > 1.0, (mutant, cid(c), bad)


def signed_bias(c, mutant):
    _, st, b, e = ratios(c, mutant)
    return float((e["out"] - st["ref"]["out"]).mean() / b["out"].mean())


@pytest.mark.parametrize("c", [c for c in CASES if c.kind == "pos"], ids=cid)
def test_signed_bias_separates_rne_from_truncation(c):
    """Positive operands and bias: every output is a sum of positive terms.  Rounding to nearest is unbiased -- the mean signed
    error over n elements is sampling noise, ~0.4 bar / sqrt(n) -- while a truncating store pulls every element down by half an
    ulp on average, ~0.7 h |r| / 2 = 0.35 of the bar h |r|.  BIAS = 0.1 sits between."""
    assert c.M * c.N >= 4096
    assert abs(signed_bias(c, None)) < BIAS / 2, signed_bias(c, None)
    assert signed_bias(c, "trunc") < -2 * BIAS, signed_bias(c, "trunc")
    r, *_ = ratios(c, "trunc")
    assert r["out"] > 1.0                           # (truncation also exceeds the elementwise bar somewhere: up to a whole ulp)


# ----------------------------------------------------------------------------------------------------- the plan
def test_planned_mirrors_the_dispatch_rules():
    p = gr.planned
    assert p(Case(BF, 0, KC, KC, 1280, 768, 768, "plain"))["tile"] == 9064064            # <= 256 tiles of 64x64, even k-tiles
    assert p(Case(BF, 0, KC, KC, 1280, 768, 704, "plain"))["tile"] == 64064              # 11 k-tiles
    assert p(Case(BF, 0, KC, KC, 1280, 3072, 768, "plain"))["tile"] == 128064            # the tuned table
    assert p(Case(BF, 0, KC, KC, 8320, 3072, 1024, "gelu"))["tile"] == 256256
    assert p(Case(BF, 0, KC, KC, 8320, 1024, 1024, "plain"))["tile"] == 13144256
    tail = p(Case(BF, 0, KC, KC, 8320, 1024, 1536, "resid"))                             # 520 tiles of 128x128: one round of 512 + 8
    assert [x[0] for x in tail["parts"]] == [128128, 9064064] and tail["parts"][1][2:] == (8192, 128)
    assert p(Case(F32, 0, KC, KC, 70, 136, 96, "plain"))["family"] == "fallback"
    assert p(Case(BF, 0, KC, KC, 70, 136, 96, "plain"))["family"] == "fallback"          # K % 64
    assert p(Case(BF, 0, KC, KC, 70, 132, 128, "plain"))["family"] == "fallback"         # N % 8
    assert p(Case(BF, 0, KC, KC, 70, 136, 128, "gelu", odd=True))["family"] == "fallback"
    assert p(Case(BF, 9144064, RC, RC, 136, 72, 128, "plain"))["family"] == "refused"    # 144-row tiles: k-contiguous A only
    assert p(Case(BF, 9064064, KC, KC, 70, 72, 192, "plain"))["family"] == "refused"     # two k-groups: K % 128
    assert p(Case(BF, 256256, KC, KC, 264, 264, 64, "plain"))["family"] == "refused"     # K >= 128
    assert p(Case(BF, 256256, KC, KC, 264, 264, 128, "full"))["family"] == "refused"     # no row maps on the 256 x 256 tile
    assert p(Case(BF, 256256, RC, KC, 264, 264, 128, "plain"))["family"] == "refused"
    sk = p(Case(BF, 0, RC, RC, 136, 72, 1280, "colsum", 5, True))                        # test_gemm_split_k_wgrad
    assert (sk["family"], sk["tile"], sk["split"]) == ("splitk", 64064, 5)
    assert p(Case(BF, 0, RC, RC, 136, 72, 1280, "colsum", 0, True))["split"] == 2        # 20 k-tiles / 10 steps


def test_cases_reach_every_tile_class_epilogue_and_split():
    plans = {c: gr.planned(c) for c in CASES}
    assert all(p["family"] != "refused" for p in plans.values())
    for dt in (BF, F16):
        mine = {c: p for c, p in plans.items() if c.dtype == dt and c.kind == "randn"}
        for tile, (bm, bn, stride, wk) in gr.TILES.items():
            classes = {(KC, KC), (KC, RC)} if bm == 144 else ({(KC, KC), (KC, RC), (RC, RC)} if tile == gr.T256 else
                                                              {(KC, KC), (KC, RC), (RC, RC), (RC, KC)})
            for al, bl in classes:
                got = {c.epi for c, p in mine.items() if p["parts"][0][0] == tile and (c.al, c.bl) == (al, bl) and p["split"] == 1}
                if tile == gr.T256 and al == RC:
                    need = {"plain", "colsum"}
                else:
                    need = {"plain", "resid" if tile == gr.T256 else "full", "gelu", "dgelu"} | ({"colsum"} if al == RC else set())
                assert need <= got, (gr.DT[dt], tile, al, bl, sorted(need - got))
            # ragged rows and columns, a short k-loop and one that wraps the ring more than once
            ks = {c.K for c, p in mine.items() if p["parts"][0][0] == tile and p["split"] == 1}
            assert min(ks) == (128 if wk == 2 or tile == gr.T256 else 64) and max(ks) >= 320
            if tile != gr.T256:
                assert any(c.M % stride and c.N % bn for c, p in mine.items() if p["parts"][0][0] == tile)
            if bm == 144:
                ms = {c.M for c, p in mine.items() if p["parts"][0][0] == tile}
                assert any(m % stride == 0 for m in ms) and any(m % stride for m in ms)
        # split-K: forced 2 and 5 on both tiles, the automatic factor, every epilogue in KC.KC and KC.RC, RC.RC with column sums
        for tile in (64064, 128128):
            for s in (2, 5):
                for al, bl in ((KC, KC), (KC, RC)):
                    got = {c.epi for c, p in mine.items() if p["family"] == "splitk" and p["tile"] == tile and p["split"] == s and
                           c.split == s and (c.al, c.bl) == (al, bl)}
                    assert {"plain", "full", "gelu", "dgelu"} <= got, (tile, s, al, bl, got)
                assert any(p["family"] == "splitk" and p["tile"] == tile and p["split"] == s and c.epi == "colsum" and c.al == RC
                           for c, p in mine.items())
        auto = [c for c, p in mine.items() if c.ws and c.split == 0 and c.K == 1536 and p["split"] > 1]
        assert {"plain", "full", "gelu", "dgelu", "colsum"} <= {c.epi for c in auto}
        assert all((c.N // 8) % 2 == 1 for c, p in mine.items() if p["family"] == "splitk")        # N = 8 x odd
        # the fallback kernel: both tiles, every class and epilogue, K = 72, N = 8 k + 4, a misaligned ldo
        fb = [c for c, p in mine.items() if p["family"] == "fallback"]
        for tile in (64, 128):
            for al, bl in ((KC, KC), (KC, RC), (RC, RC), (RC, KC)):
                got = {c.epi for c in fb if plans[c]["tile"] == tile and (c.al, c.bl) == (al, bl)}
                assert {"plain", "full", "gelu", "dgelu"} | ({"colsum"} if al == RC else set()) <= got
        assert any(c.K == 72 for c in fb) and any(c.N % 8 == 4 for c in fb) and any(c.odd for c in fb)
        # signed bias: one case per family
        assert {plans[c]["family"] for c in CASES if c.kind == "pos" and c.dtype == dt} == {"fallback", "pipe", "tile256", "splitk"}
    f32 = [c for c in CASES if c.dtype == F32]
    for tile in (64, 128):
        for al, bl in ((KC, KC), (KC, RC), (RC, RC), (RC, KC)):
            got = {c.epi for c in f32 if plans[c]["tile"] == tile and (c.al, c.bl) == (al, bl)}
            assert {"plain", "full", "gelu", "dgelu"} | ({"colsum"} if al == RC else set()) <= got
    assert all(plans[c]["family"] == "fallback" for c in f32)
    # sizes: nothing but the row tail exceeds about 600 rows
    assert all(c.M <= 600 and c.N <= 600 and c.K <= 1536 for c in SMALL) and len(LARGE) == 1


def test_gelu_cases_reach_both_tails():
    """Pre-activations (GELU) and dGELU operands in [-8, -3] and [3, 8], where 16-bit relative precision and the absolute cdf error
    part ways: the contrast scaling spreads v over many octaves, aux is drawn with sigma 3."""
    for c in SMALL:
        if c.epi not in ("gelu", "dgelu"):
            continue
        t = gr.inputs(c)
        x = gr.reference(c, t)["v"] if c.epi == "gelu" else t["aux"].double()
        assert int(((x > -8) & (x < -3)).sum()) >= 8 and int(((x > 3) & (x < 8)).sum()) >= 8, cid(c)
        if c.epi == "gelu":
            assert int(((x > -6) & (x < -4)).sum()) >= 1, cid(c)


def test_row_tail_case_has_the_fewest_rows():
    """plan_single cuts a row tail off a launch of 128x128 / 256x128 / 256x256 tiles only past one whole round of them (512 / 256
    tiles: >= 8.3 M outputs) with at most 64 tail tiles, i.e. at least 9 / 5 row blocks: 1025 rows is the fewest, at 64 tile
    columns."""
    (tail,) = LARGE
    p = gr.planned(tail)
    assert [x[0] for x in p["parts"]] == [128128, 9064064] and p["parts"][1][2:] == (1024, 1) and p["counts"]["pipe"] == 2
    fewest = None
    for tile in (128128, 2256128, 256256):
        bm, bn = gr.TILES[tile][:2]
        for R in range(1, 12):
            for C in range(1, 80):
                c = Case(BF, tile, KC, KC, (R - 1) * bm + 8, (C - 1) * bn + 8, 128, "gelu")
                if len(gr.planned(c)["parts"]) == 2:
                    fewest = c.M if fewest is None else min(fewest, c.M)
    assert fewest == 1032 and tail.M == 1025            # (the search steps in whole row blocks + 8: the 9th block is the first)
