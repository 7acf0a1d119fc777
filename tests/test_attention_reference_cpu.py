"""CPU checks of tests/attention_reference.py: the fp64 statement against autograd and the oracle, the bar against the emulated
kernel arithmetic (round to nearest even meets it, truncation fails the signed-bias check), the dispatch rules against the
library's own planner (skyemb_mha_plan: no device needed) and against the launches traced before the planner existed, and the GPU
case list of tests/test_attention_core_gpu.py against the dispatch rules.

Worst err/bar of the emulation: 16-bit within [0.2, 1] (output rounding and the one rounding of P / dS are the bar's own
terms).  fp32 sits near 0.01: the bar's fp32 terms are worst-case gamma_n bounds (module docstring of attention_reference.py,
item 2) while real sums err like sqrt(n) u, and at hd 64 the score term alone carries hd s sum|q||k| u ~ 300 u against the
few u a score actually errs by.  A tighter fp32 bar would rest on measured figures; the fp32 test only pins that the
emulation stays under it and that the bar is not absurdly loose (> 1e-3).
"""
import pytest
import torch

from tests import attention_reference as ar

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def rand(B, N, H, hd, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    qkv, dout = torch.randn(B, N, 3 * H * hd, generator=g), torch.randn(B, N, H * hd, generator=g)
    return qkv.to(dtype), dout.to(dtype)


def test_core_matches_sdpa_autograd():
    B, N, H, hd = 3, 11, 2, 16
    qkv, dout = rand(B, N, H, hd, 1)
    c = ar.core(qkv, dout, H, hd)
    x = qkv.clone().requires_grad_(True)
    t = x.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    o = torch.nn.functional.scaled_dot_product_attention(t[0], t[1], t[2])
    o = o.transpose(1, 2).reshape(B, N, H * hd)
    o.backward(dout)
    g = x.grad.reshape(B, N, 3, H * hd)
    torch.testing.assert_close(c["ref"]["out"], o.detach(), rtol=1e-12, atol=1e-12)
    for i, n in enumerate(("dq", "dk", "dv")):
        torch.testing.assert_close(c["ref"][n], g[:, :, i], rtol=1e-12, atol=1e-12)


def test_core_matches_the_oracle_attention_block(monkeypatch):
    """oracle/mae_oracle.py block() with its LayerNorm / MLP switched off and its qkv projection returning the given qkv: the
    block's output is then x + O and its gradient the attention core's, on the oracle's own [B, N, 3, H, hd] layout."""
    from oracle import mae_oracle as mo
    B, N, H, hd = 2, 9, 3, 8
    D = H * hd
    qkv, dout = rand(B, N, H, hd, 2)
    x_qkv = qkv.clone().requires_grad_(True)
    W = {n: torch.zeros(1, dtype=torch.float64) for n in ("qkv", "proj", "fc1", "fc2")}

    def fake_linear(h, w, b=None):
        if w is W["qkv"]:
            return x_qkv
        if w is W["proj"]:
            return h
        return torch.zeros(*h.shape[:-1], 4 * D if w is W["fc1"] else D, dtype=h.dtype)

    monkeypatch.setattr(mo, "linear", fake_linear)
    st = {"p.norm1.weight": torch.ones(D, dtype=torch.float64), "p.norm1.bias": torch.zeros(D, dtype=torch.float64),
          "p.norm2.weight": torch.ones(D, dtype=torch.float64), "p.norm2.bias": torch.zeros(D, dtype=torch.float64),
          "p.attn.qkv.weight": W["qkv"], "p.attn.qkv.bias": None, "p.attn.proj.weight": W["proj"], "p.attn.proj.bias": None,
          "p.mlp.fc1.weight": W["fc1"], "p.mlp.fc1.bias": None, "p.mlp.fc2.weight": W["fc2"], "p.mlp.fc2.bias": None}
    x = torch.zeros(B, N, D, dtype=torch.float64)
    o = mo.block(x, st, "p", H, 1e-6)
    o.backward(dout)
    c = ar.core(qkv, dout, H, hd)
    g = x_qkv.grad.reshape(B, N, 3, D)
    torch.testing.assert_close(c["ref"]["out"], o.detach(), rtol=1e-12, atol=1e-12)
    for i, n in enumerate(("dq", "dk", "dv")):
        torch.testing.assert_close(c["ref"][n], g[:, :, i], rtol=1e-12, atol=1e-12)


def special(kind, B, N, H, hd, seed):
    qkv, dout = rand(B, N, H, hd, seed, torch.float32)
    x = qkv.reshape(B, N, 3, H, hd)
    if kind == "logits60":                   # q . k s = +-60 against one key, as tests/test_attention_long_gpu.py spiked()
        u = torch.randn(hd, generator=torch.Generator().manual_seed(seed))
        u = u / u.norm()
        x[:, N - 1, 1] = 8.0 * u
        x[:, :, 0] += 7.5 * hd ** 0.5 * torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)[None, :, None, None] * u
    elif kind == "onehot":                   # every query row attends to one key (logit gap ~ 100)
        x[:, :, 0] = 0.0
        x[:, :, 1] = 0.0
        for i in range(N):
            x[:, i, 0, :, i % hd] = 10.0 * hd ** 0.25
            x[:, i, 1, :, i % hd] = 10.0 * hd ** 0.25
    elif kind == "zeroq":                    # query 1 is zero: uniform attention
        x[:, 1, 0] = 0.0
    elif kind == "dout_up":
        dout = dout * 2.0 ** 10
    elif kind == "dout_down":
        dout = dout * 2.0 ** -10
    elif kind == "posv":
        x[:, :, 2] = x[:, :, 2].abs() + 0.25
        dout = dout.abs() + 0.25
    return x.reshape(B, N, -1), dout


KINDS = ["randn", "logits60", "onehot", "zeroq", "dout_up", "dout_down"]
SHAPES = [(7, 5, 3, 64), (3, 17, 2, 32), (2, 65, 2, 64), (1, 257, 2, 32)]


def emulated_ratio(kind, shape, dtype, rounding="rne"):
    B, N, H, hd = shape
    qkv, dout = special(kind, B, N, H, hd, N + hd)
    qkv, dout = qkv.to(dtype).float(), dout.to(dtype).float()
    c = ar.core(qkv, dout, H, hd)
    b = ar.bars(c, dtype)
    e = ar.emulate(qkv, dout, H, hd, dtype, rounding)
    return {n: ar.worst((e[n] - c["ref"][n]).abs(), b[n]) for n in ar.NAMES}, c, b, e


@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("kind", KINDS)
def test_rne_emulation_meets_the_16bit_bar_closely(kind, dtype):
    worst = 0.0
    for shape in SHAPES:
        r, *_ = emulated_ratio(kind, shape, dtype)
        assert max(r.values()) <= 1.0, (shape, r)
        worst = max(worst, max(r.values()))
    assert worst >= 0.2, worst


def test_fp32_emulation_meets_the_fp32_bar():
    worst = 0.0
    for kind in KINDS:
        for shape in SHAPES:
            r, *_ = emulated_ratio(kind, shape, F32)
            assert max(r.values()) <= 1.0, (kind, shape, r)
            worst = max(worst, max(r.values()))
    assert worst > 1e-3, worst


def signed_bias(e, c, b, n):
    return float((e[n] - c["ref"][n]).mean() / b[n].mean())


@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_N%d_H%d_hd%d" % s)
def test_signed_bias_separates_rne_from_truncation(shape, dtype):
    """The check of tests/test_attention_core_gpu.py (BIAS there): positive V and dO, mean signed error over mean bar."""
    from tests.test_attention_core_gpu import BIAS
    _, c, b, e = emulated_ratio("posv", shape, dtype, "rne")
    for n in ("out", "dv"):
        assert abs(signed_bias(e, c, b, n)) < BIAS / 2, (n, signed_bias(e, c, b, n))
    _, c, b, e = emulated_ratio("posv", shape, dtype, "trunc")
    for n in ("out", "dv"):
        assert signed_bias(e, c, b, n) < -2 * BIAS, (n, signed_bias(e, c, b, n))


def test_round_to_truncates_toward_zero():
    x = torch.tensor([1.0 + 2 ** -8 + 2 ** -10, -(1.0 + 2 ** -8 + 2 ** -10), 3.0, 1.0 + 2 ** -12])
    assert ar.round_to(x, BF, "trunc").tolist() == [1.0, -1.0, 3.0, 1.0]
    assert ar.round_to(x, BF, "rne").tolist() == [1.0 + 2 ** -7, -(1.0 + 2 ** -7), 3.0, 1.0]
    y = torch.tensor([1.0 + 2 ** -11 + 2 ** -12, -(1.0 + 2 ** -11 + 2 ** -12), 2.0 ** -24 * 2.75])
    assert ar.round_to(y, F16, "trunc").tolist() == [1.0, -1.0, 2.0 ** -24 * 2]      # the last one subnormal
    assert ar.round_to(y, F16, "rne").tolist() == [1.0 + 2 ** -10, -(1.0 + 2 ** -10), 2.0 ** -24 * 3]


# ----------------------------------------------------------------------------------------------------- dispatch coverage
@pytest.mark.parametrize("hd,fwd,bwd", [(64, (19, 24, 35, 125), (14, 18, 26, 91)), (32, (30, 38, 52, 156), (22, 28, 38, 112))])
def test_fp32_plan_switch_points(hd, fwd, bwd):
    """attention.hip make_plan and the 160 KB switch: first N with 3, 2, 1 waves, first N that streams."""
    for bw, pts in ((False, fwd), (True, bwd)):
        sp = ar.switch_points(hd, bw)
        assert (sp["lds_w3"], sp["lds_w2"], sp["lds_w1"], sp["stream"]) == pts
    assert ar.family(1, 100, 1, 64, F32, False) == "lds_w1" and ar.family(1, 100, 1, 64, F32, True) == "stream"


def test_mfma_dispatch_rules():
    f = ar.family
    assert f(256, 5, 12, 64, BF, False) == "mfma_packed_wpb1"            # 516 tiles
    assert f(256, 17, 16, 32, BF, True) == "mfma_single_wpb4"            # 4096 tiles
    assert f(409, 17, 5, 32, F16, False) == "mfma_single_wpb4"           # 2045 tiles: the first four-wave launch
    assert f(1, 17, 2044, 32, F16, False) == "mfma_single_wpb1"
    assert f(4093, 5, 3, 32, BF, False) == "mfma_packed_wpb4"            # 683 packs x 3 heads = 2049
    assert f(3, 65, 3, 64, BF, True) == "mfma_strip3" and f(3, 129, 3, 32, F16, True) == "mfma_long"
    assert f(3, 65, 3, 80, BF, False) == "lds_w1" and f(3, 65, 3, 64, BF, False, mfma=False) == "lds_w1"
    assert f(3, 5, 3, 64, F32, False) == "lds_w4"


def test_gpu_cases_cover_every_family():
    from tests.test_attention_core_gpu import CASES, NOMFMA_CASES
    lds = {"lds_w1", "lds_w2", "lds_w3", "lds_w4", "stream"}
    mfma = {"mfma_packed_wpb1", "mfma_packed_wpb4", "mfma_single_wpb1", "mfma_single_wpb4", "mfma_strip2", "mfma_strip3",
            "mfma_strip4", "mfma_long"}
    need = {F32: lds, BF: lds | mfma, F16: lds | mfma}
    for bwd in (False, True):
        for dt, fams in need.items():
            got = {ar.family(c.B, c.N, c.H, c.hd, c.dtype, bwd, c.mfma) for c in CASES if c.dtype == dt}
            assert fams <= got, (DTYPE_NAME[dt], "bwd" if bwd else "fwd", sorted(fams - got))
        # idle waves in the last four-wave workgroup: nheads % 4 != 0 at 2045 / 2049 / 2051 tiles, packed and single-tile
        for P in ("packed", "single"):
            tiles = set()
            for c in CASES:
                if ar.family(c.B, c.N, c.H, c.hd, c.dtype, bwd) == f"mfma_{P}_wpb4":
                    p = 32 // c.N if c.N <= 16 else 1
                    tiles.add((c.B + p - 1) // p * c.H)
            assert {2045, 2049, 2051} <= tiles, (P, sorted(tiles))
        # every LDS waves-per-block value with a last block whose waves are partly idle (B H not a multiple of it)
        for dt in need:
            part = set()
            for c in CASES:
                f = ar.family(c.B, c.N, c.H, c.hd, c.dtype, bwd, c.mfma)
                if c.dtype == dt and f.startswith("lds_w") and c.B * c.H % int(f[-1]) != 0:
                    part.add(f)
            assert {"lds_w2", "lds_w3", "lds_w4"} <= part, (DTYPE_NAME[dt], "bwd" if bwd else "fwd", sorted(part))
    for dt in (BF, F16):
        got = {(c.N, ar.family(c.B, c.N, c.H, c.hd, dt, True, False)) for c in NOMFMA_CASES if c.dtype == dt and c.hd in (32, 64)}
        assert {n for n, _ in got} & {5, 17} and {n for n, _ in got} & {65, 97} and max(n for n, _ in got) > 128
        assert "stream" in {f for _, f in got}
    # last packs of 16 and 17 rows, strips at N = 33 ... 128 at both head dims, the signed-bias cases
    rows = {((c.B - 1) % (32 // c.N) + 1) * c.N for c in CASES if c.N <= 16 and c.dtype == BF}
    assert {16, 17} <= rows
    assert {(n, hd) for n in (33, 63, 64, 65, 96, 97, 127, 128) for hd in (32, 64)} <= {(c.N, c.hd) for c in CASES}
    pos = {ar.family(c.B, c.N, c.H, c.hd, c.dtype, False) for c in CASES if c.kind == "pos"}
    assert mfma <= pos


DTYPE_NAME = {BF: "bf16", F16: "f16", F32: "f32"}


# ----------------------------------------------------------------------------------------------------- the library's planner
def plan_name(p):
    """A skyemb_mha_plan answer in the words of ar.family."""
    from sky_embeddings_amd import _lib
    if p.family == _lib.MHA_LDS:
        return f"lds_w{p.waves}"
    if p.family == _lib.MHA_MFMA_STRIP:
        return f"mfma_strip{p.waves}"
    if p.family in (_lib.MHA_MFMA_PACKED, _lib.MHA_MFMA_SINGLE):
        return f"mfma_{'packed' if p.family == _lib.MHA_MFMA_PACKED else 'single'}_wpb{p.waves}"
    return {_lib.MHA_STREAM: "stream", _lib.MHA_MFMA_LONG: "mfma_long"}[p.family]


def test_dispatch_rules_agree_with_the_library_planner():
    """ar.family / ar.lds_plan against skyemb_mha_plan at every point of: three dtypes x fwd / bwd x MFMA on / off, hd in
    {8, 16, 32, 40, 64, 80, 128}, every N in 1..400 and 4097, 4098, and (B, H) that put nheads at 1 and at 2043..2052 (H = 1, and
    H = 3 for the multiples of 3) for packed and single tiles -- both sides of (nheads + 3) / 4 < 512.  Integer work only."""
    import ctypes
    from sky_embeddings_amd import _lib, ops
    L, p = _lib.lib(), _lib.MhaPlan()
    ref, points = ctypes.byref(p), 0
    for N in list(range(1, 401)) + [4097, 4098]:
        P = 32 // N if N <= 16 else 1
        shapes = [(1, 1)] + [((t - 1) * P + 1, 1) for t in range(2043, 2053)] + [((t - 1) * P + 1, 3) for t in range(681, 685)]
        for hd in (8, 16, 32, 40, 64, 80, 128):
            for dt in (BF, F16, F32):
                code = ops.dtype_code(dt)
                for bwd in (False, True):
                    w, smem = ar.lds_plan(N, hd, bwd)
                    for mfma in (True, False):
                        sw = 0 if mfma else _lib.MHA_SW_NO_MFMA
                        for B, H in shapes:
                            assert L.skyemb_mha_plan(int(bwd), code, B, N, H, hd, sw, ref) == 0, L.skyemb_last_error()
                            fam = ar.family(B, N, H, hd, dt, bwd, mfma)
                            at = (DTYPE_NAME[dt], bwd, mfma, B, N, H, hd)
                            assert plan_name(p) == fam, at
                            assert p.block == 64 * p.waves, at
                            if fam.startswith("lds_w"):
                                assert (p.waves, p.lds_bytes, p.grid_x) == (w, smem, -(-B * H // w)), at
                                assert p.per_wave_floats * 4 * w == smem and p.lds_limit == (ar.LDS_LIMIT if smem > 65536 else 0), at
                            elif fam.startswith("mfma_packed") or fam.startswith("mfma_single"):
                                nheads = -(-B // P) * H
                                assert (p.hd, p.nheads, p.grid_x, p.lds_bytes) == (hd, nheads, -(-nheads // p.waves), 0), at
                            elif fam != "stream":
                                assert (p.hd, p.grid_x) == (hd, B * H), at
                            points += 1
    assert points == 402 * 15 * 7 * 3 * 2 * 2


def test_planner_refuses_what_the_entry_points_refuse():
    import ctypes
    from sky_embeddings_amd import _lib
    L, p = _lib.lib(), _lib.MhaPlan()
    for bwd, who in ((0, b"skyemb_mha_fwd: "), (1, b"skyemb_mha_bwd: ")):
        for dt in (0, 1, 2):
            assert L.skyemb_mha_plan(bwd, dt, 1, 4099, 1, 64, 0, ctypes.byref(p)) == 1
            assert L.skyemb_last_error() == who + b"N = 4099 tokens, more than the supported 4098"
            for hd in (4, 12, 36, 0, -8):
                assert L.skyemb_mha_plan(bwd, dt, 2, 17, 3, hd, 0, ctypes.byref(p)) == 1
                assert L.skyemb_last_error() == who + b"bad shape (head dim must be a multiple of 8)"
            # a head wider than the streaming kernels take is refused exactly where the whole-head LDS plan passes 160 KB
            hd = ar.STREAM_MAX_HD + 8
            for N in range(1, 40):
                rc = L.skyemb_mha_plan(bwd, dt, 2, N, 3, hd, 0, ctypes.byref(p))
                w, smem = ar.lds_plan(N, hd, bool(bwd))
                if smem > ar.LDS_LIMIT:
                    assert rc == 1 and L.skyemb_last_error() == who + b"head dim %d with N = %d tokens: at most 512" % (hd, N)
                else:
                    assert rc == 0 and plan_name(p) == f"lds_w{w}"
            assert L.skyemb_mha_plan(bwd, dt, 2, 4098, 3, ar.STREAM_MAX_HD, 0, ctypes.byref(p)) == 0 and plan_name(p) == "stream"
    # the entry points refuse in the same words before any device work
    assert L.skyemb_mha_fwd(None, None, 1, 2, 39, 3, 520, None) == 1
    assert L.skyemb_last_error() == b"skyemb_mha_fwd: head dim 520 with N = 39 tokens: at most 512"
    assert L.skyemb_mha_bwd(None, None, None, 0, 2, 17, 3, 36, None) == 1
    assert L.skyemb_last_error() == b"skyemb_mha_bwd: bad shape (head dim must be a multiple of 8)"


def test_planner_switches():
    """Explicit switch bits: MFMA off, tiles per workgroup forced either way; -1 reads the environment (unset here: the defaults)."""
    import os
    from sky_embeddings_amd import _lib, ops
    assert "SKYEMB_MHA_MFMA" not in os.environ and "SKYEMB_MHA_WPB" not in os.environ
    for B, N, H, hd in ((256, 5, 12, 64), (256, 17, 16, 32), (3, 65, 3, 64), (3, 129, 3, 32), (3, 40, 3, 80)):
        for bwd in (False, True):
            auto, env = ops.mha_plan(bwd, BF, B, N, H, hd, 0), ops.mha_plan(bwd, BF, B, N, H, hd)
            assert all(getattr(auto, f) == getattr(env, f) for f, _ in _lib.MhaPlan._fields_)
            for sw, wpb in ((_lib.MHA_SW_WPB1, 1), (_lib.MHA_SW_WPB4, 4)):
                p = ops.mha_plan(bwd, BF, B, N, H, hd, sw)
                if N <= 32 and hd in (32, 64):
                    assert (p.waves, p.block, p.grid_x) == (wpb, 64 * wpb, -(-p.nheads // wpb)) and p.nheads == auto.nheads
                else:
                    assert all(getattr(auto, f) == getattr(p, f) for f, _ in _lib.MhaPlan._fields_)
            off = ops.mha_plan(bwd, BF, B, N, H, hd, _lib.MHA_SW_NO_MFMA)
            assert plan_name(off) == ar.family(B, N, H, hd, BF, bwd, False)


def test_planner_reproduces_the_launches_traced_before_it():
    """tests/golden/mha_launches.json: kernel, grid in threads and workgroup size of every launch of CASES and NOMFMA_CASES, from a
    kernel trace of the commit before the planner (tests/golden/make_mha_launch_golden.py)."""
    import json
    import os
    from sky_embeddings_amd import _lib, ops
    from tests.test_attention_core_gpu import CASES, NOMFMA_CASES, cid
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mha_launches.json")) as f:
        golden = json.load(f)
    cases = {cid(c): c for c in CASES + NOMFMA_CASES}
    assert sorted(golden) == sorted(cases) and len(cases) == len(CASES) + len(NOMFMA_CASES)
    for name, c in cases.items():
        for bwd in (False, True):
            p = ops.mha_plan(bwd, c.dtype, c.B, c.N, c.H, c.hd, 0 if c.mfma else _lib.MHA_SW_NO_MFMA)
            d = "bwd" if bwd else "fwd"
            kernel = {_lib.MHA_LDS: f"mha_{d}_kernel", _lib.MHA_STREAM: f"mha_{d}_stream_kernel",
                      _lib.MHA_MFMA_PACKED: f"mha_{d}_mfma_kernel<{p.hd}, {p.waves}>",
                      _lib.MHA_MFMA_SINGLE: f"mha_{d}_mfma_kernel<{p.hd}, {p.waves}>",
                      _lib.MHA_MFMA_STRIP: f"mha_{d}_strip_kernel<{p.hd}, {p.waves}>",
                      _lib.MHA_MFMA_LONG: f"mha_{d}_long_kernel<{p.hd}>"}[p.family]
            got = {"kernel": kernel, "operand": DTYPE_NAME[c.dtype], "grid": [p.grid_x * p.block, p.grid_y], "workgroup": p.block}
            assert got == golden[name][d], (name, d)
