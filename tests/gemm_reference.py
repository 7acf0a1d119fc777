"""Float64 statement of one skyemb_gemm call (include/skyemb.h), its elementwise error bar, a CPU emulation of the kernels'
arithmetic, the launch plan `plan_single` should choose, and the case table of tests/test_gemm_elementwise_gpu.py.  Pinned on the
CPU by tests/test_gemm_reference_cpu.py.

Statement (`reference`), computed in fp64 from the operands exactly as the kernel reads them (16-bit values widened):
    acc = A B^T                                   A [M, K], B [N, K] (logical; either may be stored row-contiguous)
    v   = alpha acc + bias[n] + table[tab_row[m], n] + resid[dst(m), n]        dst(m) = dst_row ? dst_row[m] : m
    out2 = v (GELU only);   y = gelu(v) | v gelu'(aux[m, n]) | v;   y -> out_f32 and / or out, at row dst(m) (dst(m) < 0: not written)
    colsum_a[m] = sum_k A[m, k]
alpha multiplies the accumulator only: every kernel scales the tile (`acc * g.alpha`, split-K: each slab) BEFORE bias, table and
residual are added (gemm.hip `acc[i][j][r] * g.alpha`, gemm_pipe.hip / gemm_pipe256.h `v * g.alpha` while staging the tile).

The bar (`bars`).  u = 2^-24 is fp32's unit roundoff; h the stored format's: 2^-8 bf16, 2^-11 fp16, u fp32.

1. Accumulation.  Products of two 16-bit values are exact in fp32 (fp32 operands: rounded once, inside the same bound).  Summing K
   terms in fp32 in ANY order -- MFMA trees, 64-wide k-tiles, two k-groups added in LDS, split-K slabs added by the reduce kernel --
   is K - 1 additions, each at most u of a partial sum that |A| |B|^T bounds: the gamma_K bound (K - 1) u |A| |B|^T.  The alpha
   multiply is one more rounding of (a slab of) the sum.  Together
       E_acc = K u |alpha| (|A| |B|^T).
2. Epilogue adds.  Each of the n_add <= 3 additions (bias, table row, residual) rounds a partial sum that
   T = |alpha acc| + |bias| + |table| + |resid| bounds:  E_v = E_acc + n_add u T  is the bound on |v32 - v|.
3. GELU / dGELU.  y32 = fl(v32 cdf32(v32)) against y = v Phi(v):
       |y32 - y| <= |v| |cdf32 - Phi| + sup|gelu'| E_v + u |y|  <=  E_CDF |v| + 1.13 E_v + 2 u |y|
   (mean value theorem on v Phi(v), whose derivative IS gelu', |gelu'| <= 1.129; the second u: the 0.5 x (1 + erf) chain of the
   fallback).  dGELU: y32 = fl(v32 dg32(aux)), aux a stored value and therefore exact:  E_CDF |v| + 1.13 E_v + 2 u |y|  with E_CDF
   bounding |dg32 - gelu'| as well.  E_CDF is an ABSOLUTE error of the cdf:
   - 16-bit pipe kernels (gemm_pipe.hip `gelu_parts`: Abramowitz-Stegun 7.1.26, hardware exp and rcp): E_CDF = 2^-20 = 9.5e-7,
     3x the 3.1e-7 (cdf) / 2.8e-7 (dGELU) an fp32 emulation reaches on a dense grid over [-9, 9]
     (test_e_cdf_bounds_the_emulated_gelu_parts); the margin is for the 1-ulp hardware exp and rcp.
   - gemm.hip (fp32, and 16-bit problems outside the pipe subset): erff / expf.  0.5 (1 + erf(x / sqrt 2)): erff to ~1 ulp of a value
     <= 1 (2 u), the argument's rounding through erf' (<= 0.5 u), 1 + erf rounded (<= 2 u before the halving): <= 3.5 u on the cdf;
     dGELU adds x pdf (|x pdf| <= 0.25 to a few ulp: 1 u) and one more add (1.2 u).  E_CDF = 8 u = 2^-21, pinned the same way.
   Being absolute, the term states the contract for x < -4: gelu(x) is accurate to E_CDF |x|, not to h of itself (there
   Phi(x) < 3.2e-5: E_CDF is 3 % of gelu(x) at x = -4 and more than all of it below x = -4.8; it passes fp16's h below x = -2.9).
4. Stored rounding, once, to nearest:  |y - r| <= h |y32| + |y32 - r| <= h |r| + (1 + h) |y32 - r|, so
       bar = h |r| + (1 + h) rest + floor,      floor = 2^-25 (fp16: the absolute rounding error of a subnormal) + 2^-126 (a flush).
   rest = E_v (no activation, and out2: v rounded ONCE -- GELU is applied to the unrounded v32, so a kernel that applies it to the
   rounded out2 errs by ~h |v| |gelu'|, far above rest) or item 3's.  colsum_a: K u sum_k |A[m, k]| + 2^-126.

The fp32 terms are worst-case bounds (every rounding in one direction), so the emulation's fp32 outputs reach 0.0005-0.47 of the
bar (highest at K = 20, where gamma_K is nearest to what a sum really errs by) and column sums 0.0001-0.07; 16-bit outputs are
dominated by h |r| and the emulation's worst err/bar per case lies in 0.83-1.00 (bf16) and 0.26-0.99 (fp16; low where every
output of a case is subnormal-sized or large against its ulp), inside the [0.05, 1] tests/test_gemm_reference_cpu.py pins per case.  What the kernels achieve on the
GPU is recorded by tests/test_gemm_elementwise_gpu.py (record_parity "gemm_elementwise"), not assumed here.
"""
import math
from collections import namedtuple

import torch

from tests.attention_reference import F16_SUB, TINY, U32, UNIT, round_to, worst  # noqa: F401  (re-exported)

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {F32: "f32", BF: "bf16", F16: "f16"}
KC, RC = 0, 1
E_CDF_PIPE = 2.0 ** -20
E_CDF_ERFF = 2.0 ** -21
GELU_SLOPE = 1.13             # sup |gelu'| = 1.1289 (at x = sqrt 2)

# tile codes (gemm_pipe.hip SKY_GEMM_PRODUCT_TILES): code -> (BM, BN, row stride, two k-groups)
TILES = {64064: (64, 64, 64, 1), 128064: (128, 64, 128, 1), 128128: (128, 128, 128, 1), 2256128: (256, 128, 256, 1),
         6128064: (128, 64, 128, 1), 6064064: (64, 64, 64, 1), 9064064: (64, 64, 64, 2), 9128128: (128, 128, 128, 2),
         9144064: (144, 64, 136, 2), 13144256: (144, 256, 130, 1), 256256: (256, 256, 256, 1)}
T256 = 256256
LEGACY = {64: 64064, 128: 128128, 12864: 128064}
# gemm_tuned.h: (M, N, K, a_kc, b_kc, tile, split)
TUNED = ((1280, 3072, 768, 1, 1, 12864, 1), (1280, 3072, 768, 1, 0, 6128064, 1), (4352, 2048, 512, 1, 1, 6128064, 1),
         (4352, 2048, 512, 1, 0, 6128064, 1), (4352, 1536, 512, 1, 1, 128, 1), (4352, 1280, 512, 1, 1, 128, 1),
         (1280, 2304, 768, 1, 1, 6064064, 1), (4352, 512, 2048, 1, 1, 9144064, 1), (4352, 512, 1536, 1, 0, 9144064, 1),
         (4352, 512, 2048, 1, 0, 9144064, 1), (4352, 512, 512, 1, 0, 6064064, 1), (8320, 3072, 1024, 1, 1, 256256, 1),
         (8320, 1024, 1024, 1, 1, 13144256, 1), (8320, 1024, 1024, 1, 0, 13144256, 1), (8320, 1024, 4096, 1, 1, 13144256, 1))

# epi: plain (out_f32) | full (alpha, bias, table / tab_row, dst_row with a -1, resid -> out_f32 + out) | resid (alpha, bias, resid ->
# out_f32 + out: `full` without row maps, for the 256 x 256 tile) | gelu (bias, GELU -> out + out2) | dgelu (aux -> out) |
# colsum (out_f32 + colsum_a, row-contiguous A) | bias (bias -> out: the signed-bias cases).
# split: skyemb_gemm_args.split_k; ws: a split-K workspace is passed; kind: randn | pos; odd: ldo = N + 4 (misaligned for the pipe).
Case = namedtuple("Case", "dtype tile al bl M N K epi split ws kind odd", defaults=(0, False, "randn", False))
EXTRA_ROWS = 5                # output rows beyond M under a dst_row scatter
TABLE_ROWS = 9
CONTRAST = {BF: ((-6, -3, 0, 3, 6), (4, -4, 0, 2, -2)), F32: ((-6, -3, 0, 3, 6), (4, -4, 0, 2, -2)),
            F16: ((-2, -1, 0, 1, 2), (2, -2, 0, 1, -1))}


def cid(c):
    s = f"{DT[c.dtype]}-t{c.tile}-{'KR'[c.al]}C{'KR'[c.bl]}C-{c.M}x{c.N}x{c.K}-{c.epi}"
    if c.ws:
        s += f"-split{c.split}"
    return s + ("" if c.kind == "randn" else "-" + c.kind) + ("-oddld" if c.odd else "")


def has(c, what):
    return {"alpha": c.epi in ("full", "resid"), "bias": c.epi in ("full", "resid", "gelu", "bias"), "table": c.epi == "full",
            "dst": c.epi == "full", "resid": c.epi in ("full", "resid"), "aux": c.epi == "dgelu", "colsum": c.epi == "colsum",
            "out_f32": c.epi in ("plain", "full", "resid", "colsum"), "out": c.epi in ("full", "resid", "gelu", "dgelu", "bias"),
            "out2": c.epi == "gelu"}[what]


def out_rows(c):
    return c.M + EXTRA_ROWS if has(c, "dst") else c.M


def lds(c):
    """Leading dimensions of the guarded buffers: every one beyond its contiguous extent, aligned as the pipe kernels need
    (8 elements of 16 bit, 4 of fp32) unless c.odd."""
    p = 4 if c.dtype == F32 else 8
    return {"lda": (c.K if c.al == KC else c.M) + p, "ldb": (c.K if c.bl == KC else c.N) + p, "ldt": c.N + 4, "ldr": c.N + 4,
            "ldaux": c.N + p, "ldo32": c.N + 4, "ldo": c.N + (4 if c.odd else p), "ldo2": c.N + 2 * p}


def ws_floats(c):
    return 8 * (c.M * c.N + c.M)


def inputs(c, seed=None):
    """The operands of case c on the CPU, fp32 and exactly representable in c.dtype where the kernel reads c.dtype: A [M, K],
    B [N, K] (logical), alpha, bias [N], table [9, N], tab_row [M], dst_row [M] (a permutation into M + 5 rows, one -1),
    resid [M + 5, N] (or [M, N]), aux [M, N].  Contrast: rows of A are scaled per 16-row fragment and rows of B (output columns)
    per 8-wide piece by powers of two (exact in every format), so a fragment or piece that lands in the wrong place is orders of
    magnitude off where it lands; an asymmetric integer block sits in A's corner.  "pos" cases: positive operands and bias at unit
    scales (every element then weighs the same in the mean signed error)."""
    M, N, K = c.M, c.N, c.K
    g = torch.Generator().manual_seed(seed if seed is not None else M * 131 + N * 17 + K + c.tile % 1000 + 7 * c.al + 3 * c.bl)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.2
    t = {"alpha": 0.5 if has(c, "alpha") else 1.0}
    if c.kind == "pos":
        A, B = A.abs() + 0.25, B.abs() + 0.05
    else:
        ea, eb = CONTRAST[c.dtype]
        A = A * torch.tensor([2.0 ** e for e in ea])[(torch.arange(M) // 16) % len(ea)][:, None]
        B = B * torch.tensor([2.0 ** e for e in eb])[(torch.arange(N) // 8) % len(eb)][:, None]
        r, k = min(16, M), min(16, K)
        A[:r, :k] = (torch.arange(256).reshape(16, 16).float() % 7 - 3)[:r, :k]
    t["A"], t["B"] = A.to(c.dtype).float(), B.to(c.dtype).float()
    if has(c, "bias"):
        t["bias"] = torch.randn(N, generator=g)
        if c.kind == "pos":
            t["bias"] = t["bias"].abs() + 0.25
    if has(c, "table"):
        t["table"] = torch.randn(TABLE_ROWS, N, generator=g)
        t["tab_row"] = torch.randint(0, TABLE_ROWS, (M,), generator=g, dtype=torch.int32)
    if has(c, "dst"):
        t["dst_row"] = torch.randperm(M + EXTRA_ROWS, generator=g)[:M].to(torch.int32)
        t["dst_row"][min(3, M - 1)] = -1
    if has(c, "resid"):
        t["resid"] = torch.randn(out_rows(c), N, generator=g)
    if has(c, "aux"):
        t["aux"] = (3.0 * torch.randn(M, N, generator=g)).to(c.dtype).float()
    return t


# ------------------------------------------------------------------------------------------------------------- statement
def phi_cdf(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def gelu64(x):
    return x * phi_cdf(x)


def dgelu64(x):
    return phi_cdf(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def dst_of(c, t):
    return t["dst_row"].long() if "dst_row" in t else torch.arange(c.M)


def place(c, t, x, fill=float("nan")):
    """[M, N] in the order of A's rows -> [out_rows, N] at dst(m); rows nobody writes hold `fill`."""
    dst = dst_of(c, t)
    keep = dst >= 0
    out = torch.full((out_rows(c), x.shape[1]), fill, dtype=x.dtype)
    out[dst[keep]] = x[keep]
    return out


def reference(c, t):
    """fp64 value of every output of the call ({name: [out_rows, N]}, NaN in the rows the call does not write; "colsum": [M])
    and the magnitudes the bar is made of."""
    A, B = t["A"].double(), t["B"].double()
    acc = A @ B.T
    mag = A.abs() @ B.abs().T
    alpha = t["alpha"]
    v = alpha * acc
    T = v.abs()
    n_add = 0
    dst = dst_of(c, t)
    keep = dst >= 0
    for name in ("bias", "table", "resid"):
        if name not in t:
            continue
        if name == "bias":
            x = t["bias"].double()[None, :].expand_as(v)
        elif name == "table":
            x = t["table"].double()[t["tab_row"].long()]
        else:
            x = torch.zeros_like(v)
            x[keep] = t["resid"].double()[dst[keep]]
        v = v + x
        T = T + x.abs()
        n_add += 1
    e_v = c.K * U32 * abs(alpha) * mag + n_add * U32 * T
    fam = planned(c)["family"]
    e_cdf = E_CDF_ERFF if fam == "fallback" else E_CDF_PIPE
    if c.epi == "gelu":
        y = gelu64(v)
        rest = e_cdf * v.abs() + GELU_SLOPE * e_v + 2 * U32 * y.abs()
    elif c.epi == "dgelu":
        y = v * dgelu64(t["aux"].double())
        rest = e_cdf * v.abs() + GELU_SLOPE * e_v + 2 * U32 * y.abs()
    else:
        y, rest = v, e_v
    ref, rests = {}, {}
    for name in ("out_f32", "out"):
        if has(c, name):
            ref[name], rests[name] = place(c, t, y), place(c, t, rest)
    if has(c, "out2"):
        ref["out2"], rests["out2"] = place(c, t, v), place(c, t, e_v)
    if has(c, "colsum"):
        ref["colsum"], rests["colsum"] = A.sum(1), c.K * U32 * A.abs().sum(1)
    return {"ref": ref, "rest": rests, "v": v, "acc": acc}


def stored_dtype(c, name):
    return F32 if name in ("out_f32", "colsum") else c.dtype


def bars(c, st):
    """{name: elementwise bound on |kernel - ref|} (module docstring, item 4); NaN where the reference is."""
    out = {}
    for name, r in st["ref"].items():
        dt = stored_dtype(c, name)
        h = UNIT[dt]
        floor = TINY + (F16_SUB if dt == F16 else 0.0)
        out[name] = h * r.abs() + (1 + h) * st["rest"][name] + floor
    return out


def ratio(got, ref, bar):
    """max err / bar over the elements the call writes; inf when an element that must stay untouched (NaN in `ref`) is not NaN in
    `got`, or a written one is NaN."""
    unwritten = torch.isnan(ref)
    if not torch.equal(torch.isnan(got), unwritten):
        return math.inf
    w = ~unwritten
    return worst((got[w] - ref[w]).abs(), bar[w])


# ------------------------------------------------------------------------------------------------------------- emulation
def fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def gelu_parts32(x):
    """gemm_pipe.hip gelu_parts, operation by operation in fp32 (exp and the reciprocal to nearest): (cdf, gauss)."""
    x = x.float()
    z = x.abs() * torch.tensor(0.70710678118654752440, dtype=torch.float32)
    gauss = torch.exp(-0.5 * x * x)
    one = torch.ones_like(z)
    tt = one / fma32(torch.full_like(z, 0.3275911), z, one)
    p = fma32(torch.full_like(z, 1.061405429), tt, torch.full_like(z, -1.453152027))
    for coef in (1.421413741, -0.284496736, 0.254829592):
        p = fma32(p, tt, torch.full_like(z, coef))
    tail = 0.5 * p * tt * gauss
    return torch.where(x >= 0, 1.0 - tail, tail), gauss


def gelu32(x, pipe):
    if pipe:
        return x * gelu_parts32(x)[0]
    return 0.5 * x * (1.0 + torch.erf(x * torch.tensor(0.70710678118654752440, dtype=torch.float32)))


def dgelu32(x, pipe):
    if pipe:
        cdf, gauss = gelu_parts32(x)
        return fma32(x * torch.tensor(0.39894228040143267794, dtype=torch.float32), gauss, cdf)
    cdf = 0.5 * (1.0 + torch.erf(x * torch.tensor(0.70710678118654752440, dtype=torch.float32)))
    return cdf + x * (torch.tensor(0.39894228040143267794, dtype=torch.float32) * torch.exp(-0.5 * x * x))


MUTANTS = ("trunc", "gelu_rounded", "tanh", "bias_after", "alpha_bias", "resid_m", "tab_dst", "swap_k")


def emulate(c, t, mutant=None):
    """The kernels' arithmetic in torch on the CPU: fp32 accumulation in 64-wide k-tiles, alpha, the adds in the kernels' order,
    gelu_parts (pipe) or erf (fallback) in fp32, one rounding to the stored type.  mutant: one of MUTANTS, a subtly wrong kernel.
    Returns {name: fp64} shaped like reference()'s."""
    assert mutant is None or mutant in MUTANTS
    A, B = t["A"], t["B"]
    M, N, K = c.M, c.N, c.K
    pipe = planned(c)["family"] != "fallback"
    order = list(range(0, K, 64))
    acc = torch.zeros(M, N)
    for i, k0 in enumerate(order):
        kb = k0
        if mutant == "swap_k" and i < 2:
            kb = order[1 - i]                                     # B's first two k-tiles change places
        acc = acc + A[:, k0:k0 + 64] @ B[:, kb:kb + 64].T
    alpha = torch.tensor(t["alpha"], dtype=torch.float32)
    dst = dst_of(c, t)
    keep = dst >= 0
    v = acc * alpha
    bias = t.get("bias")
    if bias is not None and mutant != "bias_after":
        v = (acc + bias) * alpha if mutant == "alpha_bias" else v + bias
    if "table" in t:
        rows = t["tab_row"].long()
        if mutant == "tab_dst":
            rows = t["tab_row"].long()[dst.clamp(0, M - 1)]
        v = v + t["table"][rows]
    if "resid" in t:
        x = torch.zeros_like(v)
        if mutant == "resid_m":
            x = t["resid"][:M]
        else:
            x[keep] = t["resid"][dst[keep]]
        v = v + x
    rounding = "trunc" if mutant == "trunc" else "rne"
    if c.epi == "gelu":
        arg = round_to(v, c.dtype) if mutant == "gelu_rounded" else v
        if mutant == "tanh":
            y = 0.5 * arg * (1.0 + torch.tanh(0.7978845608028654 * (arg + 0.044715 * arg ** 3)))
        else:
            y = gelu32(arg, pipe)
    elif c.epi == "dgelu":
        y = v * dgelu32(t["aux"], pipe)
    else:
        y = v
    if bias is not None and mutant == "bias_after":
        y = y + bias
    res = {}
    for name in ("out_f32", "out"):
        if has(c, name):
            res[name] = place(c, t, round_to(y, stored_dtype(c, name), rounding).double())
    if has(c, "out2"):
        res["out2"] = place(c, t, round_to(v, c.dtype, rounding).double())
    if has(c, "colsum"):
        cs = torch.zeros(M)
        for k0 in order:
            cs = cs + A[:, k0:k0 + 64].sum(1)
        res["colsum"] = cs.double()
    return res


# ------------------------------------------------------------------------------------------------------------- launch plan
def _cdiv(a, b):
    return -(-a // b)


def gemm256_applicable(c, split):
    return (c.al == KC and not has(c, "dst") and not has(c, "table") and not has(c, "colsum") and split <= 1 and c.K % 64 == 0 and
            c.K >= 128 and c.M % 8 == 0 and c.M >= 8 and c.N % 8 == 0 and (c.bl == KC or c.N % 128 == 0))


def gemm256_wgrad_applicable(c, split):
    return (c.al == RC and c.bl == RC and not has(c, "dst") and not has(c, "table") and split <= 1 and c.K % 64 == 0 and c.K >= 128 and
            c.M % 256 == 0 and c.N % 256 == 0 and c.M >= 256 and c.N >= 256)


def _split_factor(c, M, tiles, want, min_steps, ws_bytes):
    KT = c.K // 64
    S = want if want > 1 else 768 // tiles
    S = min(S, 8)
    if want <= 1:
        S = min(S, KT // min_steps)
    S = min(S, KT)
    while S > 1 and S * (M * c.N + M) * 4 > ws_bytes:
        S -= 1
    return max(S, 1)


def planned(c):
    """What skyemb_gemm does with case c (gemm.hip skyemb_gemm, gemm_pipe.hip plan_single, with the default switches):
    {"family": fallback | pipe | tile256 | splitk | refused, "tile": code (fallback: 64 / 128), "split": S,
     "parts": [(tile, S, row0, rows), ...], "counts": launches per ops.GEMM_COUNT_NAMES family}.  family = splitk: a pipe launch plus
    the reduce kernel."""
    ld = lds(c)
    M, N, K = c.M, c.N, c.K
    a_kc, b_kc = c.al == KC, c.bl == KC

    def fallback():
        tile = c.tile if c.tile else (128 if _cdiv(M, 128) * _cdiv(N, 128) >= 200 else 64)
        tile = 128 if tile == 128 else 64
        return {"family": "fallback", "tile": tile, "split": 1, "parts": [(tile, 1, 0, M)],
                "counts": {"fallback": 1, "pipe": 0, "tile256": 0, "splitk": 0}}

    used = {"ldo32": has(c, "out_f32"), "ldo": has(c, "out"), "ldo2": has(c, "out2"), "ldr": has(c, "resid"), "ldt": has(c, "table"),
            "ldaux": has(c, "aux")}
    eff = {k: (ld[k] if used[k] else (0 if k in ("ldr", "ldt", "ldaux") else N)) for k in used}     # ops.gemm_args defaults
    if c.dtype == F32 or K % 64 or N % 8:
        return fallback()
    if eff["ldo32"] % 4 or eff["ldo"] % 8 or eff["ldo2"] % 8 or eff["ldr"] % 4 or eff["ldt"] % 4 or eff["ldaux"] % 8:
        return fallback()
    if (not a_kc and (M % 8 or M < 8)) or (not b_kc and (N % 8 or N < 8)):
        return fallback()
    KT = K // 64
    ws_bytes = ws_floats(c) * 4 if c.ws else 0
    tile = LEGACY.get(c.tile, c.tile)
    want = c.split
    if tile == 0 and want == 0:
        for tm, tn, tk, ta, tb, tt, ts in TUNED:
            if (tm, tn, tk, ta, tb) == (M, N, K, int(a_kc), int(b_kc)) and (ts == 1 or c.ws):
                tile, want = LEGACY.get(tt, tt), ts
                break
    t12864, t128 = _cdiv(M, 128) * _cdiv(N, 64), _cdiv(M, 128) * _cdiv(N, 128)
    if tile == 0 and c.split <= 1 and gemm256_applicable(c, c.split):
        R, C = _cdiv(M, 256), _cdiv(N, 256)
        T = R * C
        over = T % 256
        tail_ok = (over > 0 and over <= C and (R - 1) * C % 256 == 0 and
                   (c.ws or (KT % 2 == 0 and K <= 2048 and _cdiv(M - (R - 1) * 256, 64) * _cdiv(N, 64) <= 256)))
        if T >= 512 and N % 256 == 0 and (over == 0 or over >= 214 or tail_ok):
            tile = T256
    if tile == 0 and a_kc and ((t128 >= 512 and K >= 2048) or (t128 >= 2048 and N >= 4096)):
        tile = 2256128
    if tile == 0 and (t128 >= 1024 or (t128 >= 512 and K >= 1024)):
        tile = 128128
    if tile == 0 and (t12864 >= 2048 or (t12864 >= 1024 and K >= 1024)):
        tile = 128064
    if tile == 0:
        tile = 64064
    if (tile == 64064 and c.tile == 0 and c.split <= 1 and a_kc and not has(c, "colsum") and KT % 2 == 0 and KT >= 4 and
            _cdiv(M, 64) * _cdiv(N, 64) <= 256):
        tile, want = 9064064, 1
    refused = {"family": "refused", "tile": tile, "split": 1, "parts": [], "counts": {"fallback": 0, "pipe": 0, "tile256": 0, "splitk": 0}}
    if tile not in TILES:
        return refused
    bm, bn, stride, wk = TILES[tile]
    S = 1
    if c.ws and want != 1:
        S = _split_factor(c, M, _cdiv(M, stride) * _cdiv(N, bn), want, 10 if (not a_kc and not b_kc) else 12, ws_bytes)
    if tile == T256 and (c.split > 1 or S > 1 or not (gemm256_applicable(c, c.split) or gemm256_wgrad_applicable(c, c.split))):
        return refused
    if tile != T256:                                              # gemm_pipe.hip dispatch
        pow2 = lambda r: r in (64, 128, 256)
        built = (a_kc and b_kc) or (a_kc and not b_kc and pow2(bn)) or (not a_kc and not b_kc and pow2(bm) and pow2(bn)) or \
                (not a_kc and b_kc and pow2(bm))
        if not built or (wk == 2 and KT % 2):
            return refused
    parts = [(tile, S, 0, M)]
    tail_wk2 = KT % 2 == 0 and K <= 2048
    if (tile in (128128, 2256128, T256) and S == 1 and a_kc and (c.ws or tail_wk2) and not has(c, "dst") and not has(c, "table") and
            not has(c, "colsum")):
        bm_t, slots = (128, 512) if tile == 128128 else (256, 256)
        R, C = _cdiv(M, bm_t), _cdiv(N, bn)
        full = R * C // slots * slots
        Rm = full // C
        tail_tiles = (R - Rm) * C
        r0 = Rm * bm_t
        t64 = _cdiv(M - r0, 64) * _cdiv(N, 64)
        if (Rm >= 1 and Rm < R and tail_tiles <= 64 and full - Rm * C < C and (full <= 2 * slots or tile in (2256128, T256)) and
                (c.ws or t64 <= 256)):
            parts[0] = (tile, 1, 0, r0)
            if tail_wk2 and t64 <= 256:
                parts.append((9064064, 1, r0, M - r0))
            else:
                parts.append((64064, _split_factor(c, M - r0, t64, 0, 4, ws_bytes) if c.ws else 1, r0, M - r0))
    counts = {"fallback": 0, "pipe": 0, "tile256": 0, "splitk": 0}
    for pt, ps, _, _ in parts:
        counts["tile256" if pt == T256 else "pipe"] += 1
        counts["splitk"] += 1 if ps > 1 else 0
    fam = "tile256" if tile == T256 else ("splitk" if S > 1 else "pipe")
    return {"family": fam, "tile": tile, "split": S, "parts": parts, "counts": counts}


# ------------------------------------------------------------------------------------------------------------- case table
def _rows(tile, al, which):
    """Two ragged row counts per tile: one row (one 8-row piece for a row-contiguous A) past a tile, and 2 x stride - 7 (- 8)."""
    bm, _, stride, _ = TILES[tile]
    if al == RC:
        return (bm + 8, 2 * bm - 8)[which]
    if bm == 144:
        return (145, 2 * stride - 7, 2 * stride)[which]           # past one image; not a multiple of the stride; a multiple
    if tile == T256:
        return (264, 2 * 256 - 8)[which]                          # (k-contiguous A on this tile: M % 8 == 0)
    return (bm + 1, 2 * stride - 7)[which]


def _classes(tile):
    bm = TILES[tile][0]
    if bm == 144:
        return ((KC, KC), (KC, RC))
    if tile == T256:
        return ((KC, KC), (KC, RC))                               # + the whole-tile weight gradient, added by hand
    return ((KC, KC), (KC, RC), (RC, RC), (RC, KC))


def _cases():
    cs = []
    for dt in (BF, F16):
        for tile, (bm, bn, stride, wk) in TILES.items():
            k_short = 128 if (wk == 2 or tile == T256) else 64    # the shortest loop the tile accepts
            k_long = 384 if (wk == 2 or tile == T256) else 320    # wraps a 3-stage ring (two k-tiles per stage: 3 stages) more than once
            for al, bl in _classes(tile):
                n = bn + 8 if not (tile == T256 and bl == RC) else 384      # (256 x 256, row-contiguous B: N % 128 == 0)
                m0, m1 = _rows(tile, al, 0), _rows(tile, al, 1)
                m2 = _rows(tile, al, 2) if bm == 144 else m0
                cs.append(Case(dt, tile, al, bl, m0, n, k_short, "plain"))
                cs.append(Case(dt, tile, al, bl, m1, n, k_long, "resid" if tile == T256 else "full"))
                cs.append(Case(dt, tile, al, bl, m2, n, k_short, "gelu"))
                cs.append(Case(dt, tile, al, bl, m1, n, k_long, "dgelu"))
                if al == RC:
                    cs.append(Case(dt, tile, al, bl, m1, n, k_long, "colsum"))
        # 256 x 256: the weight gradient of whole tiles
        cs.append(Case(dt, T256, RC, RC, 256, 512, 128, "plain"))
        cs.append(Case(dt, T256, RC, RC, 512, 256, 384, "colsum"))
        # split-K with every epilogue: forced 2 and 5 on 64x64 and 128x128; N = 8 x odd: the reduce kernel's 4-wide pieces against
        # the tile kernel's 8-wide ones
        for tile in (64064, 128128):
            bm, bn = TILES[tile][:2]
            for split in (2, 5):
                for al, bl in ((KC, KC), (KC, RC)):
                    for epi in ("plain", "full", "gelu", "dgelu"):
                        cs.append(Case(dt, tile, al, bl, bm + 1, bn + 8, 320, epi, split, True))
                cs.append(Case(dt, tile, RC, RC, bm + 8, bn + 8, 320, "colsum", split, True))
        # ... and the automatic factor (a workspace, split_k = 0, few tiles, K = 1536 -> 2): the 64x64 tile named (left open, a
        # k-contiguous A goes to the two-k-group tile unsplit) and, for the weight gradient, left open
        for al, bl in ((KC, KC), (KC, RC)):
            for epi in ("plain", "full", "gelu", "dgelu"):
                cs.append(Case(dt, 64064, al, bl, 65, 72, 1536, epi, 0, True))
        cs.append(Case(dt, 0, RC, RC, 72, 72, 1536, "colsum", 0, True))
        # 16-bit problems outside the pipe subset (gemm.hip): K = 72, N = 8 k + 4, a misaligned ldo
        for tile in (64, 128):
            bm = tile
            for al, bl in ((KC, KC), (KC, RC), (RC, RC), (RC, KC)):
                n = bm + 8 if bl == RC else bm + 12
                m = bm + 8 if al == RC else bm + 1
                epis = ("plain", "full", "gelu", "dgelu") + (("colsum",) if al == RC else ())
                for epi in epis:
                    cs.append(Case(dt, tile, al, bl, m, n, 72, epi))
            cs.append(Case(dt, tile, KC, KC, bm + 1, bm + 8, 128, "gelu", odd=True))
            cs.append(Case(dt, tile, KC, RC, bm + 1, bm + 8, 128, "full", odd=True))
        # the row tail (the smallest shape for which plan_single emits two parts: test_row_tail_case_is_the_smallest): GELU with the
        # pre-activation, the one pair of outputs whose tail-row offsets the 8320-row tests of test_kernels_gpu.py do not reach
        if dt == BF:
            cs.append(Case(dt, 128128, KC, KC, 1025, 8072, 128, "gelu"))
    # fp32 (gemm.hip) at tiles 64 and 128 with every epilogue; N = 4 k + ... ragged against the 4-wide vectors
    for tile in (64, 128):
        for al, bl in ((KC, KC), (KC, RC), (RC, RC), (RC, KC)):
            n = tile + 8 if bl == RC else tile + 5
            m = tile + 4 if al == RC else tile + 1
            epis = ("plain", "full", "gelu", "dgelu") + (("colsum",) if al == RC else ())
            for i, epi in enumerate(epis):
                cs.append(Case(F32, tile, al, bl, m, n, 20 if i % 2 == 0 else 72, epi))
    # signed bias: one case per 16-bit dtype and kernel family, operands and bias positive
    for dt in (BF, F16):
        cs.append(Case(dt, 64, KC, KC, 121, 76, 72, "bias", kind="pos"))                          # fallback
        cs.append(Case(dt, 128064, KC, KC, 249, 72, 128, "bias", kind="pos"))                     # pipe
        cs.append(Case(dt, T256, KC, KC, 264, 264, 128, "bias", kind="pos"))                      # 256 x 256
        cs.append(Case(dt, 64064, KC, RC, 121, 72, 320, "bias", 2, True, kind="pos"))             # split-K
    return cs


CASES = _cases()
