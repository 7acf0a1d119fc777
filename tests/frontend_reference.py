"""High-precision statements of the kernels every batch passes through first -- the two mask generators, patch_gather, the
patch_mask_values gradient, clip_crop and tile_cutouts (frontend.hip), the augmentation pipeline (augment.hip) and
skyemb_topk_merge (topk.hip) -- with the bar each output element is held to and the case tables of
tests/test_frontend_elementwise_gpu.py.  Plain numpy / torch on the CPU, fp64 wherever there is arithmetic; nothing is imported
from the package under test.  Pinned on the CPU by tests/test_frontend_reference_cpu.py.

Bars.  u = 2^-24.
    masks        equality: stable ranks by np.lexsort((index, noise)) -> ids_restore, mask, ids_keep, dec_dst, dec_tab for n_extra
                 1 | 2; the SimMIM pixel mask with count = ceil(fp32(L (u max_ratio))).
    patch gather fp32: (x - mean) / std as one fp32 subtraction and one IEEE fp32 division, NaN -> pmv, layout (c, py, px): bit
                 equality.  16-bit: that value rounded once to nearest even (fp16: clamped to +-65504 first): bit equality.
    pmv gradient partial[b][e] = sum_j w d, dpmv[e] = sum_b partial[b][e], w = isnan(pixel), in fp64.  The products are exact
                 (w is 0 or 1); the kernel adds the keep terms of an image one after the other and then the B partials:
                 |partial - ref| <= keep u sum_j |w d|,  |dpmv - ref| <= (keep + B) u sum_bj |w d|  (forward error of the two
                 sequential fp32 sums: derived, not measured).  Where the sum of |w d| is zero the output is exactly zero.
    augmentation ref64 = flips, slice, interpolate(bilinear, align_corners=False, antialias=True) on float64, brightness, noise,
                 NaN channels.  |got - ref64| <= AUG_K u (|brightness| sum|w_yx src_yx| + |noise sigma|) with the tap weights w
                 recomputed in fp64 by the formula in the header of augment.hip (aa_weights).  AUG_K = 4 x the worst such ratio
                 of the fp32 CPU oracle (oracle/augment_oracle.py) over AUG_CASES, rounded up: the margin is for computing the
                 weights and the two passes in another, equally valid fp32 order -- the tap centre scale (o + 0.5) is a number
                 of the size of S and carries an fp32 rounding of S u into weights of the size of 1, which is why the ratio is
                 not of the order of 1.  The NaN pattern equals the reference's; copy 0 of a sample is the input bit for bit.
    clip / crop, cutouts   slices and two comparisons in fp32: equality of the int32 views (NaN payloads, -0.0, the clip value's own
                 bits wherever a clip applied).
    merge        the valid prefix of every list (up to its first negative index: include/skyemb.h leaves the slots behind the
                 terminator unspecified), np.lexsort by (score descending, index ascending), the first k, padded with (-inf, -1):
                 equality of scores and indices.
What the kernels achieve on the GPU is recorded by tests/test_frontend_elementwise_gpu.py (record_parity "frontend_elementwise"):
augmentation 0.25 of the bar at S = 20 and 0.014 at S = 64 and S = 8, the gradient 0.50 (partial) and 0.25 (dpmv) when written.
"""
import math
from collections import namedtuple

import numpy as np
import torch

U32 = 2.0 ** -24
F32, BF, F16 = torch.float32, torch.bfloat16, torch.float16
DT = {F32: "f32", BF: "bf16", F16: "f16"}
NAN, INF = float("nan"), float("inf")

# worst |oracle32 - ref64| / (u (|brightness| sum|w src| + |noise sigma|)) of oracle/augment_oracle.py over AUG_CASES, measured on
# the CPU (tests/test_frontend_reference_cpu.py::test_fp32_augmentation_oracle_stays_under_a_quarter_of_the_bar holds the oracle
# to AUG_K / 4, so that neither figure drifts), and the bar's constant AUG_K = ceil(4 x AUG_ORACLE_WORST)
AUG_ORACLE_WORST = 56.8       # measured 56.77 at S = 20 (scale = 14 / 20 and 16 / 20 are not fp32 numbers); 3.1 at S = 64, 3.2 at S = 8
AUG_K = 228                    # ceil(4 x 56.8)


def bits(a):
    """The integer view of a float array (numpy or torch): what `equality of the int32 views` compares."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().contiguous()
        return a.view(torch.int32 if a.dtype == F32 else torch.int16).numpy()
    return np.ascontiguousarray(a).view(np.int32)


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar over the elements where ref is a number; 0 / 0 counts as 0, x / 0 as inf, and a NaN pattern that
    differs from the reference's as inf."""
    got, ref, bar = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bar, np.float64)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return math.inf
    err = np.abs(got - ref)[~nan]
    b = np.broadcast_to(bar, ref.shape)[~nan]
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------- masks
MASK_B = (1, 7)
MASK_L = (16, 100, 256, 1024, 4096)          # 4096: the limit of include/skyemb.h, 64 KB of LDS
MASK_LIMIT_L = 4096
MASK_CASES = [(B, L, keep, E) for B in MASK_B for L in MASK_L for keep in (1, L // 4, L) for E in (1, 2)]


def mask_id(c):
    return "B%d-L%d-keep%d-extra%d" % c


def mask_noise(B, L):
    """Uniform noise; row 0 holds an exact tie (the lower index ranks first), and with B = 7 row 2 is tied throughout (the identity
    shuffle), row 3 takes eight values only (long runs of ties) and row 5 holds -0.0 and 0.0, which compare equal."""
    g = np.random.default_rng(1000 * B + L)
    noise = g.random((B, L), dtype=np.float32)
    noise[0, 3] = noise[0, 1]
    if B > 5:
        noise[2, :] = 0.5
        noise[3] = np.floor(noise[3] * 8) / 8
        noise[5, 2], noise[5, L - 1] = 0.0, -0.0
    return noise


def stable_ranks(noise):
    """-> (order, rank) along the last axis: order = the stable argsort by np.lexsort((index, noise)), rank its inverse."""
    idx = np.broadcast_to(np.arange(noise.shape[-1]), noise.shape)
    order = np.lexsort((idx, noise), axis=-1)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, idx, axis=-1)
    return order, rank


def mask_reference(noise, keep, n_extra):
    """-> ids_restore i64 [B, L], mask f32 [B, L] (1 = removed), ids_keep i32 [B, keep], dec_dst / dec_tab i32 [B, n_extra + keep]."""
    B, L = noise.shape
    E = n_extra
    order, rank = stable_ranks(noise)
    ids_keep = order[:, :keep].astype(np.int32)
    tab = np.concatenate([np.broadcast_to(np.arange(E), (B, E)), E + ids_keep], axis=1).astype(np.int32)
    dst = (tab + np.arange(B)[:, None] * (L + E)).astype(np.int32)
    return {"ids_restore": rank.astype(np.int64), "mask": (rank >= keep).astype(np.float32), "ids_keep": ids_keep, "dec_dst": dst,
            "dec_tab": tab}


# (grid, p, C): L = grid^2.  SIMMIM_LDS_CASES ask for more than 64 KB of LDS (32 L bytes; from L = 2049) and have a test of their own
SIMMIM_CASES = [(4, 16, 9), (10, 4, 1), (16, 8, 5), (45, 4, 2)]
SIMMIM_LDS_CASES = [(46, 4, 2), (64, 4, 1)]
SIMMIM_RATIOS = (0.6, 1.0)


def simmim_id(c):
    return "grid%d-p%d-C%d" % c


def simmim_inputs(B, C, L):
    """noise [B, C, L] with a tied and an all-tied row, ratio draws u [B] that include 0 and 0.999999 (B = 1: 0.999999)."""
    g = np.random.default_rng(100 * L + 10 * C + B)
    noise = g.random((B, C, L), dtype=np.float32)
    noise[0, 0, 3] = noise[0, 0, 9]
    u = g.random(B, dtype=np.float32)
    if B > 3:
        noise[1, C - 1, :] = 0.5
        u[2], u[3] = 0.0, 0.999999
    else:
        u[0] = 0.999999
    return noise, u


def simmim_count(L, u, max_ratio):
    """int(torch.ceil(torch.tensor(L * (u * max_ratio)))): the product in double, rounded to fp32, then the ceiling."""
    return int(np.ceil(np.float32(L * (float(u) * max_ratio))))


def simmim_reference(noise, u, max_ratio, grid, p):
    """-> float 0 / 1 [B, C, grid p, grid p]: per channel the `count` patches of smallest noise (ties by index), as pixels."""
    B, C, L = noise.shape
    _, rank = stable_ranks(noise)
    count = np.array([simmim_count(L, u[b], max_ratio) for b in range(B)])
    mk = (rank < count[:, None, None]).astype(np.float32).reshape(B, C, grid, grid)
    return np.repeat(np.repeat(mk, p, axis=2), p, axis=3)


# ------------------------------------------------------------------------------------------------------------- patch gather
PG_MEAN, PG_STD = 0.2, 1.7
PG_B = 3
PG_GEOMS = [(5, 64, 64, 16), (9, 32, 64, 8), (1, 16, 32, 4), (3, 48, 32, 16)]       # (C, H, W, p)


def pg_keeps(geom):
    """(keep, with ids_keep): 1, 3 and 6 kept patches through ids_keep (the gradient's four-at-a-time tail has 1, 3 and 2 live
    lanes) and all L in order with ids_keep = NULL."""
    C, H, W, p = geom
    return [(1, True), (3, True), (6, True), ((H // p) * (W // p), False)]


PG_CASES = [(g, k, ids) for g in PG_GEOMS for k, ids in pg_keeps(g)]


def pg_id(c):
    (C, H, W, p), keep, ids = c
    return f"C{C}-{H}x{W}-p{p}-keep{keep}" + ("" if ids else "-all")


def pg_inputs(geom, keep, with_ids):
    """imgs [3, C, H, W]: image 0 has a NaN channel and a NaN block, image 1 +-inf and values that leave the fp16 range once
    normalised (+-1e6; 111400 -> 65529, which rounds to the fp16 infinity if it is not clamped), image 2 no NaN at all; pmv
    [C, p, p]; ids_keep i32 [3, keep] (a random subset in random order) or None; drows [3 keep, C p p]."""
    C, H, W, p = geom
    L = (H // p) * (W // p)
    g = np.random.default_rng(C * 1000 + H + W + p + keep)
    x = g.standard_normal((PG_B, C, H, W), dtype=np.float32)
    x[0, C - 1] = np.nan
    x[0, 0, 3:9, 2:14] = np.nan
    x[1, 0, 0, 0:8] = [np.inf, -np.inf, 1e6, -1e6, 111400.0, -111400.0, 111360.0, np.nan]
    x[1, C - 1, H - 1, W - 4:] = [-np.inf, 1e6, np.inf, -1e6]
    pmv = g.standard_normal((C, p, p), dtype=np.float32)
    ids = np.stack([g.permutation(L)[:keep] for _ in range(PG_B)]).astype(np.int32) if with_ids else None
    if ids is not None:                                    # the patches of image 1 that hold the extreme values are among the kept
        ids[1] = ([0, L - 1] + [int(v) + 1 for v in g.permutation(L - 2)])[:keep]
    drows = g.standard_normal((PG_B * keep, C * p * p), dtype=np.float32)
    return {"imgs": x, "pmv": pmv, "ids_keep": ids, "drows": drows}


def pg_patches(a, ids_keep, p):
    """[B, C, H, W] -> [B keep, C p p]: rows of the kept patches (all, in order, for ids_keep None), elements in (c, py, px) order."""
    B, C, H, W = a.shape
    gh, gw = H // p, W // p
    pat = a.reshape(B, C, gh, p, gw, p).transpose(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, C * p * p)
    if ids_keep is not None:
        pat = np.take_along_axis(pat, ids_keep.astype(np.int64)[:, :, None], axis=1)
    return pat.reshape(-1, C * p * p)


def pg_reference(t, p, dtype):
    """-> the rows as a torch tensor of `dtype`."""
    x, pmv = t["imgs"], t["pmv"]
    B, C, H, W = x.shape
    with np.errstate(invalid="ignore"):
        v = (x - np.float32(PG_MEAN)) / np.float32(PG_STD)                                   # one fp32 subtraction, one IEEE division
    assert v.dtype == np.float32
    v = np.where(np.isnan(x), np.tile(pmv, (1, H // p, W // p))[None], v)
    rows = pg_patches(v, t["ids_keep"], p)
    if dtype == F16:
        rows = np.clip(rows, np.float32(-65504.0), np.float32(65504.0))
    return torch.from_numpy(np.ascontiguousarray(rows)).to(dtype)                            # (one rounding to nearest even)


def pmv_grad_reference(t, p):
    """-> ({partial [B, C p p], dpmv [C p p]} fp64, bars of the same names)."""
    x, d = t["imgs"], t["drows"].astype(np.float64)
    B = x.shape[0]
    w = pg_patches(np.isnan(x).astype(np.float64), t["ids_keep"], p)
    keep = w.shape[0] // B
    wd = (w * d).reshape(B, keep, -1)
    mag = np.abs(wd).sum(1)
    return ({"partial": wd.sum(1), "dpmv": wd.sum((0, 1))},
            {"partial": keep * U32 * mag, "dpmv": (keep + B) * U32 * mag.sum(0)})


# ------------------------------------------------------------------------------------------------------------- augmentation
def aa_taps(in_size, out_size):
    """-> (W, span): fp64 tap weights [out_size, in_size] of the separable anti-aliased bilinear resize, by the formula in the header
    of augment.hip -- scale = in / out, support = max(scale, 1), centre = scale (o + 0.5), taps [centre - support + 0.5, centre +
    support + 0.5) clipped to the input, weight max(0, 1 - |(j - centre + 0.5) / support|), normalised -- and the taps read (a tap
    of weight zero inside the range is read too: a NaN there reaches the output).  A pass that does not resize (in == out) is
    skipped by interpolate: the pixel itself, and a NaN does not reach its neighbour."""
    if in_size == out_size:
        return np.eye(in_size), np.eye(in_size, dtype=bool)
    scale = in_size / out_size
    support = max(scale, 1.0)
    W = np.zeros((out_size, in_size))
    span = np.zeros((out_size, in_size), bool)
    for o in range(out_size):
        center = scale * (o + 0.5)
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = np.array([max(0.0, 1.0 - abs((j - center + 0.5) / support)) for j in range(lo, hi)])
        W[o, lo:hi] = w / w.sum()
        span[o, lo:hi] = True
    return W, span


def aa_weights(in_size, out_size):
    return aa_taps(in_size, out_size)[0]


AUG_SHAPES = [(2, 5, 64, 3), (1, 1, 20, 1), (1, 32, 8, 2), (3, 2, 36, 0)]                   # (B, C, S, A)
AUG_FLIPS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def aug_crops(S):
    """(top, left, h, w): the identity, one-pixel crops in two corners, one-row and one-column crops that end on the last column /
    row, and a general crop that ends on the last row and column."""
    h, w = S - S // 4 - 1, S - S // 5
    return [(0, 0, S, S), (0, 0, 1, 1), (S - 1, S - 1, 1, 1), (0, 3, 1, S - 3), (5, 0, S - 5, 1), (S - h, S - w, h, w)]


def aug_id(c):
    return "B%d-C%d-S%d-A%d" % c


def aug_inputs(shape):
    """-> imgs [B, C, S, S] and the launches of the shape: every crop of aug_crops under every flip combination is the parameter
    row of one augmented copy, B A of them per launch (A = 0: one launch of copies only).  Brightness alternates 0.8 / 1.25, sigma
    0 / 0.01; the first launch has noise = None; nan_mask sets the last channel (bit 31 at C = 32) on every third row and channel 0
    besides on every sixth.  Channel 0 of image 0 holds NaN pixels on the edges of the crops."""
    B, C, S, A = shape
    g = torch.Generator().manual_seed(S + C)
    imgs = torch.randn(B, C, S, S, generator=g)
    h, w = aug_crops(S)[-1][2:]
    for y, x in ((S - h, S - w + 2), (7, 0), (0, 5), (S - 1, S - 3), (S // 2, S // 2)):
        imgs[0, 0, y, x] = NAN
    rows = [(fh, fv) + crop for crop in aug_crops(S) for fh, fv in AUG_FLIPS]
    N = B * (1 + A)
    launches = []
    per = B * A
    n_launch = (len(rows) + per - 1) // per if per else 1
    for k in range(n_launch):
        params = torch.zeros(N, 8)
        params[:, 4:6] = S
        params[:, 6] = 1.0
        nan_mask = torch.zeros(N, dtype=torch.int32)
        slots = [n for n in range(N) if n % (1 + A) != 0]
        for j, n in enumerate(slots):
            r = (k * per + j) % len(rows)
            params[n] = torch.tensor(rows[r] + ((0.8, 0.0) if r % 2 == 0 else (1.25, 0.01)), dtype=torch.float32)
            if r % 3 == 2:
                m = 1 << (C - 1) | (1 if r % 6 == 5 else 0)
                nan_mask[n] = m - (1 << 32) if m >= 1 << 31 else m
        noise = None if k == 0 else torch.randn(N, C, S, S, generator=g)
        launches.append({"params": params, "nan_mask": nan_mask, "noise": noise})
    return imgs, launches


def aug_reference(imgs, launch, A):
    """-> (ref64 [B (1 + A), C, S, S] float64 with the NaNs the pipeline produces, bar / AUG_K of the same shape)."""
    B, C, S, _ = imgs.shape
    params, nan_mask, noise = launch["params"].double(), launch["nan_mask"], launch["noise"]
    N = B * (1 + A)
    ref = torch.empty(N, C, S, S, dtype=torch.float64)
    mag = torch.zeros(N, C, S, S, dtype=torch.float64)
    for n in range(N):
        b, a = divmod(n, 1 + A)
        x = imgs[b].double()
        if a == 0:
            ref[n] = x
            continue
        fh, fv, top, left, h, w, bright, sigma = params[n].tolist()
        top, left, h, w = int(top), int(left), int(h), int(w)
        if fh:
            x = x.flip(-1)
        if fv:
            x = x.flip(-2)
        crop = x[:, top:top + h, left:left + w]
        y = torch.nn.functional.interpolate(crop[None], size=(S, S), mode="bilinear", align_corners=False, antialias=True)[0]
        Wy, Wx = torch.from_numpy(aa_weights(h, S)), torch.from_numpy(aa_weights(w, S))
        m = Wy @ torch.nan_to_num(crop).abs() @ Wx.T * abs(bright)
        y = y * bright
        if noise is not None:
            y = y + noise[n].double() * sigma
            m = m + (noise[n].double() * sigma).abs()
        for c in range(C):
            if (int(nan_mask[n]) >> c) & 1:
                y[c] = NAN
        ref[n], mag[n] = y, m
    return ref, U32 * mag


# ------------------------------------------------------------------------------------------------------------- clip / crop, cutouts
CLIP_LO, CLIP_HI = -3.0, 2.5
CLIP_MODES = {"lo": (CLIP_LO, None), "hi": (None, CLIP_HI), "both": (CLIP_LO, CLIP_HI), "none": (None, None)}
CC_SHAPES = [(10, 72, 72, 64), (3, 71, 80, 64), (1, 64, 64, 64)]                            # (n_planes, Hs, Ws, size)
CC_CASES = [(s, m) for s in CC_SHAPES for m in CLIP_MODES] + [((540, 66, 65, 64), "both")]  # 2 211 840 outputs > 8192 x 256 threads
CC_GRID_THREADS = 8192 * 256
TC_TILE = (5, 200, 232)                                                                       # (C, H, W)
TC_BIG_ENDIAN = (1, 0, 1, 1, 0)
TC_CASES = [(S, 12, m) for S in (64, 20) for m in CLIP_MODES] + [(64, 210, "both")]          # 4 300 800 outputs > 16384 x 256 threads
TC_GRID_THREADS = 16384 * 256


def cc_id(c):
    return "n%d-%dx%d-size%d" % c[0] + "-" + c[1]


def tc_id(c):
    return "S%d-n%d-%s" % c


def special_pixels(a, g):
    """Sprinkle NaN (two payloads), +-inf and -0.0 over a float32 array, in place."""
    flat = a.reshape(-1)
    n = flat.size
    pos = g.permutation(n)[:max(5, n // 50) // 5 * 5].reshape(5, -1)
    flat[pos[0]] = np.nan
    flat[pos[1]] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    flat[pos[2]], flat[pos[3]], flat[pos[4]] = np.inf, -np.inf, -0.0
    return a


def clip_np(v, lo, hi):
    """The two comparisons in fp32; NaN compares false and stays."""
    v = v.copy()
    with np.errstate(invalid="ignore"):
        if lo is not None:
            v[v < np.float32(lo)] = np.float32(lo)
        if hi is not None:
            v[v > np.float32(hi)] = np.float32(hi)
    return v


def cc_inputs(shape):
    n, Hs, Ws, size = shape
    g = np.random.default_rng(Hs * Ws + n)
    return special_pixels(g.standard_normal((n, Hs, Ws), dtype=np.float32) * 3, g)


def cc_reference(src, size, lo, hi):
    """Centre crop [n, Hs, Ws] -> [n, size, size] (top = (Hs - size) // 2, left = (Ws - size) // 2), then the clip."""
    _, Hs, Ws = src.shape
    top, left = (Hs - size) // 2, (Ws - size) // 2
    return clip_np(np.ascontiguousarray(src[:, top:top + size, left:left + size]), lo, hi)


def tc_inputs(S, n):
    """-> (tile [C, H, W] float32 values, words [C, H, W] uint32 as resident in HBM (planes of TC_BIG_ENDIAN byte-swapped), h0, w0):
    the four corner windows first, random ones behind."""
    C, H, W = TC_TILE
    g = np.random.default_rng(S + n)
    tile = special_pixels(g.standard_normal((C, H, W), dtype=np.float32) * 3, g)
    words = tile.view(np.uint32).copy()
    for c in range(C):
        if TC_BIG_ENDIAN[c]:
            words[c] = words[c].byteswap()
    h0 = np.concatenate([[0, 0, H - S, H - S], g.integers(0, H - S + 1, n - 4)]).astype(np.int32)
    w0 = np.concatenate([[0, W - S, 0, W - S], g.integers(0, W - S + 1, n - 4)]).astype(np.int32)
    return tile, words, h0, w0


def tc_reference(tile, h0, w0, S, lo, hi):
    """out [n, C, S, S] = tile[:, h0[i] : h0[i] + S, w0[i] : w0[i] + S], then the clip."""
    return clip_np(np.stack([tile[:, h:h + S, w:w + S] for h, w in zip(h0, w0)]), lo, hi)


# ------------------------------------------------------------------------------------------------------------- merge
MERGE_CAP = 16384             # topk.hip MERGE_CAP: entries of one query the block sort holds; above, that query goes to the tournament
MERGE_WS_WORDS_PER_QUERY = 1  # ops.topk_merge: ws is int32 [Q]; nlists > 32 with a workspace -> the block sort
MERGE_SORT_MIN_LISTS = 33
MG = namedtuple("MG", "Q nlists k ws what", defaults=("",))
MERGE_CASES = [MG(Q, n, k, ws) for Q in (1, 5) for n in (1, 2, 32, 33, 200) for k in (1, 10, 100) for ws in (False, True)]
MERGE_CASES += [MG(2, 128, 128, True, "full query = MERGE_CAP entries: the last that sorts"),
                MG(2, 145, 113, True, "full query = MERGE_CAP + 1 entries: falls back to the tournament, the short one sorts"),
                MG(1, 40, 10, True, "an index above 2^32: falls back to the tournament")]
MERGE_KINDS = ("full", "ties", "short", "few", "none")       # query q of a Q = 5 case is of kind q; Q = 1: "mixed" (ties and short)


def merge_id(c):
    return f"Q{c.Q}-lists{c.nlists}-k{c.k}" + ("-ws" if c.ws else "")


def merge_inputs(c):
    """in_s f32 / in_i i64 [Q, nlists, k], every list sorted by (score descending, index ascending) and ended by (-inf, -1) when
    shorter than k.  Indices are unique within a query.  Kinds: full lists of random scores | full lists of scores from four values
    (ties across and inside lists) | lists of random length 0 .. k with valid-looking entries BEHIND the terminator | fewer than k
    entries in all lists together | none at all | mixed: ties and random lengths."""
    Q, nlists, k = c.Q, c.nlists, c.k
    g = np.random.default_rng(nlists * 1000 + k * 10 + Q)
    s = np.full((Q, nlists, k), -np.inf, np.float32)
    i = np.full((Q, nlists, k), -1, np.int64)
    total = nlists * k
    for q in range(Q):
        kind = "mixed" if Q == 1 else ("full", "short")[q] if Q == 2 else MERGE_KINDS[q]
        pool = g.permutation(4 * total + 16)[:2 * total].astype(np.int64)
        if c.what.startswith("an index") and q == 0:
            pool[0] = (1 << 33) + 5
        if kind in ("full", "ties"):
            lens = np.full(nlists, k)
        elif kind in ("short", "mixed"):
            lens = g.integers(0, k + 1, nlists)
        elif kind == "few":
            lens = np.zeros(nlists, np.int64)
            lens[g.permutation(nlists)[:min(nlists, max(k - 1, 0))]] = 1
            lens[np.cumsum(lens) > k - 1] = 0
        else:
            lens = np.zeros(nlists, np.int64)
        at = 0
        for l in range(nlists):
            n = int(lens[l])
            sc = (g.integers(0, 4, n) / 4.0 if kind in ("ties", "mixed") else g.standard_normal(n)).astype(np.float32)
            ix = pool[at:at + n]
            at += n
            o = np.lexsort((ix, -sc))
            s[q, l, :n], i[q, l, :n] = sc[o], ix[o]
            if kind in ("short", "mixed") and n + 1 < k:
                s[q, l, n + 1:], i[q, l, n + 1:] = 9.0, pool[total + l * k + n + 1:total + (l + 1) * k]
    return s, i


def merge_reference(s, i, k):
    """-> (scores f32 [Q, k], indices i64 [Q, k])."""
    Q, nlists, _ = s.shape
    out_s = np.full((Q, k), -np.inf, np.float32)
    out_i = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        sc, ix = [], []
        for l in range(nlists):
            neg = np.nonzero(i[q, l] < 0)[0]
            n = int(neg[0]) if neg.size else s.shape[2]
            sc.append(s[q, l, :n])
            ix.append(i[q, l, :n])
        sc, ix = np.concatenate(sc), np.concatenate(ix)
        o = np.lexsort((ix, -sc.astype(np.float64)))[:k]
        out_s[q, :o.size], out_i[q, :o.size] = sc[o], ix[o]
    return out_s, out_i
