"""GPU parity of the kernels every batch passes through first, ELEMENT BY ELEMENT: the two mask generators, patch_gather, the
patch_mask_values gradient, clip_crop and tile_cutouts (frontend.hip), the augmentation pipeline (augment.hip) and
skyemb_topk_merge (topk.hip) go through the C ABI, and every element of every output is held to the statement and the bar of
tests/frontend_reference.py (pinned on the CPU by tests/test_frontend_reference_cpu.py).  The cases are the smallest shapes at
which each branch and tail of the kernels is live; the case ids name them.

Outputs start as NaN (or -7 for integers) where the kernel promises to write everywhere, and carry a sentinel behind their end
where it must not write.  Each family records its worst err / bar (helpers.record_parity "frontend_elementwise"); the families
whose bar is equality record 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import frontend_reference as fr
from tests.frontend_reference import BF, F16, F32
from tests.helpers import record_parity

DEV = "cuda"
NAN = float("nan")
SENT = 12.5
PAD = 64


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
    record_parity("frontend_elementwise", {k: round(v, 4) for k, v in sorted(w.items())})


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def padded(shape, dtype=F32, fill=NAN):
    """-> (the output tensor of `shape`, its flat buffer with PAD sentinels behind the end)."""
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), fill, device=DEV, dtype=dtype)
    buf[n:] = SENT if dtype.is_floating_point else 77
    return buf[:n].view(*shape), buf


def untouched(buf):
    tail = buf[-PAD:]
    return bool((tail == (SENT if buf.dtype.is_floating_point else 77)).all())


def hold(worst, family, name, ratios):
    """Print and record the ratios of one case; all must be <= 1."""
    print(f"{name} err/bar {ratios}")
    for k, r in ratios.items():
        worst[f"{family}/{k}"] = max(worst.get(f"{family}/{k}", 0.0), r)
    bad = {k: r for k, r in ratios.items() if not r <= 1.0}
    assert not bad, (name, ratios)


def same_bits(got, ref):
    """Equality of the integer views; on failure the first differing elements."""
    g, r = fr.bits(got), fr.bits(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    if np.array_equal(g, r):
        return True
    at = np.argwhere(g != r)
    print(f"{len(at)} of {g.size} elements differ; first:", [(tuple(i), int(g[tuple(i)]), int(r[tuple(i)])) for i in at[:8]])
    return False


# ------------------------------------------------------------------------------------------------------------- masks
@pytest.fixture(scope="module")
def mask_data():
    cache = {}

    def get(B, L):
        if (B, L) not in cache:
            noise = fr.mask_noise(B, L)
            cache[B, L] = (noise, dev(noise))
        return cache[B, L]
    return get


@pytest.mark.parametrize("c", fr.MASK_CASES, ids=fr.mask_id)
def test_random_mask(ops, worst, mask_data, c):
    B, L, keep, E = c
    noise, noise_d = mask_data(B, L)
    ref = fr.mask_reference(noise, keep, E)
    ids, ids_b = padded((B, L), torch.int64, -7)
    mask, mask_b = padded((B, L))
    ids_keep, keep_b = padded((B, keep), torch.int32, -7)
    dd, dd_b = padded((B, keep + E), torch.int32, -7)
    dt, dt_b = padded((B, keep + E), torch.int32, -7)
    ops.random_mask_from_noise(noise_d, keep, ids, mask, ids_keep, dd, dt, n_extra=E)
    torch.cuda.synchronize()
    got = {"ids_restore": ids, "mask": mask, "ids_keep": ids_keep, "dec_dst": dd, "dec_tab": dt}
    for n, g in got.items():
        assert np.array_equal(g.cpu().numpy(), ref[n]), n
    assert all(untouched(b) for b in (ids_b, mask_b, keep_b, dd_b, dt_b))
    if E == 1:                                                          # the maps are optional: without them the rest is the same
        ids2, _ = padded((B, L), torch.int64, -7)
        mask2, _ = padded((B, L))
        keep2, _ = padded((B, keep), torch.int32, -7)
        ops.random_mask_from_noise(noise_d, keep, ids2, mask2, keep2)
        torch.cuda.synchronize()
        assert torch.equal(ids2, ids) and torch.equal(mask2, mask) and torch.equal(keep2, ids_keep)
    hold(worst, "mask", fr.mask_id(c), {"random": 0.0})


def run_simmim(ops, c, B, max_ratio):
    grid, p, C = c
    noise, u = fr.simmim_inputs(B, C, grid * grid)
    out, buf = padded((B, C, grid * p, grid * p))
    ops.simmim_mask_from_noise(dev(noise), dev(u), max_ratio, grid, p, out)
    torch.cuda.synchronize()
    ref = fr.simmim_reference(noise, u, max_ratio, grid, p)
    assert same_bits(out, ref) and untouched(buf)
    count = [fr.simmim_count(grid * grid, v, max_ratio) for v in u]
    assert np.array_equal(out[:, :, ::p, ::p].sum(dim=(2, 3)).cpu().numpy(), np.repeat(np.float32(count)[:, None], C, 1))


@pytest.mark.parametrize("max_ratio", fr.SIMMIM_RATIOS)
@pytest.mark.parametrize("B", fr.MASK_B)
@pytest.mark.parametrize("c", fr.SIMMIM_CASES, ids=fr.simmim_id)
def test_simmim_mask(ops, worst, c, B, max_ratio):
    run_simmim(ops, c, B, max_ratio)
    hold(worst, "mask", f"{fr.simmim_id(c)} B{B} {max_ratio}", {"simmim": 0.0})


@pytest.mark.parametrize("max_ratio", fr.SIMMIM_RATIOS)
@pytest.mark.parametrize("c", fr.SIMMIM_LDS_CASES, ids=fr.simmim_id)
def test_simmim_mask_above_64_kb_of_lds(ops, worst, c, max_ratio):
    """grid 46 (L = 2116: 67 712 bytes, the first square above 64 KB) and grid 64 (L = 4096: 131 072 bytes, the limit
    include/skyemb.h states): the kernel's dynamic-LDS limit is raised before the launch."""
    run_simmim(ops, c, 7, max_ratio)
    hold(worst, "mask", f"{fr.simmim_id(c)} {max_ratio}", {"simmim_lds": 0.0})


def test_mask_generators_refuse_rows_longer_than_the_header_states(ops):
    """L = 4097 (random masking) and grid 65 (SimMIM): refused with code 1 before any launch, skyemb_last_error set."""
    from sky_embeddings_amd._lib import SkyembError
    L = fr.MASK_LIMIT_L + 1
    noise = torch.rand(1, L, device=DEV)
    ids, ids_b = padded((1, L), torch.int64, -7)
    mask, mask_b = padded((1, L))
    keep, keep_b = padded((1, 4), torch.int32, -7)
    with pytest.raises(SkyembError, match=r"rc=1\): skyemb_random_mask_from_noise: bad shape B=1 L=4097"):
        ops.random_mask_from_noise(noise, 4, ids, mask, keep)
    grid = 65
    noise = torch.rand(1, 1, grid * grid, device=DEV)
    out, out_b = padded((1, 1, grid * 4, grid * 4))
    with pytest.raises(SkyembError, match=r"rc=1\): skyemb_simmim_mask_from_noise: bad arguments \(L=4225 grid=65 p=4\)"):
        ops.simmim_mask_from_noise(noise, torch.rand(1, device=DEV), 0.6, grid, 4, out)
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and bool(torch.isnan(mask).all()) and bool((keep == -7).all()) and bool(torch.isnan(out).all())
    assert all(untouched(b) for b in (ids_b, mask_b, keep_b, out_b))


# ------------------------------------------------------------------------------------------------------------- patch gather
@pytest.fixture(scope="module")
def pg_data():
    cache = {}

    def get(c):
        if c not in cache:
            t = fr.pg_inputs(*c)
            cache[c] = (t, {k: dev(v) for k, v in t.items()})
        return cache[c]
    return get


@pytest.mark.parametrize("dtype", [F32, BF, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("c", fr.PG_CASES, ids=fr.pg_id)
def test_patch_gather(ops, worst, pg_data, c, dtype):
    (C, H, W, p), keep, with_ids = c
    t, d = pg_data(c)
    out, buf = padded((fr.PG_B * keep, C * p * p), dtype)
    ops.patch_gather(d["imgs"], d["pmv"], d["ids_keep"], out, p, keep, fr.PG_MEAN, fr.PG_STD)
    torch.cuda.synchronize()
    ref = fr.pg_reference(t, p, dtype)
    assert same_bits(out, ref) and untouched(buf)
    if dtype == F16:
        assert bool(torch.isfinite(out).all())
    hold(worst, "patch_gather", f"{fr.pg_id(c)} {fr.DT[dtype]}", {fr.DT[dtype]: 0.0})


@pytest.mark.parametrize("c", fr.PG_CASES, ids=fr.pg_id)
def test_patch_mask_values_gradient(ops, worst, pg_data, c):
    (C, H, W, p), keep, with_ids = c
    t, d = pg_data(c)
    part, part_b = padded((fr.PG_B, C * p * p))
    dpmv, dpmv_b = padded((C, p, p))
    ops.patch_gather_bwd_pmv(d["imgs"], d["ids_keep"], d["drows"], part, dpmv, p, keep)
    torch.cuda.synchronize()
    ref, bar = fr.pmv_grad_reference(t, p)
    got = {"partial": part.cpu().numpy(), "dpmv": dpmv.cpu().numpy().reshape(-1)}
    assert not got["partial"][2].any()                                  # the image without a NaN: a row of zeros
    for n in got:
        assert not got[n][bar[n] == 0].any(), n                         # no contribution: exactly zero
    assert untouched(part_b) and untouched(dpmv_b)
    hold(worst, "pmv_grad", fr.pg_id(c), {n: fr.worst_ratio(got[n], ref[n], bar[n]) for n in got})


# ------------------------------------------------------------------------------------------------------------- augmentation
@pytest.mark.parametrize("shape", fr.AUG_SHAPES, ids=fr.aug_id)
def test_augmentation(ops, worst, shape):
    B, C, S, A = shape
    imgs, launches = fr.aug_inputs(shape)
    imgs_d = dev(imgs)
    N = B * (1 + A)
    first = torch.arange(0, N, 1 + A)
    ratios = {}
    for k, la in enumerate(launches):
        out, buf = padded((N, C, S, S))
        ops.augment(imgs_d, out, dev(la["params"]), dev(la["nan_mask"]), dev(la["noise"]), A)
        torch.cuda.synchronize()
        got = out.cpu()
        ref, bar1 = fr.aug_reference(imgs, la, A)
        assert untouched(buf)
        assert same_bits(got[first], imgs), "copy 0 is not the input"
        if not torch.equal(torch.isnan(got), torch.isnan(ref)):
            at = (torch.isnan(got) != torch.isnan(ref)).nonzero()
            print("NaN pattern differs at", at[:8].tolist(), "rows", la["params"][at[:8, 0]].tolist())
        r = fr.worst_ratio(got.numpy(), ref.numpy(), fr.AUG_K * bar1.numpy())
        if not r <= 1.0:
            e = ((got.double() - ref).abs() / (fr.AUG_K * bar1)).nan_to_num(nan=0.0)
            n = int(e.flatten().argmax()) // (C * S * S)
            print("launch", k, "worst row", n, la["params"][n].tolist(), float(e.max()))
        ratios[f"launch{k}"] = r
    hold(worst, "augment", fr.aug_id(shape), {f"S{S}": max(ratios.values())})


# ------------------------------------------------------------------------------------------------------------- clip / crop, cutouts
@pytest.fixture(scope="module")
def cc_data():
    cache = {}

    def get(shape):
        if shape not in cache:
            src = fr.cc_inputs(shape)
            cache[shape] = (src, dev(src))
        return cache[shape]
    return get


@pytest.mark.parametrize("c", fr.CC_CASES, ids=fr.cc_id)
def test_clip_crop(ops, worst, cc_data, c):
    from sky_embeddings_amd._lib import check, lib
    (n, Hs, Ws, size), mode = c
    lo, hi = fr.CLIP_MODES[mode]
    src, src_d = cc_data((n, Hs, Ws, size))
    out, buf = padded((n, size, size))
    check(lib().skyemb_clip_crop(src_d.data_ptr(), out.data_ptr(), n, Hs, Ws, size, 0.0 if lo is None else lo, 0.0 if hi is None else hi,
                                 int(lo is not None), int(hi is not None), torch.cuda.current_stream().cuda_stream), "skyemb_clip_crop")
    torch.cuda.synchronize()
    ref = fr.cc_reference(src, size, lo, hi)
    assert same_bits(out, ref) and untouched(buf)
    raw = fr.cc_reference(src, size, None, None)
    with np.errstate(invalid="ignore"):
        for v, hit in ((lo, raw < np.float32(-3.0) if lo is not None else None), (hi, raw > np.float32(2.5) if hi is not None else None)):
            if v is not None:                                           # wherever a clip applied: the clip value itself
                assert hit.any() and (fr.bits(out)[hit] == fr.bits(np.float32([v]))[0]).all()
    hold(worst, "clip_crop", fr.cc_id(c), {mode: 0.0})


@pytest.fixture(scope="module")
def tc_data():
    cache = {}

    def get(S, n):
        if (S, n) not in cache:
            tile, words, h0, w0 = fr.tc_inputs(S, n)
            cache[S, n] = (tile, h0, w0, dev(words.view(np.int32)), dev(h0), dev(w0))
        return cache[S, n]
    return get


@pytest.mark.parametrize("c", fr.TC_CASES, ids=fr.tc_id)
def test_tile_cutouts(ops, worst, tc_data, c):
    S, n, mode = c
    lo, hi = fr.CLIP_MODES[mode]
    tile, h0, w0, words_d, h0_d, w0_d = tc_data(S, n)
    C = tile.shape[0]
    out, buf = padded((n, C, S, S))
    ops.tile_cutouts(words_d, dev(np.int32(fr.TC_BIG_ENDIAN)), h0_d, w0_d, S, out, lo=lo, hi=hi)
    torch.cuda.synchronize()
    ref = fr.tc_reference(tile, h0, w0, S, lo, hi)
    assert same_bits(out, ref) and untouched(buf)
    raw = fr.tc_reference(tile, h0, w0, S, None, None)
    with np.errstate(invalid="ignore"):
        for v, hit in ((lo, raw < np.float32(-3.0) if lo is not None else None), (hi, raw > np.float32(2.5) if hi is not None else None)):
            if v is not None:
                assert hit.any() and (fr.bits(out)[hit] == fr.bits(np.float32([v]))[0]).all()
    hold(worst, "tile_cutouts", fr.tc_id(c), {mode: 0.0})


# ------------------------------------------------------------------------------------------------------------- merge
@pytest.mark.parametrize("c", fr.MERGE_CASES, ids=fr.merge_id)
def test_topk_merge(ops, worst, c):
    s, i = fr.merge_inputs(c)
    ref_s, ref_i = fr.merge_reference(s, i, c.k)
    out_s, s_b = padded((c.Q, c.k))
    out_i, i_b = padded((c.Q, c.k), torch.int64, -7)
    ws = torch.zeros(c.Q * fr.MERGE_WS_WORDS_PER_QUERY, dtype=torch.int32, device=DEV) if c.ws else None
    ops.topk_merge(dev(s), dev(i), c.Q, c.nlists, c.k, out_s, out_i, ws=ws)
    torch.cuda.synchronize()
    gi, gs = out_i.cpu().numpy(), out_s.cpu().numpy()
    if not np.array_equal(gi, ref_i):
        at = np.argwhere(gi != ref_i)
        print("indices differ at", [(tuple(a), int(gi[tuple(a)]), int(ref_i[tuple(a)])) for a in at[:8]])
    assert np.array_equal(gi, ref_i) and same_bits(out_s, ref_s)
    assert untouched(s_b) and untouched(i_b)
    hold(worst, "merge", fr.merge_id(c), {"ws" if c.ws else "nows": 0.0})
