"""Pins tests/frontend_reference.py on the CPU before any kernel is held to it: its statements against the oracles the project
already trusts (oracle/mae_oracle.py, augment_oracle.py, tile_oracle.py, tests/golden/maskgen.npz), the constant of the
augmentation bar against the fp32 oracle it was measured on, the fp64 tap weights against interpolate itself, and the case tables
against the kernel limits they are meant to cross."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import augment_oracle as ao
from oracle import mae_oracle as mo
from oracle import tile_oracle as to
from tests import frontend_reference as fr
from tests.helpers import GOLDEN


# ------------------------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("c", [c for c in fr.MASK_CASES if c[1] <= 1024], ids=fr.mask_id)
def test_mask_reference_equals_the_oracle(c):
    B, L, keep, E = c
    noise = fr.mask_noise(B, L)
    ref = fr.mask_reference(noise, keep, E)
    tok = torch.arange(B * L, dtype=torch.float32).reshape(B, L, 1)
    ratio = 1.0 - (keep + 0.5) / L                                     # int(L (1 - ratio)) == keep
    xm, mask_o, ids_o = mo.random_masking_from_noise(tok, ratio, torch.from_numpy(noise))
    assert xm.shape[1] == keep
    assert np.array_equal(ref["ids_restore"], ids_o.numpy()) and np.array_equal(ref["mask"], mask_o.numpy())
    assert np.array_equal(ref["ids_keep"], (xm[:, :, 0] - torch.arange(B)[:, None] * L).numpy().astype(np.int32))
    # the decoder maps: encoder token E + r of sample b lands on decoder row E + ids_keep[b, r]; the extra tokens keep their place
    assert np.array_equal(ref["dec_tab"][:, :E], np.broadcast_to(np.arange(E), (B, E)))
    assert np.array_equal(ref["dec_tab"][:, E:], ref["ids_keep"] + E)
    assert np.array_equal(ref["dec_dst"], ref["dec_tab"] + np.arange(B)[:, None] * (L + E))
    assert ref["mask"].sum(1).tolist() == [L - keep] * B
    if B > 5:
        assert np.array_equal(ref["ids_restore"][2], np.arange(L))   # the all-tied row: the identity


def test_mask_cases_reach_the_limit_of_the_header():
    assert max(c[1] for c in fr.MASK_CASES) == fr.MASK_LIMIT_L == 4096
    assert 4 * fr.MASK_LIMIT_L * 4 == 65536                            # mask_kernel: four rows of L floats
    for grid, p, C in fr.SIMMIM_CASES:
        assert 8 * grid * grid * 4 <= 65536
    for grid, p, C in fr.SIMMIM_LDS_CASES:
        assert 65536 < 8 * grid * grid * 4 <= 8 * fr.MASK_LIMIT_L * 4
    assert fr.SIMMIM_LDS_CASES[-1][0] ** 2 == fr.MASK_LIMIT_L
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "skyemb.h")).read()
    assert "Both generators take L <= 4096" in header


@pytest.mark.parametrize("max_ratio", fr.SIMMIM_RATIOS)
@pytest.mark.parametrize("c", fr.SIMMIM_CASES + fr.SIMMIM_LDS_CASES[:1], ids=fr.simmim_id)
def test_simmim_mask_reference_equals_the_oracle(c, max_ratio):
    grid, p, C = c
    for B in (1, 7):
        noise, u = fr.simmim_inputs(B, C, grid * grid)
        ref = fr.simmim_reference(noise, u, max_ratio, grid, p)
        want = mo.simmim_mask_from_noise(torch.from_numpy(noise), torch.from_numpy(u), max_ratio, p)
        assert np.array_equal(ref, want.numpy())
        if B == 7:
            assert ref[2].sum() == 0 and 0.0 in u and np.float32(0.999999) in u


def test_simmim_counts_equal_the_reference_generators():
    """tests/golden/maskgen.npz: masks the reference's own MaskGenerator drew and the ratio draw behind each."""
    z = np.load(os.path.join(GOLDEN, "maskgen.npz"))
    for key in sorted({k.rsplit("/", 1)[0] for k in z.files}):
        size, p, C, mx = key.split("/")[1].split("_")
        size, p, C, mx = int(size), int(p), int(C), float(mx)
        u, masks = z[key + "/u"], z[key + "/masks"]
        L = (size // p) ** 2
        noise = np.random.default_rng(2).random((len(u), C, L), dtype=np.float32)
        ref = fr.simmim_reference(noise, u, mx, size // p, p)
        assert ref.shape == masks.shape
        got = ref[:, :, ::p, ::p].sum((2, 3))
        assert np.array_equal(got, masks[:, :, ::p, ::p].sum((2, 3)))
        assert np.array_equal(got[:, 0], [fr.simmim_count(L, v, mx) for v in u])


# ------------------------------------------------------------------------------------------------------------- patch gather
@pytest.mark.parametrize("c", fr.PG_CASES, ids=fr.pg_id)
def test_patch_reference_equals_norm_inputs_and_the_nan_fill(c):
    (C, H, W, p), keep, with_ids = c
    t = fr.pg_inputs((C, H, W, p), keep, with_ids)
    assert (t["ids_keep"] is None) == (keep == (H // p) * (W // p) and not with_ids)
    cfg = mo.MAEConfig(img_size=H, patch_size=p, in_chans=C, pixel_mean=fr.PG_MEAN, pixel_std=fr.PG_STD)
    x = torch.from_numpy(t["imgs"])
    xn = mo.norm_inputs(x, cfg)
    xn = torch.where(torch.isnan(xn), torch.from_numpy(t["pmv"]).repeat(1, H // p, W // p).expand(fr.PG_B, -1, -1, -1), xn)
    L = (H // p) * (W // p)
    pat = xn.reshape(fr.PG_B, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(fr.PG_B, L, C * p * p)
    if with_ids:
        ids = torch.from_numpy(t["ids_keep"]).long()
        assert all(len(set(r.tolist())) == keep for r in ids)
        pat = torch.gather(pat, 1, ids[:, :, None].expand(-1, -1, C * p * p))
    want = pat.reshape(fr.PG_B * keep, -1)
    assert np.array_equal(fr.bits(fr.pg_reference(t, p, fr.F32)), fr.bits(want))
    assert np.array_equal(fr.bits(fr.pg_reference(t, p, fr.BF)), fr.bits(want.to(fr.BF)))
    half = fr.pg_reference(t, p, fr.F16)
    assert np.array_equal(fr.bits(half), fr.bits(want.clamp(-65504.0, 65504.0).to(fr.F16)))
    assert bool(torch.isfinite(half).all()) and float(half.max()) == 65504.0 and float(half.min()) == -65504.0
    assert bool(torch.isinf(want).any()) and not bool(torch.isinf(want.to(fr.F16)).all())
    assert bool(torch.isinf(want.to(fr.F16)).sum() > torch.isinf(want).sum())               # values the clamp alone keeps finite


def pmv_emulate(t, p, tail_bug=False):
    """pmv_partial_kernel + colsum in fp32, patch after patch; tail_bug: the weight of the last group's clamped lanes not zeroed."""
    x, d = t["imgs"], t["drows"]
    B = x.shape[0]
    w = fr.pg_patches(np.isnan(x).astype(np.float32), t["ids_keep"], p).reshape(B, -1, d.shape[1])
    d = d.reshape(w.shape)
    keep = w.shape[1]
    part = np.zeros((B, d.shape[2]), np.float32)
    for j0 in range(0, keep, 4):
        for u in range(4):
            j = min(j0 + u, keep - 1)
            if j0 + u < keep or tail_bug:
                part += w[:, j] * d[:, j]
    out = np.zeros(d.shape[2], np.float32)
    for b in range(B):
        out += part[b]
    return {"partial": part, "dpmv": out}


@pytest.mark.parametrize("c", fr.PG_CASES, ids=fr.pg_id)
def test_pmv_gradient_bar_holds_an_fp32_sum_and_not_a_doubled_tail(c):
    geom, keep, with_ids = c
    p = geom[3]
    t = fr.pg_inputs(geom, keep, with_ids)
    ref, bar = fr.pmv_grad_reference(t, p)
    good = pmv_emulate(t, p)
    assert all(fr.worst_ratio(good[n], ref[n], bar[n]) <= 1.0 for n in ref)
    assert not ref["partial"][2].any() and not bar["partial"][2].any() and not good["partial"][2].any()   # the image without NaN
    assert ref["partial"][0].any()
    if keep % 4:
        bad = pmv_emulate(t, p, tail_bug=True)
        assert fr.worst_ratio(bad["partial"], ref["partial"], bar["partial"]) > 1.0
        assert fr.worst_ratio(bad["dpmv"], ref["dpmv"], bar["dpmv"]) > 1.0
    assert {k % 4 for _, k, _ in fr.PG_CASES} >= {1, 2, 3, 0}


# ------------------------------------------------------------------------------------------------------------- augmentation
@pytest.mark.parametrize("n_in,n_out", [(64, 64), (1, 64), (47, 64), (52, 64), (61, 64), (14, 20), (16, 20), (17, 20), (5, 8), (7, 8),
                                        (3, 8), (26, 36), (29, 36), (31, 36)])
def test_tap_weights_sum_to_one_and_reproduce_interpolate(n_in, n_out):
    W = fr.aa_weights(n_in, n_out)
    assert np.abs(W.sum(1) - 1.0).max() <= 4e-16 and (W >= 0).all()
    assert ((W > 0).sum(1) <= 3).all()                                 # crops never exceed the output: at most three taps
    eye = torch.eye(n_in, dtype=torch.float64)
    # impulse images: column j of the weights is the response to an impulse at j, along either axis
    rows = torch.nn.functional.interpolate(eye[None, None], size=(n_out, n_in), mode="bilinear", align_corners=False, antialias=True)[0, 0]
    cols = torch.nn.functional.interpolate(eye[None, None], size=(n_in, n_out), mode="bilinear", align_corners=False, antialias=True)[0, 0]
    assert np.abs(rows.numpy() - W).max() <= 1e-15 and np.abs(cols.numpy() - W.T).max() <= 1e-15


@pytest.fixture(scope="module")
def aug_oracle_ratios():
    out = {}
    for shape in fr.AUG_SHAPES:
        B, C, S, A = shape
        imgs, launches = fr.aug_inputs(shape)
        worst = 0.0
        for la in launches:
            ref, bar1 = fr.aug_reference(imgs, la, A)
            got = ao.augment(imgs, la["params"], la["nan_mask"], la["noise"], A)
            assert torch.equal(torch.isnan(got), torch.isnan(ref))
            worst = max(worst, fr.worst_ratio(got.numpy(), ref.numpy(), bar1.numpy()))
            first = torch.arange(0, B * (1 + A), 1 + A)
            assert np.array_equal(fr.bits(got[first]), fr.bits(imgs)) and np.array_equal(fr.bits(ref[first].float()), fr.bits(imgs))
        out[shape] = worst
    return out


@pytest.mark.parametrize("shape", fr.AUG_SHAPES, ids=fr.aug_id)
def test_fp32_augmentation_oracle_stays_under_a_quarter_of_the_bar(aug_oracle_ratios, shape):
    print(fr.aug_id(shape), "oracle32 err / (u mag):", aug_oracle_ratios[shape])
    assert aug_oracle_ratios[shape] <= fr.AUG_K / 4


def test_augmentation_bar_constant_is_four_times_the_measured_ratio(aug_oracle_ratios):
    worst = max(aug_oracle_ratios.values())
    print("worst", worst)
    assert fr.AUG_K == math.ceil(4 * fr.AUG_ORACLE_WORST)
    assert 0.5 * fr.AUG_ORACLE_WORST <= worst <= fr.AUG_ORACLE_WORST   # the figure written in the module is the one measured


def test_augmentation_reference_is_the_weighted_sum_and_the_cases_cover_the_edges():
    shape = fr.AUG_SHAPES[0]
    B, C, S, A = shape
    imgs, launches = fr.aug_inputs(shape)
    seen = set()
    for la in launches:
        ref, bar1 = fr.aug_reference(imgs, la, A)
        for n in range(B * (1 + A)):
            if n % (1 + A) == 0:
                continue
            fh, fv, top, left, h, w, bright, sigma = la["params"][n].tolist()
            seen.add((int(fh), int(fv), int(top), int(left), int(h), int(w)))
            x = imgs[n // (1 + A)].double()
            x = x.flip(-1) if fh else x
            x = x.flip(-2) if fv else x
            (Wy, sy), (Wx, sx) = (tuple(torch.from_numpy(v) for v in fr.aa_taps(int(k), S)) for k in (h, w))
            crop = x[:, int(top):int(top) + int(h), int(left):int(left) + int(w)]
            y = Wy @ torch.nan_to_num(crop) @ Wx.T * bright
            if la["noise"] is not None:
                y = y + la["noise"][n].double() * sigma
            y[(sy.double() @ torch.isnan(crop).double() @ sx.double().T) > 0] = fr.NAN     # a NaN under any tap read, of weight zero too
            keep = [c for c in range(C) if not (int(la["nan_mask"][n]) >> c) & 1]
            # the weighted sum over the taps read has the reference's NaNs and its values to fp64 rounding
            assert torch.equal(torch.isnan(y[keep]), torch.isnan(ref[n][keep])), la["params"][n]
            assert float((torch.nan_to_num(y[keep]) - torch.nan_to_num(ref[n][keep])).abs().max()) <= 1e-13
    assert seen == {f + c for c in fr.aug_crops(S) for f in fr.AUG_FLIPS}
    assert launches[0]["noise"] is None and launches[1]["noise"] is not None
    # bit 31 at C = 32, a total that is no multiple of 256, a launch without augmented copies
    _, l32 = fr.aug_inputs(fr.AUG_SHAPES[2])
    assert any(int(m) < 0 for la in l32 for m in la["nan_mask"])
    assert any((B * (1 + A) * C * S * S) % 256 for B, C, S, A in fr.AUG_SHAPES) and any(A == 0 for *_, A in fr.AUG_SHAPES)


# ------------------------------------------------------------------------------------------------------------- clip / crop, cutouts
@pytest.mark.parametrize("c", fr.TC_CASES[:8], ids=fr.tc_id)
def test_cutout_reference_equals_the_oracle(c):
    S, n, mode = c
    lo, hi = fr.CLIP_MODES[mode]
    tile, words, h0, w0 = fr.tc_inputs(S, n)
    C, H, W = fr.TC_TILE
    ref = fr.tc_reference(tile, h0, w0, S, lo, hi)
    assert np.array_equal(fr.bits(ref), fr.bits(to.cutouts_np(tile, h0, w0, S, lo, hi)))
    assert {(int(a), int(b)) for a, b in zip(h0[:4], w0[:4])} == {(0, 0), (0, W - S), (H - S, 0), (H - S, W - S)}
    # the resident words: the planes marked big-endian decode to the tile through a byte swap, the others as they are
    assert 0 < sum(fr.TC_BIG_ENDIAN) < C
    for ch in range(C):
        dec = words[ch].byteswap() if fr.TC_BIG_ENDIAN[ch] else words[ch]
        assert np.array_equal(dec, tile[ch].view(np.uint32))
    if lo is not None:
        raw = fr.tc_reference(tile, h0, w0, S, None, None)
        with np.errstate(invalid="ignore"):
            assert (raw < lo).any() and np.array_equal(fr.bits(ref[raw < lo]), np.full((raw < lo).sum(), fr.bits(np.float32([lo]))[0]))
    assert np.isnan(ref).any() and np.isinf(ref).any() == (mode != "both") and (fr.bits(ref) == np.int32(-2 ** 31)).any()


@pytest.mark.parametrize("c", fr.CC_CASES[:-1], ids=fr.cc_id)
def test_clip_crop_reference(c):
    (n, Hs, Ws, size), mode = c
    lo, hi = fr.CLIP_MODES[mode]
    src = fr.cc_inputs((n, Hs, Ws, size))
    ref = fr.cc_reference(src, size, lo, hi)
    t = torch.from_numpy(src)
    top, left = (Hs - size) // 2, (Ws - size) // 2
    want = t[:, top:top + size, left:left + size].clone()
    if lo is not None:
        want[want < lo] = lo                                           # utils/dataloaders.py:293-300: NaN < x is False
    if hi is not None:
        want[want > hi] = hi
    assert np.array_equal(fr.bits(ref), fr.bits(want))
    assert np.isnan(ref).any() and (fr.bits(ref) == np.int32(-2 ** 31)).any()


def test_second_pass_cases_exceed_the_capped_grids():
    (n, Hs, Ws, size), _ = fr.CC_CASES[-1]
    assert fr.CC_GRID_THREADS < n * size * size < 2 * fr.CC_GRID_THREADS
    S, n, _ = fr.TC_CASES[-1]
    assert fr.TC_GRID_THREADS < n * fr.TC_TILE[0] * S * S < 2 * fr.TC_GRID_THREADS
    assert any((Hs - size) % 2 and Hs != Ws for (_, Hs, Ws, size), _ in fr.CC_CASES)


# ------------------------------------------------------------------------------------------------------------- merge
def test_merge_reference_on_a_hand_written_example():
    ninf = -np.inf
    s = np.array([[[0.9, 0.5, 0.5, ninf], [0.9, 0.5, ninf, 7.0], [ninf, 8.0, 8.0, 8.0]]], np.float32)
    i = np.array([[[7, 2, 30, -1], [3, 11, -1, 99], [-1, 5, 6, 8]]], np.int64)
    out_s, out_i = fr.merge_reference(s, i, 4)
    assert out_i.tolist() == [[3, 7, 2, 11]] and out_s.tolist() == [[np.float32(0.9), np.float32(0.9), 0.5, 0.5]]   # ties: lower index first
    out_s, out_i = fr.merge_reference(s, i, 7)
    assert out_i.tolist() == [[3, 7, 2, 11, 30, -1, -1]] and np.isneginf(out_s[0, 5:]).all()          # entries behind a terminator: not read
    out_s, out_i = fr.merge_reference(s[:, 2:], i[:, 2:], 4)
    assert out_i.tolist() == [[-1] * 4] and np.isneginf(out_s).all()


def test_merge_cases_cover_both_kernels_and_the_fall_backs():
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "sky_embeddings_amd", "csrc", "topk.hip")).read()
    assert f"constexpr int MERGE_CAP = {fr.MERGE_CAP};" in src and "nlists > 32 && ws != nullptr" in src
    assert fr.MERGE_SORT_MIN_LISTS == 33
    totals = {}
    for c in fr.MERGE_CASES:
        s, i = fr.merge_inputs(c)
        assert s.shape == (c.Q, c.nlists, c.k)
        valid = np.cumprod(i >= 0, axis=2).astype(bool)
        for q in range(c.Q):
            ix = i[q][valid[q]]
            assert len(set(ix.tolist())) == ix.size                     # unique indices: unique sort keys
            for l in range(c.nlists):
                n = int(valid[q, l].sum())
                o = np.lexsort((i[q, l, :n], -s[q, l, :n]))
                assert np.array_equal(o, np.arange(n))                  # every list sorted by (score descending, index ascending)
        totals[c] = valid.sum((1, 2))
        if c.Q == 5:
            t = totals[c]
            assert t[0] == t[1] == c.nlists * c.k and t[3] < c.k and t[4] == 0
            ref_s, ref_i = fr.merge_reference(s, i, c.k)
            assert (ref_i[3] < 0).any() and (ref_i[4] < 0).all()
            if c.nlists > 1 and c.k > 1:
                assert (np.diff(ref_s[1]) == 0).any() and 0 < t[2] < c.nlists * c.k
                assert (i[2][~valid[2]] >= 0).any()                    # valid-looking entries behind a terminator
    at_cap, above, wide = fr.MERGE_CASES[-3:]
    assert totals[at_cap][0] == fr.MERGE_CAP and totals[above][0] == fr.MERGE_CAP + 1 and totals[above][1] <= fr.MERGE_CAP
    assert (fr.merge_inputs(wide)[1] > 2 ** 32).sum() == 1 and wide.ws and wide.nlists >= fr.MERGE_SORT_MIN_LISTS
