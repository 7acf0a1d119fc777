"""Shared helpers for the parity tests (load goldens into oracle structures)."""
import os
from collections import OrderedDict

import numpy as np
import torch

from oracle import mae_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    img, patch, C, D, depth, heads, Dd, ddepth, dheads, norm_pix = [int(v) for v in z["cfg"]]
    cfg = mo.MAEConfig(img_size=img, patch_size=patch, in_chans=C, embed_dim=D, depth=depth, num_heads=heads,
                       decoder_embed_dim=Dd, decoder_depth=ddepth, decoder_num_heads=dheads,
                       norm_pix_loss=bool(norm_pix), loss_fn=str(z["loss_fn"]), pixel_mean=float(z["pixel_mean"]),
                       pixel_std=float(z["pixel_std"]), ra_dec="ra_dec" in z.files)
    state = OrderedDict()
    for name_, _shape in mo.state_layout(cfg):
        state[name_] = torch.from_numpy(z["state/" + name_].copy())
    return z, cfg, state


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def load_simmim_case(name):
    """SimMIM-mode goldens (tests/golden/make_golden.py simmim_case): -> (npz, cfg, state, imgs, pixel_mask, ra_dec|None)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    img, patch, C, D, depth, heads, norm_pix, rd = [int(v) for v in z["cfg"][:8]]
    pool = len(z["cfg"]) > 8 and bool(z["cfg"][8])                  # attention pooling (case J)
    cfg = mo.config_for("simmim", img_size=img, patch_size=patch, in_chans=C, embed_dim=D, depth=depth, num_heads=heads,
                        norm_pix_loss=bool(norm_pix), loss_fn=str(z["loss_fn"]), pixel_mean=float(z["pixel_mean"]),
                        pixel_std=float(z["pixel_std"]), ra_dec=bool(rd), attn_pool=pool)
    state = OrderedDict()
    for name_, _shape in mo.state_layout(cfg):
        state[name_] = torch.from_numpy(z["state/" + name_].copy())
    ra_dec = torch.from_numpy(z["ra_dec"].copy()) if rd else None
    return z, cfg, state, torch.from_numpy(z["imgs"].copy()), torch.from_numpy(z["pixel_mask"].copy()), ra_dec


# ---- guarded device buffers of the per-element GEMM tests (test_gemm_elementwise_gpu.py, test_gemm_group_elementwise_gpu.py)
DEV = "cuda"
SENT = 12.5
NAN = float("nan")


def guarded_in(x, dtype, ld):
    """2-D x as a view into a NaN buffer [rows + 2, ld]: a NaN row before and after, NaN columns beyond x's."""
    R, C = x.shape
    buf = torch.full((R + 2, ld), NAN, device=DEV, dtype=dtype)
    v = buf[1:R + 1, :C]
    v.copy_(x.to(DEV, dtype))
    return v


def guarded_vec(x, dtype, fill, pad):
    buf = torch.full((x.numel() + 2 * pad,), fill, device=DEV, dtype=dtype)
    v = buf[pad:pad + x.numel()]
    v.copy_(x.to(DEV, dtype))
    return v


class Out:
    """An output view [R, C] (NaN) inside a sentinel buffer [R + 2, ld]."""

    def __init__(self, R, C, dtype, ld):
        self.buf = torch.full((R + 2, ld), SENT, device=DEV, dtype=dtype)
        self.view = self.buf[1:R + 1, :C]
        self.view.fill_(NAN)

    def outside_intact(self):
        b = self.buf.clone()
        b[1:-1, :self.view.shape[1]] = SENT
        return bool((b == SENT).all())

    def bits(self):
        return self.view.contiguous().view(torch.int32 if self.view.dtype == torch.float32 else torch.int16)


def gemm_device_inputs(c, t):
    """The operands gemm_reference.inputs(c) made, on the device behind guards: {"A", "B", "kw": the epilogue's arguments of
    ops.gemm / ops.gemm_args}.  A and B are views with ld beyond the contiguous extent into NaN buffers; the same for resid, aux,
    table and bias; tab_row and dst_row have guard entries around them that name a valid but wrong row whose row is NaN."""
    from tests import gemm_reference as gr
    ld = gr.lds(c)
    Mo = gr.out_rows(c)
    d = {"A": guarded_in(t["A"] if c.al == gr.KC else t["A"].T, c.dtype, ld["lda"]),
         "B": guarded_in(t["B"] if c.bl == gr.KC else t["B"].T, c.dtype, ld["ldb"])}
    kw = {}
    if "bias" in t:
        kw["bias"] = guarded_vec(t["bias"], torch.float32, NAN, 4)
    if "table" in t:
        table = torch.cat([t["table"], torch.full((1, c.N), NAN)])           # the last row: NaN, named by tab_row's guard entries
        kw.update(table=guarded_in(table, torch.float32, ld["ldt"]), ldt=ld["ldt"],
                  tab_row=guarded_vec(t["tab_row"], torch.int32, gr.TABLE_ROWS, 1))
    resid = t.get("resid")
    if "dst_row" in t:
        unmapped = sorted(set(range(Mo)) - set(t["dst_row"].tolist()))
        kw["dst_row"] = guarded_vec(t["dst_row"], torch.int32, unmapped[0], 1)   # guard entries: an unmapped row (its residual row is NaN)
        resid = resid.clone()
        resid[unmapped] = NAN                                                # (a row of dst_row = -1 may request row 0 and drops it)
    if resid is not None:
        kw.update(resid=guarded_in(resid, torch.float32, ld["ldr"]), ldr=ld["ldr"])
    if "aux" in t:
        kw.update(aux=guarded_in(t["aux"], c.dtype, ld["ldaux"]), ldaux=ld["ldaux"])
    d["kw"] = kw
    return d


def record_parity(name, values):
    """Achieved errors of a parity test, merged into gpurun_out/parity_errors.json (scratch; `tests/parity_report.py` copies
    the file into profiles/ after a GPU run) and printed: the bars in the tests are set at 2x these figures."""
    import json
    import os
    root = os.environ.get("GRAFT_REPO_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "gpurun_out", "parity_errors.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = values
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass
    print(f"[parity] {name}: {values}")
