"""One grouped GEMM launch (skyemb_gemm_group_plan / _launch, include/skyemb.h) on top of tests/gemm_reference.py: the fp64 statement,
the bar, the operands and the CPU emulation of ONE problem are that module's (`Case`, `inputs`, `reference`, `bars`, `ratio`, `lds`,
`has`, `emulate`); this one adds what a group adds.  Pinned on the CPU by tests/test_gemm_group_reference_cpu.py, run on the GPU by
tests/test_gemm_group_elementwise_gpu.py.

A grouped case is GroupCase(name, dtype, tile, order, problems, hint): `problems` are gemm_reference.Case with split = 0 and
tile = the group's tile code; `order` is what SKYEMB_GROUP_XCD_ORDER holds while the plan is built (None: unset); `hint` the byte
count of a prefetch hint on the first problem (0: none).

Added here:
- epilogue "colsum16": a row-contiguous A, a 16-bit `out` and `colsum_a`, no out_f32 -- the gradient mirror engine._make_wgrad_group
  plans when g16 is set.  Its statement is the "colsum" statement; its bar the stored-rounding bar of gemm_reference.bars with the
  16-bit h (`reference` renames out_f32 to out, gemm_reference.bars then takes h from the case's dtype).
- contrast between problems: problem j's operands come from a seed of their own and A carries an extra power of two SCALE[dtype][j %
  len] (exact in the format), so a tile computed from a neighbour's pointers, K or leading dimensions is orders of magnitude off.
  The scales are >= 1: in the epilogues that add bias, table and residual (unit size) the product must stay the larger term.  The
  problems of a case have pairwise different (M, N, K).
- the header (`header`, `slot_to_tile`, `lookup`, `walk`, `chosen_tile`): starts[i] = prefix sum of ceil(M / stride_m) ceil(N / BN)
  rounded up to 8, total, class mask, the tile the plan chooses at tile = 0, and the map from workgroup b to a slot of the
  concatenated tile list: gt = (b & 7) (total >> 3) + (b >> 3) when the order is on, b when it is off.
- `run_group`: the launch on the CPU, workgroup by workgroup, each real tile copied from gemm_reference.emulate of its problem into
  a memory image [rows + BM, ld] of every output (NaN = never written), with the subtly wrong launches of GROUP_MUTANTS.

Which tile took which class (GROUP_CASES): the cross product is small enough to run whole --
  mask 4 (RC.RC)        every grouped tile x {bf16, fp16} x both tile orders (ring tiles: unset and 1; 256 x 256: unset and 0)
  mask 1 (KC.KC)        64064, 128064, 128128, 9128128 x {bf16 (order unset), fp16 (order 1)}
  mask 2 (KC.RC)        the same
  mask 6 (KC.RC+RC.RC)  64064, 128064, 128128 (the tiles built with MIXED) x the same; on 9128128 the plan refuses it
  32 problems           64064, bf16 (order 1) and fp16 (order unset)
  prefetch hint         128064, bf16, 4004 bytes on the first problem
K per problem: 64 / 128 / 192 / 320 on the one-k-group ring tiles; 9128128 needs K % 128 == 0 and K <= 384 leaves 128 / 256 / 384,
so its four-problem groups repeat 128 once (at different M, N); 256 x 256 takes whole tiles with K >= 128 only: 128 / 192 / 320 / 256.
"""
from collections import namedtuple

import torch

from tests import gemm_reference as gr
from tests.gemm_reference import BF, F16, KC, RC, T256, TILES, Case, round_to

GROUPED_TILES = (64064, 128064, 128128, 9128128, T256)      # gemm_pipe.hip SKY_GEMM_PRODUCT_TILES rows with GROUPED
RING_TILES = GROUPED_TILES[:4]
MIXED_TILES = (64064, 128064, 128128)                       # ... with MIXED
MASKS = {64064: (1, 2, 4, 6), 128064: (1, 2, 4, 6), 128128: (1, 2, 4, 6), 9128128: (1, 2, 4), T256: (4,)}
GROUP_MAX = 32
XCD_BIT = 1 << 30
HEADER_BYTES = 256
SCALE = {BF: (0, 5, 2, 7, 3, 6), F16: (0, 3, 1, 4, 2)}
HINT_BYTES = 4004                                           # a multiple of 4 (skyemb.h), not of 16

GroupCase = namedtuple("GroupCase", "name dtype tile order problems hint", defaults=(0,))


def gid(gc):
    return f"{gr.DT[gc.dtype]}-t{gc.tile}-{gc.name}-order{'unset' if gc.order is None else gc.order}"


def _cdiv(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------------------------------------- one problem
def base(c):
    """The gemm_reference case that states problem c: colsum16 is "colsum" stored in 16 bits."""
    return c._replace(epi="colsum") if c.epi == "colsum16" else c


def has(c, what):
    if c.epi == "colsum16":
        return what in ("out", "colsum")
    return gr.has(c, what)


def lds(c):
    return gr.lds(base(c))


def out_rows(c):
    return gr.out_rows(base(c))


def inputs(gc, j):
    c = gc.problems[j]
    t = gr.inputs(base(c), seed=1000 * (j + 1) + c.M * 131 + c.N * 17 + c.K)
    s = SCALE[gc.dtype]
    t["A"] = (t["A"] * 2.0 ** s[j % len(s)]).to(c.dtype).float()
    return t


def _rename16(d):
    return {"out": d["out_f32"], "colsum": d["colsum"]}


def reference(c, t):
    st = gr.reference(base(c), t)
    if c.epi == "colsum16":
        st = dict(st, ref=_rename16(st["ref"]), rest=_rename16(st["rest"]))
    return st


def bars(c, st):
    return gr.bars(base(c), st)


def emulate(c, t, trunc16=False):
    e = gr.emulate(base(c), t)
    if c.epi == "colsum16":
        e = _rename16(e)
        e["out"] = round_to(e["out"].float(), c.dtype, "trunc" if trunc16 else "rne").double()
    return e


def single_refused(gc):
    """Problems of gc for which skyemb_gemm(tile = the group's, split_k = 1) runs no single launch of the same tile body (refused,
    the fallback kernel, or two parts): left out of the bit-equality check."""
    out = []
    for j, c in enumerate(gc.problems):
        p = gr.planned(base(c))
        if p["family"] not in ("pipe", "tile256") or p["tile"] != gc.tile or len(p["parts"]) != 1:
            out.append(j)
    return out


# --------------------------------------------------------------------------------------------------------- the header
def class_bit(c):
    return (1 if c.bl == KC else 2) if c.al == KC else (8 if c.bl == KC else 4)


def class_mask(problems):
    m = 0
    for c in problems:
        m |= class_bit(c)
    return m


def ntiles(c, tile):
    _, bn, stride, _ = TILES[tile]
    return _cdiv(c.M, stride) * _cdiv(c.N, bn)


def order_on(tile, order):
    """Header word 1, bit 30 (skyemb_gemm_group_plan): "0..." turns the per-XCD order off, "1..." on for every tile; unset: on
    for the 256 x 256 tile only."""
    if order is not None and order[:1] == "0":
        return False
    return tile == T256 or (order is not None and order[:1] == "1")


def group256_fits(c):
    return gr.gemm256_wgrad_applicable(base(c), 1) and c.epi in ("plain", "colsum", "colsum16")


def chosen_tile(problems):
    """gemm_pipe.hip group_tile with the default switches."""
    t12864 = sum(_cdiv(c.M, 128) * _cdiv(c.N, 64) for c in problems)
    t128 = sum(_cdiv(c.M, 128) * _cdiv(c.N, 128) for c in problems)
    t256 = sum((c.M // 256) * (c.N // 256) for c in problems)
    tile = 128064 if t12864 >= 320 else 64064
    if t128 >= 400:
        tile = 128128
    if all(group256_fits(c) and c.K >= 2048 for c in problems) and 160 <= t256 <= 256:
        tile = T256
    return tile


def header(tile, problems, order):
    starts = [0]
    for c in problems:
        starts.append(starts[-1] + _cdiv(ntiles(c, tile), 8) * 8)
    total = starts[-1]
    on = order_on(tile, order)
    return {"n": len(problems), "starts": starts, "total": total, "word1": total | (XCD_BIT if on else 0), "on": on,
            "mask": class_mask(problems), "f16": problems[0].dtype == F16}


def slot_to_tile(b, total, on):
    return (b & 7) * (total >> 3) + (b >> 3) if on else b


def lookup(gt, starts, n):
    """(problem, tile index inside it) of slot gt, as the kernels find it: the last i < n with starts[i] <= gt."""
    p = 0
    for i in range(1, n):
        if gt >= starts[i]:
            p = i
    return p, gt - starts[p]


def walk(tile, problems, on):
    """[(problem, tile) or None for a padding slot] per workgroup of the launch."""
    h = header(tile, problems, None)
    out = []
    for b in range(h["total"]):
        p, tb = lookup(slot_to_tile(b, h["total"], on), h["starts"], h["n"])
        out.append((p, tb) if tb < ntiles(problems[p], tile) else None)
    return out


# --------------------------------------------------------------------------------------------------------- the launch on the CPU
GROUP_MUTANTS = ("prev_args", "other_k", "drop_last", "pad_writes", "xcd_twice", "trunc16")
LD_OF = {"out_f32": "ldo32", "out": "ldo", "out2": "ldo2"}


def mem_shape(c, tile, name):
    """Memory image of an output: the view [rows, N] at the top left of [rows + BM, ld] (colsum: [M] of [M + BM])."""
    bm = TILES[tile][0]
    if name == "colsum":
        return (c.M + bm,)
    return (out_rows(c) + bm, lds(c)[LD_OF[name]])


def to_mem(c, tile, name, x):
    m = torch.full(mem_shape(c, tile, name), float("nan"), dtype=torch.float64)
    if name == "colsum":
        m[:c.M] = x
    else:
        m[:x.shape[0], :c.N] = x
    return m


def tile_origin(c, tile, wg):
    """gemm_pipe_body: tile index -> (m0, n0); tiles run down the columns first when N > M."""
    _, bn, stride, _ = TILES[tile]
    tiles_m, tiles_n = _cdiv(c.M, stride), _cdiv(c.N, bn)
    colmajor = c.N > c.M
    quo, rem = divmod(wg, tiles_m if colmajor else tiles_n)
    tile_m, tile_n = (rem, quo) if colmajor else (quo, rem)
    return tile_m * stride, tile_n * bn


def _write_tile(mem, c, t, src, tile, tb, clip=True):
    bm, bn = TILES[tile][:2]
    m0, n0 = tile_origin(c, tile, tb)
    if clip:
        rows, cols = torch.arange(m0, min(m0 + bm, c.M)), torch.arange(n0, min(n0 + bn, c.N))
        d = gr.dst_of(base(c), t)[rows]
        d = d[d >= 0]
        for name, x in src.items():
            if name == "colsum":
                if n0 == 0:
                    mem[name][rows] = x[rows]
            else:
                mem[name][d[:, None], cols[None, :]] = x[d[:, None], cols[None, :]]
        return
    # a tile past the problem's last one, stored without the row / column masks: finite values at the flat addresses m ld + n
    rows, cols = torch.arange(m0, m0 + bm), torch.arange(n0, n0 + bn)
    for name, x in src.items():
        if name == "colsum":
            continue
        flat = mem[name].view(-1)
        idx = (rows[:, None] * mem[name].shape[1] + cols[None, :]).reshape(-1)
        val = torch.nan_to_num(x[(rows % x.shape[0])[:, None], (cols % c.N)[None, :]], nan=1.0).reshape(-1)
        keep = idx < flat.numel()
        flat[idx[keep]] = val[keep]


def _hybrid(c, t, c_from, t_from):
    """Problem c computed with ANOTHER problem's operands and K (rows taken modulo the other's counts)."""
    t2 = dict(t)
    t2["A"] = t_from["A"][torch.arange(c.M) % c_from.M]
    t2["B"] = t_from["B"][torch.arange(c.N) % c_from.N]
    return c._replace(K=c_from.K), t2


def run_group(gc, ts, on, mutant=None, full=None):
    """The launch workgroup by workgroup -> [{name: memory image}] per problem.  Mutants (one wrong tile unless said otherwise):
    prev_args   the last tile of problem 1 computed with problem 0's operands and K
    other_k     tile 0 of the problem with the longest K summed over the shortest K of the group only
    drop_last   every problem one tile short (starts off by one)
    pad_writes  the padding workgroup at tb = ntiles stores a tile, unmasked
    xcd_twice   the per-XCD map applied again to the tile index INSIDE its problem (tb, with the problem's own tile count).  Applied
                twice to the launch's slots it is a permutation of them and changes no result (pinned by the CPU test); inside a
                problem whose tile count is no multiple of 8 it is not one: tiles are computed twice and others never.  Order on only.
    trunc16     colsum16's 16-bit store truncates."""
    assert mutant is None or mutant in GROUP_MUTANTS
    P, tile = gc.problems, gc.tile
    if full is None or mutant == "trunc16":
        full = [emulate(c, t, trunc16=mutant == "trunc16") for c, t in zip(P, ts)]
    mem = [{name: to_mem(c, tile, name, torch.full_like(x, float("nan"))) for name, x in f.items()} for c, f in zip(P, full)]
    h = header(tile, P, None)
    wrong = {}
    if mutant == "prev_args" and len(P) > 1:
        wrong[(1, ntiles(P[1], tile) - 1)] = emulate(*_hybrid(P[1], ts[1], P[0], ts[0]))
    if mutant == "other_k":
        ks = [c.K for c in P]
        p, k = ks.index(max(ks)), min(ks)
        if k < P[p].K:
            t2 = dict(ts[p], A=ts[p]["A"][:, :k], B=ts[p]["B"][:, :k])
            wrong[(p, 0)] = emulate(P[p]._replace(K=k), t2)
    for b in range(h["total"]):
        p, tb = lookup(slot_to_tile(b, h["total"], on), h["starts"], h["n"])
        nt = ntiles(P[p], tile)
        if tb >= nt - (1 if mutant == "drop_last" else 0):
            if mutant == "pad_writes" and tb == nt:
                _write_tile(mem[p], P[p], ts[p], full[p], tile, tb, clip=False)
            continue
        if mutant == "xcd_twice" and on:
            tb = (tb & 7) * (nt >> 3) + (tb >> 3)
            if tb >= nt:
                continue
        _write_tile(mem[p], P[p], ts[p], wrong.get((p, tb), full[p]), tile, tb)
    return mem


def worst_ratio(gc, mems, sts):
    """max err / bar over every output of every problem of the launch, the memory around the views included (gemm_reference.ratio:
    inf for a NaN where a value belongs and for a value where nothing may be written)."""
    w = 0.0
    for c, mem, st in zip(gc.problems, mems, sts):
        b = bars(c, st)
        for name, m in mem.items():
            w = max(w, gr.ratio(m, to_mem(c, gc.tile, name, st["ref"][name]), to_mem(c, gc.tile, name, b[name])))
    return w


# --------------------------------------------------------------------------------------------------------- case table
def _k(tile, i):
    if tile == 9128128:
        return (128, 256, 384, 128)[i]
    if tile == T256:
        return (128, 192, 320, 256)[i]
    return (64, 128, 192, 320)[i]


def wgrad_problems(dt, tile):
    """Mask 4: smaller than a tile; ragged on both edges; whole tiles; >= 9 tiles (9 of 16 slots: real padding), ragged again.
    256 x 256 takes whole tiles only."""
    bm, bn = TILES[tile][:2]
    if tile == T256:
        shapes = ((256, 256, "plain"), (512, 256, "colsum"), (256, 512, "colsum16"), (768, 768, "colsum16"))
    else:
        shapes = ((8, 8, "plain"), (bm + 8, bn - 8, "colsum"), (2 * bm, bn, "colsum16"), (3 * bm - 8, 2 * bn + 8, "colsum16"))
    return [Case(dt, tile, RC, RC, m, n, _k(tile, i), epi) for i, (m, n, epi) in enumerate(shapes)]


def kckc_problems(dt, tile):
    bm, bn, stride, _ = TILES[tile]
    return [Case(dt, tile, KC, KC, bm + 1, bn + 8, _k(tile, 1), "gelu"), Case(dt, tile, KC, KC, 2 * stride - 7, bn - 8, _k(tile, 2), "full"),
            Case(dt, tile, KC, KC, 3, 8, _k(tile, 0), "plain")]


def kcrc_problems(dt, tile):
    bm, bn, stride, _ = TILES[tile]
    return [Case(dt, tile, KC, RC, bm + 1, bn + 8, _k(tile, 2), "dgelu"), Case(dt, tile, KC, RC, 2 * stride - 7, 2 * bn - 8, _k(tile, 0), "resid")]


def mixed_problems(dt, tile):
    bm, bn, stride, _ = TILES[tile]
    return [Case(dt, tile, KC, RC, bm + 1, bn + 8, _k(tile, 2), "dgelu"), Case(dt, tile, RC, RC, bm + 8, bn - 8, _k(tile, 1), "colsum"),
            Case(dt, tile, KC, RC, 2 * stride - 7, 2 * bn - 8, _k(tile, 0), "resid"), Case(dt, tile, RC, RC, 2 * bm, bn + 16, _k(tile, 3), "colsum16")]


def many_problems(dt):
    """GROUP_MAX weight gradients of one or two 64 x 64 tiles each: 256 slots, 48 of them real."""
    return [Case(dt, 64064, RC, RC, 8 + 8 * (j % 16), 8 * (1 + (3 * j) % 8), (64, 128, 192)[j % 3], ("plain", "colsum", "colsum16")[j % 3])
            for j in range(GROUP_MAX)]


def _group_cases():
    gs = []
    for dt in (BF, F16):
        for tile in GROUPED_TILES:
            for order in ((None, "0") if tile == T256 else (None, "1")):
                gs.append(GroupCase("wgrad", dt, tile, order, wgrad_problems(dt, tile)))
        order = None if dt == BF else "1"
        for tile in RING_TILES:
            gs.append(GroupCase("kckc", dt, tile, order, kckc_problems(dt, tile)))
            gs.append(GroupCase("kcrc", dt, tile, order, kcrc_problems(dt, tile)))
            if tile in MIXED_TILES:
                gs.append(GroupCase("mixed", dt, tile, order, mixed_problems(dt, tile)))
        gs.append(GroupCase("many", dt, 64064, "1" if dt == BF else None, many_problems(dt)))
    gs.append(GroupCase("hint", BF, 128064, None, wgrad_problems(BF, 128064)[1:3], HINT_BYTES))
    return gs


GROUP_CASES = _group_cases()
