"""The cases of the two-stage search's launch golden (tests/golden/prefilter_launches.json): one call of an entry point of
csrc/topk_prefilter.hip each, at the smallest shapes the routes take (D = 128, Q = 17, one Q = 257 for two query tiles), chosen so
that every branch of the host layer's schedule is walked.  tools/prefilter_launch_record.py makes the calls under a kernel trace,
tests/golden/make_prefilter_launch_golden.py turns the trace into the golden, and tests/test_prefilter_plan_cpu.py rebuilds every
case's launch list from ops.prefilter_plan.  A case is data-independent: the launches depend on the shape alone.

Fields: kind 'rows' | 'tokens' | 'mean'; bank 'f32' (rows only: fp32 bank + fp16 image) | 'f16' | 'bf16'; N rows (images on the
token routes); thr0: a floor is handed in; dead: None, or the bank tiles (of 256 stage-1 rows) a selection leaves without a
selected row -- every other row (image) is selected; direct_sel: the position at which a selected token search's first slice ends
(the caller's to choose: 1 .. n_live); lo: None (SKYEMB_PREFILTER_LO unset), '0' or '1'."""
BT = 256


def case(id, kind, bank, N, k=5, P=1, combine="min", top_t=0, thr0=False, dead=None, direct_sel=0, lo=None, Q=17, D=128):
    return dict(id=id, kind=kind, bank=bank, N=N, k=k, P=P, combine=combine, top_t=top_t, thr0=thr0, dead=dead, direct_sel=direct_sel,
                lo=lo, Q=Q, D=D)


BIG = 320 * BT                  # T = 320 whole tiles: the six slice ends are distinct

CASES = [
    # ---- row search
    case("rows-f32-T=first", "rows", "f32", 2048),                           # the empty direct launch and the second final select
    case("rows-f16-T=first-tail", "rows", "f16", 2048 + 44),
    case("rows-bf16-T=first+1", "rows", "bf16", 2304),
    case("rows-f32-ragged", "rows", "f32", 2304 + 100),
    case("rows-f16-k129", "rows", "f16", 8192, k=129),                       # cap 8192, first 16
    case("rows-f16-big-tail", "rows", "f16", BIG + 7),
    case("rows-bf16-big-thr0", "rows", "bf16", BIG, thr0=True),
    case("rows-f32-big-thr0-lo1", "rows", "f32", BIG, thr0=True, lo="1"),
    case("rows-f16-thr0-tail", "rows", "f16", 2560 + 3, thr0=True),
    case("rows-f16-Q257", "rows", "f16", 4096, Q=257),
    case("rows-f16-Q257-lo1", "rows", "f16", 4096, Q=257, lo="1"),
    case("rows-f32-lo0", "rows", "f32", 4096, lo="0"),
    case("rows-bf16-lo1", "rows", "bf16", 4096 + 1, lo="1"),
    case("rows-bf16-lo0", "rows", "bf16", 4096, lo="0"),
    case("rows-f16-sel-tail-live", "rows", "f16", 2560 + 37, dead=(3,)),
    case("rows-bf16-sel-tail-dead", "rows", "bf16", 2560 + 37, dead=(10,)),
    case("rows-f32-sel", "rows", "f32", 2560 + 37, dead=(0, 9)),
    case("rows-f16-sel-T=first", "rows", "f16", 2560, dead=(1, 2), lo="1"),
    # ---- token search, min / max
    case("tok-P1-min-f16", "tokens", "f16", 4096, P=1),
    case("tok-P4-max-bf16-tail", "tokens", "bf16", 1024 + 3, P=4, combine="max"),
    case("tok-P64-min-f16", "tokens", "f16", 64, P=64),
    case("tok-P4-min-bf16-lo1-thr0", "tokens", "bf16", 1024, P=4, lo="1", thr0=True),
    case("tok-P4-min-top1", "tokens", "f16", 1024, P=4, top_t=1),
    case("tok-P4-min-top2-tail", "tokens", "f16", 1024 + 3, P=4, top_t=2),
    case("tok-P4-min-top2-bf16-lo1", "tokens", "bf16", 1024, P=4, top_t=2, lo="1"),
    case("tok-P4-min-topP", "tokens", "f16", 1024, P=4, top_t=4),
    case("tok-P4-max-top2", "tokens", "bf16", 1024, P=4, combine="max", top_t=2),
    case("tok-P4-min-big-tail-thr0", "tokens", "f16", BIG // 4 + 1, P=4, thr0=True),
    case("tok-P4-min-Q257", "tokens", "f16", 1024, P=4, Q=257),
    case("tok-P4-sel-direct1", "tokens", "f16", 1024 + 3, P=4, dead=(2,), direct_sel=1),
    case("tok-P4-sel-interior", "tokens", "bf16", 1024 + 3, P=4, combine="max", dead=(2,), direct_sel=5),
    case("tok-P4-sel-direct=n_live", "tokens", "f16", 1024 + 3, P=4, dead=(2,), direct_sel=16),
    case("tok-P4-sel-top2-tail-dead", "tokens", "bf16", 1024 + 3, P=4, top_t=2, dead=(16,), direct_sel=3),
    case("tok-P4-sel-top1-lo1", "tokens", "f16", 1024, P=4, top_t=1, dead=(0, 5), direct_sel=2, lo="1"),
    # ---- token search, mean (stage 1 walks the pooled image: N rows)
    case("mean-P4-f16", "mean", "f16", 2048, P=4, combine="mean"),
    case("mean-P4-bf16-tail-lo0", "mean", "bf16", 2048 + 9, P=4, combine="mean", lo="0"),
    case("mean-P1-f16-lo1-thr0", "mean", "f16", 4096 + 5, P=1, combine="mean", lo="1", thr0=True),
    case("mean-P64-bf16", "mean", "bf16", 2560, P=64, combine="mean"),
]


def stage1_rows(c):
    """Rows stage 1 walks: token rows, or images under mean."""
    return c["N"] * c["P"] if c["kind"] == "tokens" else c["N"]


def selection_info(c):
    """(n_live, last_live) of the case's selection, as skyemb_prefilter_select_prepare / skyemb_token_prefilter_select_prepare
    report them: every tile but the dead ones holds a selected row."""
    tiles_all = -(-stage1_rows(c) // BT)
    assert all(0 <= t < tiles_all for t in c["dead"])
    return tiles_all - len(c["dead"]), int(tiles_all - 1 not in c["dead"])


def selection_flags(c):
    """The selection as one flag per row (rows) or image (tokens), numpy bool."""
    import numpy as np
    per_tile = BT // c["P"] if c["kind"] == "tokens" else BT
    flags = np.ones(c["N"], dtype=bool)
    for t in c["dead"]:
        flags[t * per_tile:(t + 1) * per_tile] = False
    return flags
