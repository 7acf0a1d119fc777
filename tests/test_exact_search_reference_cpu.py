"""CPU pins of tests/exact_search_reference.py: the case tables reach every route and hold the edge values by value, the restated
list counts and the sample-floor predicate equal the library's own host functions for every case, check_lists accepts lists
built from the statement and rejects each of six planted defects."""
import numpy as np
import pytest

from oracle import similarity_oracle as so
from tests import exact_search_reference as er
from tests.exact_search_reference import INF


@pytest.fixture(scope="module")
def ops():
    from sky_embeddings_amd import ops as _ops
    _ops.lib()
    return _ops


# ------------------------------------------------------------------------------------------------------------- tables
def test_every_route_name_has_a_case():
    topk = {c.route for c in er.STREAM_CASES + er.TILED_CASES + er.NW4_CASES + er.STREAM_OFF_CASES}
    assert topk == set(er.TOPK_ROUTES)
    assert {c.route for c in er.NW4_CASES} == {"tile64x128"} and len(er.NW4_CASES) >= 6
    assert {c.route for c in er.STREAM_OFF_CASES} == {"tile16"}
    assert {c.route for c in er.SCORE_CASES} == set(er.SCORE_ROUTES)
    assert {c.route for c in er.SCORE_STREAM_OFF_CASES} == {"scores16"}
    assert {c.route for c in er.NORM_CASES} == set(er.NORM_ROUTES)
    assert {er.kth_route(S) for S, _ in er.KTH_CASES} == set(er.KTH_ROUTES)
    for c in er.STREAM_CASES:
        assert c.route in ("stream8", "stream4") and c.route == "stream%d" % er.stream_waves(c.D, c.k)
    for c in er.TILED_CASES:
        assert c.route in ("tile16", "tile64x256") and c.route == ("tile16" if er.small_tile(c.Q, c.k) else "tile64x256")


def test_the_wave_switch_sits_where_the_lds_formula_puts_it():
    assert [er.stream_waves(768, k) for k in (112, 113, 128)] == [8, 4, 4]
    assert [er.stream_waves(1024, k) for k in (96, 97)] == [8, 4]
    assert er.stream_waves(64, 128) == 8
    assert 64 * 768 + 1024 * 112 == er.LDS_CAP


def test_streaming_table_holds_its_edge_values():
    S = er.STREAM_CASES
    assert {c.Q for c in S} == {1, 3, 5, 15, 16} and {c.D for c in S} == {64, 192, 768, 1024}
    for w, name in ((8, "stream8"), (4, "stream4")):
        N = {c.N for c in S if c.route == name}
        assert {1, 15, 17, 63, 64 * w - 1, 64 * w + 1, 2 * 64 * w, 2100} <= N, (name, sorted(N))
    assert {c.k for c in S if c.D == 768} >= {1, 2, 112, 113, 128}
    assert {c.k for c in S if c.D == 1024} == {96, 97}
    assert {(c.route, c.k) for c in S if c.D == 1024} == {("stream8", 96), ("stream4", 97)}
    for name in ("stream8", "stream4"):
        assert any(c.N < c.k for c in S if c.route == name)
        assert any(c.N < 16 for c in S if c.route == name)
        assert any(c.N < 64 * int(name[-1]) for c in S if c.route == name)            # wavefronts without a single row
    # a wavefront whose slice ends inside a 16-row step
    assert any(hi > lo and (hi - lo) % 16 for c in S for lo, hi in er.list_ranges(c.route, c.N, er.case_nlists(c)))


def test_tiled_table_holds_its_edge_values():
    T = er.TILED_CASES
    assert {c.Q for c in T} >= {1, 16, 17, 63, 64, 65, 129} and {c.N for c in T} >= {1, 255, 256, 257, 2049}
    assert {c.D for c in T} == {4, 12, 36, 100, 1028} and {c.k for c in T} >= {1, 128, 129, 300}
    assert any(c.k > c.N for c in T)
    assert {c.nchunks for c in T if c.N == 300} == {1, 3, 5, 6}
    for c in T:
        assert not er.stream_applicable(c.Q, c.D, c.k)
    # both many-query cases on either side of k = 128, and D = 1028 for Q <= 16 (the first D past the streaming kernel)
    assert {c.route for c in T if c.Q > 16 and c.k == 128} == {"tile64x256"} and {c.route for c in T if c.Q > 16 and c.k == 129} == {"tile16"}
    assert any(c.Q <= 16 and c.D == 1028 for c in T) and er.stream_applicable(16, 1024, 96) and not er.stream_applicable(16, 1028, 96)
    # N = 300 in 3 chunks of the 256-row tile: a ragged second chunk and an empty third; one count leaves >= 2 chunks empty
    assert er.list_ranges("tile16", 300, 3) == [(0, 256), (256, 300), (512, 300)]
    assert max(sum(hi <= lo for lo, hi in er.list_ranges(c.route, c.N, c.nchunks)) for c in T if c.nchunks) >= 2


def test_every_route_sees_weights_offsets_and_all_four_floor_forms():
    for cases in (er.STREAM_CASES, er.TILED_CASES, er.NW4_CASES, er.STREAM_OFF_CASES):
        for name in {c.route for c in cases}:
            mine = [c for c in cases if c.route == name]
            assert {c.weighted for c in mine} == {True, False}, name
            assert {c.idx_offset for c in mine} == {0, 2 ** 31 + 5, 2 ** 40}, name
            assert any(c.N >= 9 and c.Q >= 3 for c in mine), name                    # duplicates, NaN / inf / zero rows, zero query
            forms = set()
            for n, c in enumerate(cases):
                if c.route == name and c.N >= 9:
                    forms |= {er.FLOOR_FORMS[(q + n) % 4] for q in range(c.Q)}
            assert forms == set(er.FLOOR_FORMS), name


def test_other_tables_hold_their_edge_values():
    assert {c.N for c in er.SCORE_CASES} == {1, 15, 16, 17, 1000, 4097} and {c.Q for c in er.SCORE_CASES} == {1, 5, 16, 17, 65}
    for name in er.SCORE_ROUTES:
        assert {c.N for c in er.SCORE_CASES if c.route == name} == {1, 15, 16, 17, 1000, 4097}
    assert er.FLOOR_S == (16, 40, 2050, 32768, 32761) and {kk for _, _, kk in er.FLOOR_CASES} == {"one", "tiles"}
    assert er.floor_k(32761, "tiles") == 2048 == er.FLOOR_TILE_LIMIT and er.floor_k(40, "tiles") == 3
    assert (4, 32769, 64, 1) in er.FLOOR_REFUSALS and (4, 40, 64, 4) in er.FLOOR_REFUSALS
    assert {(c.N, c.D) for c in er.NORM_CASES} >= {(1, 64), (16, 956), (16, 960), (17, 100)}
    assert er.norms_route(16, 956, 1, 1) == "rows<1,1>" and er.norms_route(16, 960, 1, 1) == "flat"
    assert 17 * 960 * 4 <= 65536 < 17 * 964 * 4
    assert er.norms_route(16, 100, 1, 0) == "rows<1,0>" and er.norms_route(17, 100, 1, 0) == "flat" == er.norms_route(16, 100, 1, 0, aligned=False)
    assert any(not c.aligned for c in er.NORM_CASES)
    assert er.KTH_S == (1, 2048, 2049, 32768, 32769)
    assert [er.kth_route(S) for S in er.KTH_S] == ["wave", "wave", "bisect", "bisect", "radix"]
    assert er.KTH_RUN > 1024
    for S in er.KTH_S[1:]:
        x = er.kth_data(S)
        k = er.kth_k(x, "in_run")
        srt = -np.sort(-x[1])
        assert srt[k - 1] == np.float32(0.25) and (x[1] == np.float32(0.25)).sum() == er.KTH_RUN and 1 < k < S
        assert np.isnan(x[3]).all() and len(np.unique(x[2])) == 1 and np.isinf(x[6]).any()
        assert np.signbit(x[4]).any() and not np.signbit(x[4]).all() and (x[4] == 0).all()
        assert (np.abs(x[5]) < np.finfo(np.float32).tiny).all() and (x[5] != 0).all()


def test_lds_cap_of_the_16_query_tile():
    k = er.largest_k("tile16")
    assert er.tile_lds_bytes("tile16", k) <= er.LDS_CAP < er.tile_lds_bytes("tile16", k + 1) and k == 811
    assert er.tile_lds_bytes("tile64x256", 128) <= er.LDS_CAP and er.tile_lds_bytes("tile64x128", 128) <= er.LDS_CAP


# ------------------------------------------------------------------------------------------------------------- library
def test_restated_counts_equal_the_librarys(ops):
    for c in er.STREAM_CASES + er.TILED_CASES:
        name, n = er.route(c.Q, c.N, c.D, c.k)
        assert name == c.route and n == ops.cosine_topk_chunks(c.N, c.Q, c.D, c.k), c
    for N in (1, 63, 64, 511, 512, 513, 2100, 100000, 1 << 20, (1 << 31) - 1):           # the count's own steps
        for Q, D, k in ((1, 64, 1), (16, 768, 112), (16, 768, 113), (16, 1024, 97), (16, 1028, 97), (17, 768, 10), (300, 64, 128),
                        (300, 64, 129)):
            assert er.route(Q, N, D, k)[1] == ops.cosine_topk_chunks(N, Q, D, k), (Q, N, D, k)


def test_restated_sample_floor_predicate_equals_the_librarys(ops):
    for Q, S, kk in er.FLOOR_CASES:
        k = er.floor_k(S, kk)
        assert er.sample_floor_applicable(Q, S, er.FLOOR_D, k) and ops.sample_floor_applicable(Q, S, er.FLOOR_D, k), (Q, S, k)
    for Q, S, D, k in er.FLOOR_REFUSALS:
        assert not er.sample_floor_applicable(Q, S, D, k) and not ops.sample_floor_applicable(Q, S, D, k), (Q, S, D, k)
    for Q in (1, 16, 17):
        for S in (1, 16, 17, 32768, 32769):
            for D in (64, 96, 1024, 1088):
                for k in (1, 2, 2048, 2049):
                    assert er.sample_floor_applicable(Q, S, D, k) == ops.sample_floor_applicable(Q, S, D, k), (Q, S, D, k)


# ------------------------------------------------------------------------------------------------------------- the checker
Q_, N_, D_, K_ = 5, 300, 64, 20
OFF_ = 2 ** 31 + 5
RANGES_ = er.list_ranges("stream8", N_, 8)                                  # 48 rows per list: list 6 holds 12, list 7 none


@pytest.fixture(scope="module")
def planted():
    q, x, w = er.search_data(Q_, N_, D_, True, 7)
    ref = so.cosine_scores_np(q, x, w, er.EPS)
    thr, forms = er.make_floors(ref, K_, 0)
    assert set(forms) == set(er.FLOOR_FORMS)
    return q, x, w, ref, thr


def lists(planted, thr0=None):
    ref = planted[3]
    ps, pi = er.statement_lists(ref, K_, thr0, OFF_, RANGES_)
    return ps.copy(), pi.copy(), ref


def test_oracle_defines_the_planted_rows(planted):
    q, x, w, ref, _ = planted
    assert np.array_equal(er.bits(ref[:, 0]), er.bits(ref[:, 2])) and np.array_equal(er.bits(ref[:, 0]), er.bits(ref[:, N_ - 1]))
    assert (ref[:, 5] == -INF).all() and (ref[:, 6] == -INF).all() and (ref[:, 7] == 0).all()
    finite = np.ones(N_, bool)
    finite[[5, 6]] = False
    assert (ref[2, finite] == 0).all() and not np.signbit(ref[2, finite]).any()
    assert not np.isnan(ref).any()
    rs, ri = so.cosine_topk_np(q, x, K_, w, er.EPS)
    es, ei = er.search_reference(ref, K_)
    assert np.array_equal(ri, ei) and np.array_equal(er.bits(rs), er.bits(es))


def test_check_lists_accepts_the_statement(planted):
    q, x, w, ref, thr = planted
    for thr0 in (None, thr):
        ps, pi, _ = lists(planted, thr0)
        er.check_lists(ps, pi, ref, N_, K_, thr0, OFF_)
        er.check_ranges(ps, pi, ref, K_, thr0, OFF_, RANGES_)
        rs, ri = so.cosine_topk_np(q, x, K_, w, er.EPS)
        ms, mi = er.merge_reference(ps, pi, K_)
        es, ei = er.restrict_by_floor(rs, ri, thr0, OFF_)
        assert np.array_equal(mi, ei) and np.array_equal(er.bits(ms), er.bits(es))
    # the floor forms do what they say: equal to a score removes that row, above-all leaves lone terminators
    ps, pi, _ = lists(planted, thr)
    assert (pi[3, :, 0] < 0).all() and (ps[3, :, 0] == -INF).all()                       # query 3: above_all
    assert (ps[2][pi[2] >= 0] > thr[2]).all() and thr[2] == 0                            # query 2 (zero): the floor is the tie itself
    assert (pi[2, :, 0] < 0).all()
    # any other cut of the bank is as good to check_lists, and a k above the bank's rows
    for nl, name in ((1, "tile16"), (3, "tile16"), (5, "tile16"), (32, "stream4")):
        rg = er.list_ranges(name, N_, nl)
        for k in (1, K_, 400):
            a, b = er.statement_lists(ref, k, thr, 0, rg)
            er.check_lists(a, b, ref, N_, k, thr, 0)


def test_check_lists_rejects_a_swapped_tie(planted):
    ps, pi, ref = lists(planted)
    assert ps[2, 0, 0] == ps[2, 0, 1] == 0                                               # the zero query: rows 0, 1, 2, ... tie
    pi[2, 0, [0, 1]] = pi[2, 0, [1, 0]]
    with pytest.raises(AssertionError, match="not ordered"):
        er.check_lists(ps, pi, ref, N_, K_, None, OFF_)


def test_check_lists_rejects_a_row_at_the_floor(planted):
    ps, pi, ref = lists(planted)
    thr = np.full(Q_, -INF, np.float32)
    thr[1] = ps[1, 3, 4]                                                                 # a kept row's own score
    with pytest.raises(AssertionError, match="at or below the floor"):
        er.check_lists(ps, pi, ref, N_, K_, thr, OFF_)
    ps, pi, _ = lists(planted, thr)
    er.check_lists(ps, pi, ref, N_, K_, thr, OFF_)


def test_check_lists_rejects_a_duplicate_across_lists(planted):
    ps, pi, ref = lists(planted)
    ps[2, 0, K_ - 1], pi[2, 0, K_ - 1] = ps[2, 1, 0], pi[2, 1, 0]                         # ordered, right bits, above the floor
    with pytest.raises(AssertionError, match="duplicate row across lists"):
        er.check_lists(ps, pi, ref, N_, K_, None, OFF_)


def test_check_lists_rejects_a_missing_terminator(planted):
    ps, pi, ref = lists(planted)
    n = er.valid_len(pi[0, 6])
    assert n == 12 < K_ and er.valid_len(pi[0, 7]) == 0                                   # 12 rows, and an empty range
    ps[0, 6, n:], pi[0, 6, n:] = np.float32(np.nan), -7777                               # the pre-fill, never overwritten
    with pytest.raises(AssertionError, match="missing terminator"):
        er.check_lists(ps, pi, ref, N_, K_, None, OFF_)
    with pytest.raises(AssertionError, match="no terminator"):
        er.check_ranges(ps, pi, ref, K_, None, OFF_, RANGES_)
    ps, pi, _ = lists(planted)
    ps[0, 6, n], pi[0, 6, n] = ps[0, 5, 0], pi[0, 5, 0] + 1000                            # a list that simply runs on
    with pytest.raises(AssertionError):
        er.check_lists(ps, pi, ref, N_, K_, None, OFF_)


def test_check_lists_rejects_a_wrong_score_bit(planted):
    ps, pi, ref = lists(planted)
    ps.view(np.int32)[4, 2, 3] ^= 1
    with pytest.raises(AssertionError, match="wrong score bits"):
        er.check_lists(ps, pi, ref, N_, K_, None, OFF_)


def test_check_lists_rejects_an_index_outside_the_bank(planted):
    for bad in (OFF_ + N_, OFF_ - 1 + 2 ** 32, 3):
        ps, pi, ref = lists(planted)
        pi[1, 5, K_ - 1] = bad
        with pytest.raises(AssertionError, match="index outside the bank"):
            er.check_lists(ps, pi, ref, N_, K_, None, OFF_)


def test_check_lists_rejects_a_missing_row_and_untouched_output(planted):
    ps, pi, ref = lists(planted)
    ps[0, 0, 0:K_ - 1], pi[0, 0, 0:K_ - 1] = ps[0, 0, 1:K_].copy(), pi[0, 0, 1:K_].copy()  # the list's best row dropped
    ps[0, 0, K_ - 1], pi[0, 0, K_ - 1] = -INF, -1
    with pytest.raises(AssertionError, match="merged lists differ"):
        er.check_lists(ps, pi, ref, N_, K_, None, OFF_)
    ps, pi = np.full_like(ps, np.nan), np.full_like(pi, -7777)
    with pytest.raises(AssertionError):
        er.check_lists(ps, pi, ref, N_, K_, None, OFF_)


# ------------------------------------------------------------------------------------------------------------- other statements
def test_norm_statement_is_the_oracles_own_arithmetic():
    x, w = er.norm_data(16, 100)
    for ww in (w, None):
        norms, xw = er.norms_reference(x, ww)
        wv = w if ww is not None else np.ones(100, np.float32)
        assert np.array_equal(er.bits(xw), er.bits(wv[None, :] * x))
        acc = np.float64(0)
        for d in range(100):                                                             # fp64 stand-in: the fp32 chain is close
            acc += np.float64(xw[3, d]) * np.float64(x[3, d])
        assert abs(float(norms[3]) - np.sqrt(acc)) <= 1e-5 * np.sqrt(acc)
    # as a bank norm it is what the scores divide by: score(x, x) == 1 up to rounding
    s = so.cosine_scores_np(x[:1], x[:1], w, er.EPS)
    assert abs(float(s[0, 0]) - 1.0) < 1e-5


def test_sample_floor_and_kth_statements():
    g = np.random.default_rng(3)
    sc = g.standard_normal((2, 40), dtype=np.float32)
    fl, tmax = er.sample_floor_reference(sc, 2)
    assert tmax.shape == (2, 3) and tmax[0, 2] == sc[0, 32:40].max()
    assert fl[0] == np.nextafter(np.sort(tmax[0])[-2], -INF) and fl.dtype == np.float32
    x = np.array([[1.0, np.nan, -0.0, 0.0, -INF, 2.0]], np.float32)
    assert er.kth_reference(x, 1)[0] == np.nextafter(np.float32(2), -INF)
    tiny = np.nextafter(np.float32(0), -INF)
    assert er.kth_reference(x, 3)[0] == tiny and er.kth_reference(x, 4)[0] == tiny and tiny < 0
    assert er.kth_reference(x, 5)[0] == -INF and er.kth_reference(x, 6)[0] == -INF
