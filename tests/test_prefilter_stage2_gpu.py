"""GPU: stage 2 of the two-stage many-query search CANDIDATE BY CANDIDATE, against the statements of
tests/prefilter_stage2_reference.py: the final select_kernel's choice and `bound`, the re-score's scores, order and index offset,
the certificate `redo`, and the soundness of what was left out -- on the real lists stage 1 left in the workspace (the device's own
cand_d: no model of dot^).  Every case applies all four checkers to EVERY query and asserts the path its planted queries must
take from the read-back arrays.  tests/test_prefilter_stage2_cpu.py shows that the builders put their rows where the cases need
them and that each checker rejects its defect.  The last section reads the token route's final running list.

Everything goes through the C ABI with the guarded buffers of tests/prefilter_gpu_harness.py and idx_offset = 2^33 + 7."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import similarity_oracle as so
from tests import prefilter_stage1_reference as sr
from tests import prefilter_stage2_reference as s2
from tests import token_prefilter_reference as tpr
from tests.prefilter_gpu_harness import TORCH16, Guarded, Search, dev, prepare, ptr, set_lo, stream, ws_arrays
from tests.prefilter_stage2_reference import INF, K, OFFSET, PLANTED_Q, Q

LOS = {False: "hi", True: "hi+lo"}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a device"
    from sky_embeddings_amd import ops as _ops
    _ops.lib()
    return _ops


def check_all(s, c, fmt, lo, k, flags=None, few=False, label=""):
    """The four checkers on every query of the search `s` over the case `c`.  -> (per query dict(path, nsel, margin, live), the
    memberships the band left undecided) with margin = (out_s[k-1] - bound) / hw of the k-th returned row (None when bound = -inf)
    and path = what the read-back arrays say: 'needed' (bound = -inf, redo = 0), 'quota-certified' (finite bound, redo = 0),
    'quota-refused' (finite bound, redo = 1), 'handed-back' (bound = -inf and redo = 1: fewer than k candidates, or the overflow
    flag).  Fails when the band leaves more than 1 % of the (query, candidate) memberships undecided."""
    assert s.guards_ok
    sel = flags is not None
    sc = s2.exact_scores(c["tw"], c["qn"], c["x"], c["xn"])
    den = sr.den32(c["qn"], c["xn"]).astype(np.float64)
    eps_a = sr.eps_a(fmt, s.D, lo)
    lists, info, undecided, members = s.lists(), [], 0, 0
    for q in range(s.Q):
        rows = lists[q].astype(np.int64)
        cd = s.ws["cand_d"][q, :len(rows)]
        assert len(rows) == 0 or (rows.min() >= 0 and rows.max() < len(s.rowp)), q
        live = s2.counting(rows, s.rowp, sel)
        U, L = s2.intervals(cd, rows, s.ws["qbase"][q], s.rowp, c["xn"], sel=sel)
        nsel, bound = int(s.ws["nsel"][q]), float(s.ws["bound"][q])
        r, dc = s2.check_final_select(rows, U, L, k, nsel, s.ws["sel_i"][q], bound, live, ties=s2.tie_classes(cd, rows, s.rowp, c["xn"]))
        assert r is None, (label, q, r)
        undecided, members = undecided + dc, members + int(live.sum())
        chosen = s.ws["sel_i"][q, :nsel].astype(np.int64)
        assert flags is None or flags[chosen].all(), (label, q)
        r = s2.check_rescore(chosen, None, None, None, None, k, OFFSET, s.out_s[q], s.out_i[q], few, scores=sc[q])
        assert r is None, (label, q, r)
        r = s2.check_certificate(s.out_s[q], bound, s.ws["overflow"][q], nsel, k, few, s.redo[q])
        assert r is None, (label, q, r)
        want_s, want_i = s2.topk_of(sc[q], k, flags, few, OFFSET)
        r = s2.check_soundness(rows, live, chosen, sc[q], k, nsel, bound, s.redo[q], s.out_s[q], s.out_i[q], want_s, want_i)
        assert r is None, (label, q, r)
        margin = None
        if bound > -INF and nsel >= k and s.out_i[q, k - 1] >= 0:
            kth = int(s.out_i[q, k - 1] - OFFSET)
            margin = float((float(s.out_s[q, k - 1]) - bound) / s2.hw_of(c["tw"][q:q + 1], c["x"][kth:kth + 1], den[q:q + 1, kth:kth + 1], eps_a)[0, 0])
        path = ("needed" if s.redo[q] == 0 else "handed-back") if bound == -INF else "quota-certified" if s.redo[q] == 0 else "quota-refused"
        info.append(dict(path=path, nsel=nsel, margin=margin, live=int(live.sum())))
    print(label, "undecided memberships", undecided, "of", members)
    assert undecided <= 0.01 * members, (label, undecided, members)
    return info, undecided


def ordinary_ok(s, c, info):
    """Every query that is not planted: certified by construction."""
    for q in range(s.Q):
        if q not in c["planted"]:
            assert s.redo[q] == 0 and s.ws["bound"][q] == -INF and s.ws["overflow"][q] == 0, (q, info[q])


def record(case, fmt, lo, checked, planted):
    """One line of profiles/r21_prefilter_stage2_paths.json (the PATHS lines of this file's output, as printed).  A case
    that plants one or a few queries names each; a case about all of them gives the count per path and the range of nsel."""
    info, undecided = checked
    planted = list(planted)
    m_cert = [i["margin"] for i in info if i["path"] == "quota-certified"]
    m_ref = [i["margin"] for i in info if i["path"] == "quota-refused" and i["margin"] is not None]
    if len(planted) > 4:
        paths = {p: sum(info[q]["path"] == p for q in planted) for p in sorted({info[q]["path"] for q in planted})}
        nsel = {"min": min(info[q]["nsel"] for q in planted), "max": max(info[q]["nsel"] for q in planted)}
    else:
        paths, nsel = {str(q): info[q]["path"] for q in planted}, {str(q): info[q]["nsel"] for q in planted}
    print("PATHS " + json.dumps(dict(case=case, fmt=fmt, lo=LOS[lo], planted=paths, nsel=nsel,
                                     min_certified_margin_hw=round(min(m_cert), 4) if m_cert else None,
                                     max_refused_margin_hw=round(max(m_ref), 4) if m_ref else None, undecided=undecided)))


# ---------------------------------------------------------------------------------------------- needed, quota, ties at the bound
PLANTED = [(name, fmt, lo) for name in s2.WINDOWS for fmt in s2.FMTS for lo in (False, True)]


@pytest.mark.parametrize("name,fmt,lo", PLANTED, ids=[f"{n}-{f}-{LOS[l]}" for n, f, l in PLANTED])
def test_planted_paths(ops, monkeypatch, name, fmt, lo):
    """needed: bound = -inf, k <= nsel <= 256, redo = 0.  quota-certified: bound finite, nsel = 256, out_s[k-1] > bound, redo = 0,
    the oracle's answer.  quota-refused: bound finite and >= out_s[k-1], redo = 1.  ties: bound = the 400 copies' U, the 105 above
    it selected, 151 of the copies and none twice, redo = 0."""
    set_lo(monkeypatch, lo)
    c = s2.planted_case(name, fmt, lo)
    s = Search(ops, fmt, c["tw"], c["qn"], c["x"], c["xn"], K, idx_offset=OFFSET)
    checked = info, _ = check_all(s, c, fmt, lo, K, label=f"{name} {fmt} {LOS[lo]}")
    record(name, fmt, lo, checked, c["planted"])
    ordinary_ok(s, c, info)
    q = PLANTED_Q
    nsel, bound, kth = int(s.ws["nsel"][q]), float(s.ws["bound"][q]), float(s.out_s[q, K - 1])
    print(name, fmt, LOS[lo], "nsel", nsel, "bound", bound, "k-th", kth, "redo", s.redo[q], "margin", info[q]["margin"])
    chosen = set(s.ws["sel_i"][q, :nsel].tolist())
    assert set(c["top"].tolist()) <= chosen and set((s.out_i[q] - OFFSET).tolist()) == set(c["top"].tolist())
    if name == "needed":
        assert bound == -INF and K <= nsel <= 256 and s.redo[q] == 0
        return
    assert np.isfinite(bound) and nsel == 256 and info[q]["live"] > 256
    if name == "quota-refused":
        assert bound >= kth and s.redo[q] == 1
        return
    assert kth > bound and s.redo[q] == 0
    sc = s2.exact_scores(c["tw"][q:q + 1], c["qn"][q:q + 1], c["x"], c["xn"])[0]
    assert s2.same_answer(s.out_s[q], s.out_i[q], *s2.topk_of(sc, K, idx_offset=OFFSET))
    if name == "ties":
        distinct, copies = c["groups"][0][0], c["groups"][1][0]
        rows = s.lists()[q].astype(np.int64)
        U, _ = s2.intervals(s.ws["cand_d"][q, :len(rows)], rows, s.ws["qbase"][q], s.rowp, c["xn"])
        Uc = U[np.isin(rows, copies)]
        assert len(Uc) == 400 and (Uc == Uc[0]).all() and abs(Uc[0] - bound) <= s2.BAND * (abs(bound) + c["hw"])
        assert set(distinct.tolist()) <= chosen and len(chosen & set(copies.tolist())) == 151 and len(chosen) == 256


# ------------------------------------------------------------------------------------------------------------- exact score ties
@pytest.mark.parametrize("fmt", s2.FMTS)
def test_exact_score_ties_return_the_lowest_rows(ops, monkeypatch, fmt):
    set_lo(monkeypatch, False)
    c = s2.score_tie_case(fmt)
    s = Search(ops, fmt, c["tw"], c["qn"], c["x"], c["xn"], K, idx_offset=OFFSET)
    checked = info, _ = check_all(s, c, fmt, False, K, label=f"score-ties {fmt}")
    record("exact-score-ties", fmt, False, checked, c["planted"])
    ordinary_ok(s, c, info)
    q = PLANTED_Q
    assert (s.out_i[q] - OFFSET).tolist() == c["copies"][:K].tolist() and len(np.unique(sr.f32bits(s.out_s[q]))) == 1
    assert set(c["copies"].tolist()) <= set(s.ws["sel_i"][q, :s.ws["nsel"][q]].tolist()) and s.redo[q] == 0 and s.ws["bound"][q] == -INF


# ------------------------------------------------------------------------------------------------------------------- unboundable
@pytest.mark.parametrize("fmt,lo", [("fp32", False), ("fp16", True), ("bf16", False)], ids=["fp32-hi", "fp16-hi+lo", "bf16-hi"])
def test_unboundable_rows_are_selected_and_score_minus_inf(ops, monkeypatch, fmt, lo):
    set_lo(monkeypatch, lo)
    c = s2.unboundable_case(fmt)
    s = Search(ops, fmt, c["tw"], c["qn"], c["x"], c["xn"], K, idx_offset=OFFSET)
    checked = info, _ = check_all(s, c, fmt, lo, K, label=f"unboundable {fmt}")
    record("unboundable", fmt, lo, checked, c["planted"])
    ordinary_ok(s, c, info)
    assert s.out_s[PLANTED_Q, K - 1] < 0 and s.redo[PLANTED_Q] == 0
    assert (s.out_i[PLANTED_Q, :2] - OFFSET).tolist() == sorted(c["rows"]["zero"])           # the all-zero rows score 0: the best here
    for q in range(Q):
        chosen = set(s.ws["sel_i"][q, :s.ws["nsel"][q]].tolist())
        assert set(c["unb"]) <= chosen, (q, sorted(set(c["unb"]) - chosen))                   # what cannot be bounded is never dropped
        assert not set((s.out_i[q] - OFFSET).tolist()) & set(c["rows"]["nan"] + c["rows"]["inf"] + c["rows"]["late"])


# ---------------------------------------------------------------------------------------------------------------- floor too high
@pytest.mark.parametrize("fmt", s2.FMTS)
def test_floor_too_high_and_floors_that_are_no_numbers(ops, monkeypatch, fmt):
    set_lo(monkeypatch, False)
    c = dict(s2.plain_case(fmt, s2.N_OF[fmt], 600), planted={3: "refused", 4: "needed", 5: "needed"})
    s = Search(ops, fmt, c["tw"], c["qn"], c["x"], c["xn"], K, thr0=s2.floors(c).astype(np.float32), idx_offset=OFFSET)
    checked = info, _ = check_all(s, c, fmt, False, K, label=f"floor {fmt}")
    record("floor-too-high", fmt, False, checked, c["planted"])
    ordinary_ok(s, c, info)
    assert s.ws["cnt"][3] == 0 and s.ws["nsel"][3] == 0 and s.redo[3] == 1
    assert np.isneginf(s.out_s[3]).all() and (s.out_i[3] == -1).all()
    for q in (4, 5):                                                                         # no floor: the oracle's answer (check_soundness)
        assert s.redo[q] == 0 and s.ws["bound"][q] == -INF and K <= s.ws["nsel"][q] <= 256 and np.isfinite(s.ws["tau"][q])


# -------------------------------------------------------------------------------------------------------------------- k = 1, 192
@pytest.mark.parametrize("k", [1, 192])
@pytest.mark.parametrize("fmt", s2.FMTS)
def test_k_1_and_the_ceiling_192(ops, monkeypatch, fmt, k):
    set_lo(monkeypatch, fmt == "fp16")
    N = s2.N_K192[fmt] if k == 192 else s2.N_OF[fmt]
    assert ops.topk_prefilter_applicable(Q, N, s2.D, k) and not ops.topk_prefilter_applicable(Q, N, s2.D, 193)
    assert sr.cap_of(k) == (8192 if k == 192 else 4096)
    c = s2.plain_case(fmt, N, 800 + k)
    s = Search(ops, fmt, c["tw"], c["qn"], c["x"], c["xn"], k, idx_offset=OFFSET)
    assert s.cap == sr.cap_of(k)
    checked = info, _ = check_all(s, c, fmt, fmt == "fp16", k, label=f"k{k} {fmt}")
    record(f"k={k}", fmt, fmt == "fp16", checked, range(Q))
    ordinary_ok(s, c, info)
    assert (s.ws["nsel"] >= k).all() and (np.diff(s.out_s.astype(np.float64), axis=1) <= 0).all()


# --------------------------------------------------------------------------------------------------------------------- selections
@pytest.mark.parametrize("fmt", s2.FMTS)
def test_selection_with_fewer_rows_than_k(ops, monkeypatch, fmt):
    """The FEW instances: 3 selected rows (two whole live tiles: the take-all slice is the whole search), one of them with a NaN:
    have = 2, the (-inf, -1) tail from there, redo = 0."""
    set_lo(monkeypatch, False)
    N = s2.N_OF[fmt]
    c = s2.plain_case(fmt, N, 600, with_nan_row=s2.FEW_ROWS[1])
    flags = np.zeros(N, dtype=bool)
    flags[list(s2.FEW_ROWS)] = True
    s = Search(ops, fmt, c["tw"], c["qn"], c["x"], c["xn"], K, flags=flags, idx_offset=OFFSET)
    assert s.tiles.tolist() == sorted({r // 256 for r in s2.FEW_ROWS})
    checked = info, _ = check_all(s, c, fmt, False, K, flags=flags, few=True, label=f"few {fmt}")
    record("selection-few", fmt, False, checked, range(Q))
    assert (s.ws["cnt"] == 512).all() and (s.ws["nsel"] == 3).all() and np.isneginf(s.ws["bound"]).all() and (s.redo == 0).all()
    good = {s2.FEW_ROWS[0] + OFFSET, s2.FEW_ROWS[2] + OFFSET}
    for q in range(Q):
        assert set(s.out_i[q, :2].tolist()) == good and (s.out_i[q, 2:] == -1).all() and np.isneginf(s.out_s[q, 2:]).all(), q
        assert np.isfinite(s.out_s[q, :2]).all() and info[q]["live"] == 3


@pytest.mark.parametrize("lo", [False, True], ids=["hi", "hi+lo"])
def test_selection_whose_take_all_slice_is_final(ops, monkeypatch, lo):
    """8 live tiles of 10 under a 50 % selection: the final select reads the take-all slice as stored, deselected rows included."""
    set_lo(monkeypatch, lo)
    N = 2560
    c = s2.plain_case("fp16", N, 700)
    flags = sr.selection(N, (3, 6), 5)
    s = Search(ops, "fp16", c["tw"], c["qn"], c["x"], c["xn"], K, flags=flags, idx_offset=OFFSET)
    assert len(s.tiles) == 8 and sr.schedule(N, K, False, True, n_live=8, last_live=1)["launches"] == sr.PHASES_SEL[8]
    checked = info, _ = check_all(s, c, "fp16", lo, K, flags=flags, label=f"take-all-final {LOS[lo]}")
    record("selection-take-all-final", "fp16", lo, checked, range(Q))
    ordinary_ok(s, c, info)
    slot_rows = (s.tiles[:, None].astype(np.int64) * 256 + np.arange(256)[None, :]).reshape(-1)
    assert (s.ws["cnt"] == 2048).all() and (s.ws["cand_i"][:, :2048] == slot_rows[None, :]).all()
    for q in range(Q):
        assert info[q]["live"] == int(flags[slot_rows].sum()) and K <= info[q]["nsel"] <= 256
        assert flags[s.ws["sel_i"][q, :info[q]["nsel"]]].all()


# ----------------------------------------------------------------------------------------------- overflow reaches the certificate
@pytest.mark.parametrize("fmt", s2.FMTS)
def test_overflow_reaches_the_certificate(ops, monkeypatch, fmt):
    """thr0 = -1: the staging lists overflow (the stage-1 file's case) and every query is handed back -- those whose list still
    holds k candidates although their own k-th returned score beats their bound: only the overflow term of the certificate says 1
    (the others, left with an empty list, by the n < k rule as well).  At Q = 40 the lists that survive the overflow are short
    (the needed path: on the MI355X every bound here is -inf), so the comparison below is an easy one; the weight of the case
    lies in check_certificate, which asks redo == (overflow | !(out_s[k-1] > bound)) of every query with the flag read back."""
    set_lo(monkeypatch, False)
    c = dict(s2.plain_case(fmt, 2048, 900), planted=dict.fromkeys(range(Q), "refused"))
    s = Search(ops, fmt, c["tw"], c["qn"], c["x"], c["xn"], K, thr0=np.full(Q, -1.0, np.float32), idx_offset=OFFSET)
    checked = info, _ = check_all(s, c, fmt, False, K, label=f"overflow {fmt}")
    record("overflow", fmt, False, checked, range(Q))
    assert (s.ws["overflow"] == 1).all() and (s.redo == 1).all()
    full = s.ws["nsel"] >= K
    assert full.sum() >= 1 and (s.out_s[full, K - 1] > s.ws["bound"][full]).all()


# ------------------------------------------------------------------------------------------------- the token route's last step
def unorderable(o):
    o = np.asarray(o, dtype=np.uint32)
    return o ^ np.where(o >> 31, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))


class TokenSearch:
    """One call of skyemb_cosine_topk_tokens_prefiltered over the bank xw [N, P, D] (float32 values of `fmt`), guarded."""
    def __init__(self, ops, fmt, q, xw, k, combine, thr0):
        L = ops.lib()
        N, P, D = xw.shape
        nq = q.shape[0]
        flat = xw.reshape(N * P, D)
        tw, qn = so.prep_queries_np(q, None)
        with np.errstate(all="ignore"):
            xn = so.wnorms_np(flat)
        bank, xn_d, rowp, side = prepare(ops, fmt, flat, xn)
        assert side is None
        nbytes = L.skyemb_token_prefilter_ws_bytes(nq, D, k)
        base = L.skyemb_topk_prefilter_ws_bytes(nq, D, k)
        ws, out_s, out_i, redo = Guarded(nbytes), Guarded(nq * k * 4), Guarded(nq * k * 8), Guarded(nq * 4)
        tw_d, qn_d, thr_d = dev(tw), dev(qn), dev(thr0)
        rc = L.skyemb_cosine_topk_tokens_prefiltered(ptr(tw_d), ptr(qn_d), nq, ptr(bank), ops.dtype_code(TORCH16[fmt]), ptr(xn_d), None, rowp.ptr(),
                                                     N, P, D, k, ops.COMBINE_CODES[combine], sr.EPS, OFFSET, ptr(thr_d), ws.ptr(), nbytes,
                                                     out_s.ptr(), out_i.ptr(), redo.ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0, L.skyemb_last_error()
        assert all(g.intact() for g in (ws, out_s, out_i, redo, rowp))
        raw = ws.mem.cpu().numpy()
        self.ws = ws_arrays(raw, ops.topk_prefilter_ws_layout(nq, D, k), nq, D)
        self.keys = raw[base:base + nq * 256 * 8].view(np.uint64).reshape(nq, 256)
        self.out_s, self.out_i, self.redo = out_s.np(np.float32, nq, k), out_i.np(np.int64, nq, k), redo.np(np.int32, nq)

    def list_matches_output(self, q):
        kk = int((self.out_i[q] >= 0).sum())
        keys = self.keys[q, :kk]
        got = set(zip(unorderable(keys >> np.uint64(32)).tolist(), ((~keys) & np.uint64(0xFFFFFFFF)).astype(np.int64).tolist()))
        return got == set(zip(sr.f32bits(self.out_s[q, :kk]).tolist(), (self.out_i[q, :kk] - OFFSET).tolist())) and len(got) == kk


TOKEN = [(fmt, P, combine) for fmt in ("fp16", "bf16") for P in (4, 64) for combine in ("min", "max")]
ZERO_Q, NAN_Q = 7, 1


@pytest.mark.parametrize("fmt,P,combine", TOKEN, ids=[f"{f}-P{p}-{c}" for f, p, c in TOKEN])
def test_token_route_final_list(ops, monkeypatch, fmt, P, combine):
    set_lo(monkeypatch, False)
    N, D = 2560 // P, s2.D
    rng = np.random.default_rng(50 + P)
    q = rng.standard_normal((Q, D), dtype=np.float32)
    q[ZERO_Q] = 0
    centre = rng.standard_normal((N, 1, D))
    xw = sr.store((centre + 0.7 * rng.standard_normal((N, P, D))).reshape(N * P, D), fmt).reshape(N, P, D)
    sc = tpr.tsr.combined_scores(q, xw, combine)
    copies = np.sort(np.concatenate([[int(np.argmax(sc[0]))], rng.permutation(np.setdiff1d(np.arange(N), [int(np.argmax(sc[0]))]))[:2 * K - 1]]))
    xw[copies] = xw[int(np.argmax(sc[0]))]                                                   # 2k bit-identical images
    free = np.setdiff1d(np.arange(N), copies)
    b1 = free[int(np.argmax(sc[NAN_Q][free]))]
    m = int(free[free != b1][0])
    tok = tpr.tsr.token_scores(q[NAN_Q:NAN_Q + 1], xw[b1:b1 + 1])[0, 0]
    xw[m] = xw[b1]
    xw[m, int(np.argmin(tok)) if combine == "max" else 0, 5] = np.nan                        # under max: not the token that decides
    thr0 = np.where(np.arange(Q) % 2 == 0, np.nan, -INF).astype(np.float32)                  # floors that are no floors
    t = TokenSearch(ops, fmt, q, xw, K, combine, thr0)
    with np.errstate(all="ignore"):
        ref_s, ref_i = tpr.tsr.topk_tokens(q, xw, K, combine, None, idx_offset=OFFSET)
    assert np.array_equal(t.redo, t.ws["overflow"]) and t.redo.tolist() == [int(i == ZERO_Q) for i in range(Q)]
    for i in range(Q):
        assert t.list_matches_output(i), i
        if t.redo[i] == 0:
            assert s2.same_answer(t.out_s[i], t.out_i[i], ref_s[i], ref_i[i]), i
    assert (t.out_i[0] - OFFSET).tolist() == copies[:K].tolist()
    if combine == "min":
        assert not ((t.out_i - OFFSET) == m).any()
    else:
        got = (t.out_i[NAN_Q] - OFFSET).tolist()                                             # judged by its other tokens: ties with b1
        assert int(b1) in got and m in got and t.out_s[NAN_Q, got.index(m)] == t.out_s[NAN_Q, got.index(int(b1))]


@pytest.mark.parametrize("fmt,combine", [("fp16", "min"), ("bf16", "max"), ("fp16", "max"), ("bf16", "min")])
def test_token_route_tail_when_fewer_than_k_images_score(ops, monkeypatch, fmt, combine):
    set_lo(monkeypatch, False)
    P, D = 4, s2.D
    N = 2560 // P
    rng = np.random.default_rng(77)
    q = rng.standard_normal((Q, D), dtype=np.float32)
    xw = sr.store(rng.standard_normal((N * P, D)), fmt).reshape(N, P, D)
    dead = np.setdiff1d(np.arange(N), [2, 300, N - 1])
    xw[dead, 0 if combine == "min" else slice(None), 3] = np.nan
    t = TokenSearch(ops, fmt, q, xw, K, combine, None)
    with np.errstate(all="ignore"):
        ref_s, ref_i = tpr.tsr.topk_tokens(q, xw, K, combine, None, idx_offset=OFFSET)
    assert (t.redo == 0).all() and (ref_i[:, 3:] == -1).all() and (ref_i[:, :3] >= 0).all()
    for i in range(Q):
        assert t.list_matches_output(i) and s2.same_answer(t.out_s[i], t.out_i[i], ref_s[i], ref_i[i]), i
