"""CPU: the restatement of the token search under a selection of images (tests/token_select_reference.py): its identities, the
poison and tie rules, the bit layout of the packed words; the refusals of the `_sel` entry points and of the Python layer before
any device work; the command line's --bank-select-snr."""
import numpy as np
import pytest
import torch

from tests import token_search_reference as tsr
from tests import token_select_reference as tsel
from tests import token_topt_reference as ttr
from sky_embeddings_amd import _lib

NINF = np.float32(-np.inf)


def _case(seed, N=41, P=4, D=64, Q=3):
    rng = np.random.default_rng(seed)
    w = rng.random(D, dtype=np.float32) + 0.1
    return rng.standard_normal((N, P, D), dtype=np.float32), rng.standard_normal((Q, D), dtype=np.float32), w / w.sum(), rng


def test_packed_words_bit_layout():
    """bit i & 31 of word i >> 5 is image i; ceil(N / 32) words; padding bits zero; unpack inverts pack."""
    for N in (1, 31, 32, 33, 37, 64, 531):
        flags = np.random.default_rng(N).random(N) < 0.5
        flags[[0, N - 1]] = True
        words = tsel.pack_words(flags)
        assert words.dtype == np.uint32 and words.shape == ((N + 31) // 32,)
        for i in range(N):
            assert bool((int(words[i >> 5]) >> (i & 31)) & 1) == bool(flags[i])
        if N % 32:
            assert int(words[-1]) >> (N % 32) == 0
        assert np.array_equal(tsel.unpack_words(words, N), flags)
    assert tsel.pack_words(np.array([True] + [False] * 32 + [True]))[0] == 1 and tsel.pack_words(np.ones(40, bool))[1] == 0xFF


def test_all_ones_selection_is_the_plain_search():
    bank, q, w, _ = _case(1)
    bank[5, 2, 3] = np.nan
    ones = np.ones(bank.shape[0], bool)
    for combine in tsr.COMBINES:
        for k in (1, 7, 41):
            ref = tsr.topk_tokens(q, bank, k, combine, w, idx_offset=9)
            got = tsel.topk_tokens_select(q, bank, k, combine, ones, weights=w, idx_offset=9)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
            ref = ttr.topk_tokens_top(q, bank, k, combine, 3, w)
            got = tsel.topk_tokens_select(q, bank, k, combine, ones, top_t=3, weights=w)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert np.array_equal(tsel.token_scores_select(q, bank, combine, ones, weights=w), tsr.combined_scores(q, bank, combine, w))


def test_selection_from_whole_bank_token_scores_is_the_compacted_bank():
    """A token score depends on its own row only: slicing the whole bank's token scores is scoring the compacted bank."""
    bank, q, w, rng = _case(2)
    flags = rng.random(bank.shape[0]) < 0.5
    s = tsr.token_scores(q, bank, w)
    assert np.array_equal(s[:, flags], tsr.token_scores(q, np.ascontiguousarray(bank[flags]), w))
    for combine in tsr.COMBINES:
        for t in (None, 2):
            a = tsel.topk_tokens_select(q, bank, 7, combine, flags, top_t=t, weights=w, idx_offset=3)
            b = tsel.topk_of_token_scores_select(s, 7, combine, flags, top_t=t, idx_offset=3)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            assert np.array_equal(tsel.token_scores_select(q, bank, combine, flags, t, w),
                                  tsel.scores_of_token_scores_select(s, combine, flags, t))


def test_result_is_the_plain_search_with_deselected_images_removed():
    """Independent of the compaction: the whole bank's combined scores with the deselected columns at -inf, then top-k."""
    bank, q, w, rng = _case(3)
    flags = rng.random(bank.shape[0]) < 0.4
    for combine in tsr.COMBINES:
        sc = tsr.combined_scores(q, bank, combine, w)
        sc[:, ~flags] = NINF
        ref = tsr.topk_of_scores(sc, 30, 5)
        got = tsel.topk_tokens_select(q, bank, 30, combine, flags, weights=w, idx_offset=5)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        n = int(flags.sum())
        assert n < 30 and (got[1][:, n:] == -1).all() and np.isneginf(got[0][:, n:]).all() and (got[1][:, :n] >= 5).all()


def test_poisoned_deselected_images_leave_the_result_unchanged():
    bank, q, w, rng = _case(4)
    flags = rng.random(bank.shape[0]) < 0.5
    for poison in (np.nan, 1e30, -1e30):
        bad = bank.copy()
        bad[~flags] = poison
        for combine in tsr.COMBINES:
            for t in (None, 1, 4):
                a = tsel.topk_tokens_select(q, bank, 10, combine, flags, top_t=t, weights=w)
                b = tsel.topk_tokens_select(q, bad, 10, combine, flags, top_t=t, weights=w)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                assert np.array_equal(tsel.token_scores_select(q, bank, combine, flags, t, w),
                                      tsel.token_scores_select(q, bad, combine, flags, t, w))


def test_ties_across_a_deselected_image_go_to_the_lower_index():
    bank, q, w, _ = _case(5, N=12)
    bank[3] = bank[6] = bank[9] = bank[1]                        # four equal images; 6 is deselected
    flags = np.ones(12, bool)
    flags[6] = False
    q = bank[1].mean(axis=0, keepdims=True)
    for combine in tsr.COMBINES:
        s, i = tsel.topk_tokens_select(q, bank, 12, combine, flags, weights=w, idx_offset=100)
        pos = [int(np.where(i[0] == 100 + j)[0][0]) for j in (1, 3, 9)]
        assert pos[1] == pos[0] + 1 and pos[2] == pos[0] + 2 and s[0][pos[0]] == s[0][pos[2]]
        assert not (i == 106).any() and i[0, 11] == -1 and np.isneginf(s[0, 11])


def test_empty_selection():
    bank, q, w, _ = _case(6)
    s, i = tsel.topk_tokens_select(q, bank, 5, "mean", np.zeros(bank.shape[0], bool), weights=w)
    assert np.isneginf(s).all() and (i == -1).all() and s.shape == (3, 5)
    assert np.isneginf(tsel.token_scores_select(q, bank, "max", np.zeros(bank.shape[0], bool))).all()


def test_sel_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument validation happens before any device work, so this is safe without a GPU.  The refusals are those of the `_top`
    calls plus the alignment of `select`; select == NULL reaches the `_top` call's own text."""
    L = _lib.lib()
    assert L.skyemb_version() == _lib.ABI_VERSION == 111
    for name in ("skyemb_cosine_token_scores_sel", "skyemb_cosine_token_topk_sel", "skyemb_pack_select"):
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    buf = np.zeros(256, np.float32).ctypes.data           # a host address: no call below may get as far as reading it

    def err(rc):
        assert rc != 0
        return L.skyemb_last_error()

    def topk(dt=_lib.F32, P=4, D=64, combine=0, top_t=2, bank=buf, sel=buf):
        nl = L.skyemb_cosine_token_topk_chunks(10, P, 1, D, 5)         # 0 for a shape that is refused anyway
        return L.skyemb_cosine_token_topk_sel(buf, buf, bank, dt, buf, 1, 10, P, D, 5, combine, top_t, 1e-6, 0, nl, None, buf, buf, sel, None)

    def scores(dt=_lib.F32, P=4, D=64, combine=0, top_t=2, bank=buf, sel=buf):
        return L.skyemb_cosine_token_scores_sel(buf, buf, bank, dt, buf, 1, 10, P, D, combine, top_t, 1e-6, buf, sel, None)

    for dt in (_lib.F32, _lib.F16, _lib.BF16):
        for call in (topk, scores):
            for top_t, P in ((-1, 4), (17, 4), (5, 4), (17, 64)):
                assert f"top_t={top_t} P={P}".encode() in err(call(dt=dt, P=P, top_t=top_t))
            assert b"unknown combine" in err(call(dt=dt, combine=7))
            assert b"16 % P == 0" in err(call(dt=dt, P=9)) and b"D % 64 == 0" in err(call(dt=dt, D=96))
            assert b"bad arguments" in err(call(dt=dt, bank=None))
            for off in (1, 2, 3):
                msg = err(call(dt=dt, sel=buf + off))
                assert b"select must be 4-byte aligned" in msg and b"_sel" in msg, msg
    for dt in (3, 7, -1):
        for call in (topk, scores):
            msg = err(call(dt=dt))
            assert b"bank_dtype must be" in msg and str(dt).encode() in msg, msg
    assert b"nlists must come from" in err(L.skyemb_cosine_token_topk_sel(buf, buf, buf, _lib.F32, buf, 1, 10, 4, 64, 5, 0, 0, 1e-6, 0, 3,
                                                                         None, buf, buf, buf, None))
    # select == NULL is the `_top` call
    top = err(L.skyemb_cosine_token_topk_top(None, None, None, _lib.F32, None, 1, 10, 16, 64, 5, 0, 0, 1e-6, 0, 1, None, None, None, None))
    assert err(L.skyemb_cosine_token_topk_sel(None, None, None, _lib.F32, None, 1, 10, 16, 64, 5, 0, 0, 1e-6, 0, 1, None, None, None, None,
                                              None)) == top
    top = err(L.skyemb_cosine_token_scores_top(buf, buf, buf, _lib.F32, buf, 1, 10, 4, 64, 0, 9, 1e-6, buf, None))
    assert err(L.skyemb_cosine_token_scores_sel(buf, buf, buf, _lib.F32, buf, 1, 10, 4, 64, 0, 9, 1e-6, buf, None, None)) == top
    assert b"skyemb_pack_select: bad arguments" in err(L.skyemb_pack_select(None, 10, buf, None))
    assert b"skyemb_pack_select: bad arguments" in err(L.skyemb_pack_select(buf, 0, buf, None))
    assert b"4-byte aligned" in err(L.skyemb_pack_select(buf, 10, buf + 2, None))


def test_python_layer_refuses_bad_selections_before_any_device_work():
    from sky_embeddings_amd import search
    for flags in (torch.ones(8, dtype=torch.uint8), torch.ones(8), torch.ones(2, 4, dtype=torch.bool), torch.tensor(True), [True] * 8):
        with pytest.raises(ValueError, match="Selection"):
            search.Selection(flags)
    bank, q = torch.zeros(8, 4, 64), torch.zeros(1, 64)
    for bad in (torch.ones(7, dtype=torch.bool), torch.ones(9, dtype=torch.bool)):
        with pytest.raises(ValueError, match="select describes"):
            search.cosine_topk_tokens(q, bank, 2, select=bad)
        with pytest.raises(ValueError, match="select describes"):
            search.cosine_token_scores(q, bank, select=bad)
        with pytest.raises(ValueError, match="select describes"):
            search.cosine_topk(q, torch.zeros(8, 64), 2, select=bad)
    with pytest.raises(ValueError, match="Selection"):
        search.cosine_topk_tokens(q, bank, 2, select=torch.ones(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="flat"):
        search.cosine_topk(q, bank, 2, select=torch.ones(8, dtype=torch.bool))


def test_cli_bank_select_snr_needs_bank(monkeypatch):
    import similarity_search
    parser = similarity_search.parseArguments()
    assert parser.parse_args(["m"]).bank_select_snr is False
    assert parser.parse_args(["m", "--bank", "--bank-select-snr"]).bank_select_snr is True
    monkeypatch.setattr("sys.argv", ["similarity_search.py", "m", "--bank-select-snr"])
    with pytest.raises(SystemExit) as e:
        similarity_search.main()
    assert "--bank-select-snr" in str(e.value) and "--bank" in str(e.value).replace("--bank-select-snr", "")
