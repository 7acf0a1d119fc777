"""CPU: half-precision resident banks (fp16 / bf16) for the patch-token search -- the `_lp` bindings and their refusals before any
device work, the derived bound on what the storage rounding can do to a combined score (against the reference's goldens), and
the Python layer's dtype refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import similarity_oracle as so
from tests import token_search_reference as tsr
from sky_embeddings_amd import _lib, ops, search

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ((130, 1, 512), (65, 16, 128), (65, 64, 64))
LP_SYMBOLS = ("skyemb_cosine_token_scores_lp", "skyemb_cosine_token_topk_lp", "skyemb_weighted_norms_lp", "skyemb_standardise_lp")


def test_lp_bindings_load_and_refuse_bad_arguments_before_any_launch():
    """The four additive entry points exist under the unchanged ABI version 111; every bad call returns non-zero with a text
    that names the cause.  Argument validation happens before any device work, so this is safe without a GPU."""
    L = _lib.lib()
    assert L.skyemb_version() == _lib.ABI_VERSION == 111
    exported = ctypes.CDLL(_lib.SO_PATH)
    for name in LP_SYMBOLS:
        assert name in _lib.PROTOTYPES and hasattr(exported, name), name
    buf = np.zeros(256, np.float32).ctypes.data          # a host address: no call below may get as far as reading it
    F16, BF16, F32 = _lib.F16, _lib.BF16, _lib.F32

    def err(rc):
        assert rc != 0
        return L.skyemb_last_error()

    def topk(bank=buf, dt=F16, P=16, D=64, combine=0, tw=buf):
        return L.skyemb_cosine_token_topk_lp(tw, buf, bank, dt, buf, 1, 10, P, D, 5, combine, 1e-6, 0, 1, None, buf, buf, None)

    def scores(bank=buf, dt=F16, P=16, D=64, combine=0, out=buf):
        return L.skyemb_cosine_token_scores_lp(buf, buf, bank, dt, buf, 1, 10, P, D, combine, 1e-6, out, None)

    for dt in (F16, BF16):
        assert b"bad arguments" in err(topk(bank=None, dt=dt)) and b"skyemb_cosine_token_topk_lp" in L.skyemb_last_error()
        assert b"bad arguments" in err(topk(tw=None, dt=dt))
        assert b"bad arguments" in err(scores(bank=None, dt=dt)) and b"skyemb_cosine_token_scores_lp" in L.skyemb_last_error()
        assert b"bad arguments" in err(scores(out=None, dt=dt))
        assert b"16 % P == 0" in err(topk(P=9, dt=dt)) and b"16 % P == 0" in err(scores(P=9, dt=dt))
        assert b"D % 64 == 0" in err(topk(D=96, dt=dt)) and b"D % 64 == 0" in err(scores(D=96, dt=dt))
        assert b"unknown combine" in err(topk(combine=7, dt=dt)) and b"unknown combine" in err(scores(combine=7, dt=dt))
    for dt in (F32, 7):
        for rc in (topk(dt=dt), scores(dt=dt), topk(dt=dt, bank=None), scores(dt=dt, P=9)):
            msg = err(rc)
            assert b"bank_dtype must be SKYEMB_BF16 (0) or SKYEMB_F16 (2)" in msg and str(dt).encode() in msg
        assert b"dtype must be SKYEMB_BF16 (0) or SKYEMB_F16 (2)" in err(L.skyemb_weighted_norms_lp(buf, dt, None, buf, 4, 64, None))
        assert b"out_dtype must be SKYEMB_BF16 (0) or SKYEMB_F16 (2)" in err(L.skyemb_standardise_lp(buf, buf, buf, buf, dt, 4, 64, None))
    for dt in (F16, BF16):
        assert b"must not be NULL" in err(L.skyemb_weighted_norms_lp(None, dt, None, buf, 4, 64, None))
        assert b"must not be NULL" in err(L.skyemb_weighted_norms_lp(buf, dt, None, None, 4, 64, None))
        assert b"bad shape" in err(L.skyemb_weighted_norms_lp(buf, dt, None, buf, 4, 66, None))
        assert b"bad shape" in err(L.skyemb_weighted_norms_lp(buf, dt, None, buf, 0, 64, None))
        assert b"must not be NULL" in err(L.skyemb_standardise_lp(None, buf, buf, buf, dt, 4, 64, None))
        assert b"must not be NULL" in err(L.skyemb_standardise_lp(buf, buf, None, buf, dt, 4, 64, None))
        assert b"must not be NULL" in err(L.skyemb_standardise_lp(buf, buf, buf, None, dt, 4, 64, None))
        assert b"bad shape" in err(L.skyemb_standardise_lp(buf, buf, buf, buf, dt, 4, 66, None))


@pytest.mark.parametrize("dtype,u", [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)])
def test_storage_rounding_stays_within_the_derived_bound_of_the_goldens(dtype, u):
    """A bank rounded to nearest into fp16 / bf16 moves every combined score by at most 2u / (1 - u): an element-wise relative
    error <= u moves the weighted dot by <= u |t|_w |x|_w (Cauchy-Schwarz) and the norm by a factor within 1 +- u; min, mean
    and max are 1-Lipschitz.  + 1e-6 for the fp32 contract's own distance from the torch formula (5e-7) and the restatement's
    1.8e-7, which leaves 3.2e-7 unused.

    Premise, asserted below: nothing overflows, and every element is rounded with relative error <= u EXCEPT fp16 subnormals
    (|x| < 2^-14; the golden latents do hold a few, the smallest 1.9e-6), whose error is absolute, <= 2^-25.  Those add at most
    e = 2^-25 sqrt(sum of w over the row's subnormal elements) / |x|_w to the dot's and to the norm's relative error, i.e. 2e
    to a score; e <= 1e-7 is asserted for every row and both weight modes, so 2e fits into the unused 3.2e-7 and the bound
    holds as stated."""
    z = np.load(os.path.join(GOLDEN, "similarity.npz"))
    bound = 2 * u / (1 - u) + 1e-6
    worst = 0.0
    for (T, P, N) in CASES:
        key = f"sim/{T}_{P}_{N}"
        tgt, tst = torch.from_numpy(z[key + "/target"]), z[key + "/test"]
        assert np.isfinite(tst).all() and np.abs(tst).max() <= 65504.0, key
        bank16 = torch.from_numpy(tst).to(dtype)
        wide = bank16.to(torch.float32).numpy()
        sub = (np.abs(tst) < 2.0 ** -14) if dtype == torch.float16 else np.zeros(tst.shape, bool)
        assert np.isfinite(wide).all()
        assert (np.abs(wide - tst) <= np.where(sub, 2.0 ** -25, u * np.abs(tst))).all()
        avg, w = so.determine_target_features(tgt)
        for wv in (w.numpy().astype(np.float64), np.ones(tst.shape[-1])):
            e = 2.0 ** -25 * np.sqrt((wv * sub).sum(-1)) / np.sqrt((wv * tst.astype(np.float64) ** 2).sum(-1))
            print(dtype, key, "subnormal elements:", int(sub.sum()), "largest e =", e.max())
            assert e.max() <= 1e-7, (key, e.max())
        for uw in (1, 0):
            s = tsr.token_scores(avg[None].numpy(), wide, w.numpy() if uw else None)
            for combine in tsr.COMBINES:
                err = float(np.abs(tsr.combine_scores(s, combine)[0] - z[f"{key}/cosine_{combine}_{uw}"]).max())
                print(dtype, key, combine, uw, "max |delta| vs golden =", err, "bound", bound)
                assert err <= bound, (dtype, key, combine, uw, err, bound)
                worst = max(worst, err)
    print(dtype, "largest |delta| over the 18 golden arrays =", worst, "bound", bound)


def test_unsupported_bank_dtypes_raise_value_error():
    """TokenBank checks the element type before anything else, so the refusal needs no device; ops' argument checking says the
    same for every entry that takes a bank."""
    for t in (torch.float64, torch.int16):
        bank = torch.zeros(4, 4, 64, dtype=t)
        for call in (lambda: search.TokenBank(bank), lambda: ops.bank_dtype_code(t, "x"),
                     lambda: search.cosine_topk_tokens(torch.zeros(1, 64), bank, 2),
                     lambda: search.cosine_token_scores(torch.zeros(1, 64), bank)):
            with pytest.raises(ValueError, match="torch.float32, torch.float16, torch.bfloat16"):
                call()
    assert [ops.bank_dtype_code(t, "x") for t in (torch.bfloat16, torch.float32, torch.float16)] == [_lib.BF16, _lib.F32, _lib.F16]
    with pytest.raises(ValueError, match="torch.float16 or torch.bfloat16"):
        search.standardise_to(torch.zeros(4, 64), torch.zeros(64), torch.ones(64), torch.float32)
    from sky_embeddings_amd.utils.eval_fns import build_embedding_bank
    with pytest.raises(ValueError, match="bank_dtype"):
        build_embedding_bank(None, [], "cpu", pool='tokens', bank_dtype=torch.float64)
    with pytest.raises(ValueError, match="standardise_with_first_batch"):
        build_embedding_bank(None, [], "cpu", pool='tokens', bank_dtype=torch.float16)


def test_unknown_bank_dtype_exits_from_argparse(capsys):
    import similarity_search
    parser = similarity_search.parseArguments()
    assert parser.parse_args(["m"]).bank_dtype == "f32"
    for name in ("f32", "f16", "bf16"):
        assert parser.parse_args(["m", "--bank-dtype", name]).bank_dtype == name
    with pytest.raises(SystemExit):
        parser.parse_args(["m", "--bank-dtype", "f8"])
    assert "--bank-dtype" in capsys.readouterr().err
