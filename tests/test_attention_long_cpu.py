"""CPU: the attention and attention-pool entry points refuse sequences past SKYEMB_MHA_MAX_N (4098 tokens: the front end's 4096 patches + cls +
RA/Dec) in argument validation, before any device work, so this runs without a GPU."""
import ctypes
import os
import re

from sky_embeddings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_states_the_token_limit():
    text = open(os.path.join(ROOT, "include", "skyemb.h")).read()
    assert re.search(r"#define\s+SKYEMB_MHA_MAX_N\s+4098\b", text)


def test_mha_rejects_too_long_sequences():
    L = _lib.lib()
    for dtype in (0, 1, 2):
        rc = L.skyemb_mha_fwd(None, None, dtype, 1, 4099, 1, 64, None)
        assert rc == 1 and b"N = 4099 tokens, more than the supported 4098" in L.skyemb_last_error()
        rc = L.skyemb_mha_bwd(None, None, None, dtype, 2, 5000, 3, 32, None)
        assert rc == 1 and b"N = 5000 tokens, more than the supported 4098" in L.skyemb_last_error()


def test_attnpool_rejects_too_long_sequences():
    L = _lib.lib()
    p = ctypes.c_void_p(16)                                   # never dereferenced: validation fails first
    rc = L.skyemb_attnpool_fwd_long(p, p, 0, p, p, 1, 4099, 1, 64, None)
    assert rc == 1 and b"N=4099" in L.skyemb_last_error()
    rc = L.skyemb_attnpool_bwd_long(p, p, 0, p, p, p, p, 1, 4099, 1, 64, None)
    assert rc == 1 and b"N=4099" in L.skyemb_last_error()
    # the plain entry points keep their 256-token contract
    rc = L.skyemb_attnpool_fwd(p, p, 0, p, p, 1, 257, 1, 64, None)
    assert rc == 1 and b"N=257" in L.skyemb_last_error()
    rc = L.skyemb_attnpool_bwd(p, p, 0, p, p, p, p, 1, 257, 1, 64, None)
    assert rc == 1 and b"N=257" in L.skyemb_last_error()
