"""GPU: the attention entry points give, bit for bit, the results recorded before their host layer became one planner and one driver
(tests/golden/mha_result_hashes.json: SHA-256 of out, dq, dk, dv over CASES and NOMFMA_CASES of tests/test_attention_core_gpu.py,
written by tools/mha_launch_record.py --hashes from the commit before).  The kernels are "same call, same bits" and the operands
come from a seeded CPU generator, so the hashes hold on any MI355X.  tests/test_attention_reference_cpu.py holds the launches
themselves (kernel, grid, workgroup) to the same commit's trace."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_attention_core_gpu as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "mha_result_hashes.json")) as f:
    GOLDEN = json.load(f)


def result_hashes(ops, c):
    """{out, dq, dk, dv: SHA-256 of the bytes} of one forward and one backward call on case c.  Operands are made on the CPU in the
    case's dtype and copied over, results copied back: the two attention kernels are the only launches."""
    qkv, dout = t.inputs(c, c.B * 131 + c.N * 17 + c.hd + c.H)                  # check_case's seed
    D = c.H * c.hd
    qd, dd = qkv.to(c.dtype).to("cuda"), dout.to(c.dtype).to("cuda")
    out = torch.empty(c.B, c.N, D, dtype=c.dtype, device="cuda")
    dqkv = torch.empty(c.B, c.N, 3 * D, dtype=c.dtype, device="cuda")
    ops.mha_fwd(qd, out, c.B, c.N, c.H, c.hd)
    ops.mha_bwd(qd, dd, dqkv, c.B, c.N, c.H, c.hd)
    g = dqkv.cpu().reshape(c.B, c.N, 3, D)
    res = {"out": out.cpu(), "dq": g[:, :, 0], "dk": g[:, :, 1], "dv": g[:, :, 2]}
    as_int = torch.int32 if c.dtype == torch.float32 else torch.int16
    return {n: hashlib.sha256(v.contiguous().view(as_int).numpy().tobytes()).hexdigest() for n, v in res.items()}


def test_golden_lists_every_case():
    assert sorted(GOLDEN) == sorted(t.cid(c) for c in t.CASES + t.NOMFMA_CASES)


@pytest.mark.parametrize("c", t.CASES, ids=t.cid)
def test_results_are_the_recorded_bits(c):
    from sky_embeddings_amd import ops
    assert result_hashes(ops, c) == GOLDEN[t.cid(c)]


def test_results_with_mfma_switched_off_are_the_recorded_bits():
    """SKYEMB_MHA_MFMA=0 is read once per process: a child process."""
    code = r'''
import json
from tests import test_attention_core_gpu as t, test_attention_host_gpu as h
from sky_embeddings_amd import ops
print(json.dumps({t.cid(c): h.result_hashes(ops, c) for c in t.NOMFMA_CASES}))
'''
    env = dict(os.environ, SKYEMB_MHA_MFMA="0", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got == {t.cid(c): GOLDEN[t.cid(c)] for c in t.NOMFMA_CASES}
