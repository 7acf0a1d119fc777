#!/usr/bin/env python3
"""One skyemb_mha_fwd and one skyemb_mha_bwd call per case of tests/test_attention_core_gpu.py (CASES in this process, then
NOMFMA_CASES in a fresh child process with SKYEMB_MHA_MFMA=0: the switch is read once per process).  No other kernel of the project
runs: operands are made on the CPU in the case's dtype and copied over, results copied back.  Two uses, on any two builds of the library:

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/mha_launch_record.py
      the trace then holds two attention launches per case in case order, between the runtime's copy kernels (one CSV per process);
      tests/golden/make_mha_launch_golden.py turns the CSVs into tests/golden/mha_launches.json or compares two runs.
  python3 tools/mha_launch_record.py --hashes OUT.json
      SHA-256 of out, dq, dk, dv per case (tests/golden/mha_result_hashes.json was written this way; tests/test_attention_host_gpu.py
      replays it with the same function).

usage: mha_launch_record.py [--hashes OUT.json] [--leg mfma|nomfma|both]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_attention_core_gpu as t  # noqa: E402
from tests.test_attention_host_gpu import result_hashes  # noqa: E402


def run_leg(cases):
    from sky_embeddings_amd import ops
    ops.lib()
    return {t.cid(c): result_hashes(ops, c) for c in cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hashes")
    ap.add_argument("--leg", default="both", choices=("mfma", "nomfma", "both"))
    a = ap.parse_args()
    z = {}
    if a.leg in ("mfma", "both"):
        z.update(run_leg(t.CASES))
    if a.leg == "nomfma":
        assert os.environ.get("SKYEMB_MHA_MFMA") == "0"
        z.update(run_leg(t.NOMFMA_CASES))
    if a.leg == "both":
        env = dict(os.environ, SKYEMB_MHA_MFMA="0")
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "nomfma", "--hashes", "-"], env=env,
                               capture_output=True, text=True, timeout=600)
        assert child.returncode == 0, child.stdout[-1000:] + child.stderr[-3000:]
        z.update(json.loads(child.stdout.strip().splitlines()[-1]))
    if a.hashes == "-":
        print(json.dumps(z))
    elif a.hashes:
        with open(a.hashes, "w") as f:
            json.dump(z, f, indent=0, sort_keys=True)
            f.write("\n")
    print(f"mha_launch_record: {len(z)} cases, leg {a.leg}", file=sys.stderr)


if __name__ == "__main__":
    main()
