#!/usr/bin/env python
"""Writes profiles/mse_mean_margins.json: runs tests/test_token_mse_mean_gpu.py::test_per_image_constants_read_back in a child process
with SKYEMB_MSE_MEAN_MARGINS naming a scratch file -- the test then appends one JSON line per case: the largest
L / (D mean (1 + gamma)) and the largest |dot^ - real| / bound it saw over its 64 x 2092 pairs -- and puts the lines into the
committed layout {test, device, note, cases}.

    python tools/mse_mean_margins.py --out profiles/mse_mean_margins.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST = "tests/test_token_mse_mean_gpu.py::test_per_image_constants_read_back"
NOTE = ("per case the largest L / (D mean64 (1 + gamma)) over the pairs with D mean64 > 2^-20 and the largest |dot^ - real| / (eps ||q'|| R1); "
        "dot^ is the exact sum of the 16-bit operands' products over the device's pooled image rounded to fp32, L uses the device's row constants")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mse_mean_margins.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        lines = os.path.join(tmp, "margins.jsonl")
        env = dict(os.environ, SKYEMB_MSE_MEAN_MARGINS=lines)
        subprocess.check_call([sys.executable, "-m", "pytest", TEST, "-q", "-p", "no:cacheprovider"], cwd=ROOT, env=env)
        cases = [json.loads(line) for line in open(lines)]
    import torch                                            # after the child: this process opens the GPU only to name it
    out = dict(test=TEST, device=torch.cuda.get_device_name(0), note=NOTE, cases=cases)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=a.out, cases=len(cases))))


if __name__ == "__main__":
    main()
