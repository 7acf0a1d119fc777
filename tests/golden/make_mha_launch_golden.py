#!/usr/bin/env python3
"""Reads the kernel traces of `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/mha_launch_record.py` (one CSV
per process: the CASES leg and the SKYEMB_MHA_MFMA=0 child) into one row per case and direction, in case order:
{kernel (integer template arguments kept), operand (bf16 / f16 / f32: the kernel's element type), grid [x, y] in
threads, workgroup size, lds (the trace's LDS figure: static + dynamic, rounded to the allocation granule)}.

  make_mha_launch_golden.py write DIR OUT.json     tests/golden/mha_launches.json, from the parent commit's trace (without lds:
                                                   the planner states dynamic bytes only, so LDS is compared trace against trace)
  make_mha_launch_golden.py write DIR OUT.json --lds    the same with lds kept (the evidence under profiles/)
  make_mha_launch_golden.py compare DIR_A DIR_B    every field of every row, lds included; prints a summary, exit 1 on a difference
"""
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


OPERAND = (("DF16b", "bf16"), ("DF16_", "f16"), ("bool _Accum", "bf16"), ("float", "f32"))


def short_name(full):
    """(kernel with its integer template arguments, operand format) of a trace's Kernel_Name.  The profiler's demangler does not
    know the 16-bit types: it leaves '_ZN12_GLOBAL__N_119mha_fwd_mfma_kernelILi64ELi1EEEvPKDF16_PDF16_iiii' (DF16_ = _Float16, DF16b =
    __bf16) as it is and prints __bf16 parameters as 'bool _Accum'; fp32 comes out as 'mha_fwd_kernel<float>(float const*, ...)'."""
    operand = next(name for mark, name in OPERAND if mark in full)
    m = re.match(r"_ZN12_GLOBAL__N_1\d+?(mha_[a-z_]+_kernel)I((?:Li\d+E)*)", full)
    if m:
        base, ints = m.group(1), re.findall(r"Li(\d+)E", m.group(2))
    else:
        m = re.match(r"void \(anonymous namespace\)::(mha_[a-z_]+_kernel)<([^>]*)>", full)
        base, ints = m.group(1), [a.strip() for a in m.group(2).split(",") if a.strip().isdigit()]
    return base + (f"<{', '.join(ints)}>" if ints else ""), operand


def rows_of(path):
    """The attention dispatches of one trace CSV in dispatch order (the runtime's own copy kernels dropped)."""
    with open(path, newline="") as f:
        rd = [{k.lower(): v for k, v in r.items()} for r in csv.DictReader(f)]
    rd = sorted((r for r in rd if "mha_" in r["kernel_name"]), key=lambda r: int(r["dispatch_id"]))
    out = []
    for r in rd:
        kernel, operand = short_name(r["kernel_name"])
        out.append({"kernel": kernel, "operand": operand, "grid": [int(r["grid_size_x"]), int(r["grid_size_y"])],
                    "workgroup": int(r["workgroup_size_x"]), "lds": int(r["lds_block_size"])})
    return out


def launches(trace_dir):
    """{case id: {"fwd": row, "bwd": row}} over CASES and NOMFMA_CASES."""
    from tests import test_attention_core_gpu as t
    legs = {2 * len(t.CASES): t.CASES, 2 * len(t.NOMFMA_CASES): t.NOMFMA_CASES}
    assert len(legs) == 2
    z = {}
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)):
        rows = rows_of(path)
        assert len(rows) in legs, (path, len(rows), "dispatches: not two per case of either leg")
        for i, c in enumerate(legs.pop(len(rows))):
            assert "fwd" in rows[2 * i]["kernel"] and "bwd" in rows[2 * i + 1]["kernel"], (t.cid(c), rows[2 * i], rows[2 * i + 1])
            z[t.cid(c)] = {"fwd": rows[2 * i], "bwd": rows[2 * i + 1]}
    assert not legs, "a leg's trace is missing"
    return z


def main():
    if sys.argv[1] == "write":
        z = launches(sys.argv[2])
        for c in z.values():
            for r in c.values():
                if "--lds" not in sys.argv:
                    del r["lds"]
        with open(sys.argv[3], "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(z[k])}" for k in sorted(z)) + "\n}\n")
        print(f"{len(z)} cases -> {sys.argv[3]}")
    else:
        a, b = launches(sys.argv[2]), launches(sys.argv[3])
        diff = [(k, d) for k in sorted(set(a) | set(b)) for d in ("fwd", "bwd") if a.get(k, {}).get(d) != b.get(k, {}).get(d)]
        kernels = {r["kernel"] + " " + r["operand"] for c in a.values() for r in c.values()}
        print(f"{len(a)} / {len(b)} cases, {2 * len(a)} dispatches, {len(kernels)} distinct kernels; kernel name, operand type, grid, "
              f"workgroup size and LDS size differ in {len(diff)} dispatches")
        for k, d in diff[:20]:
            print(" ", k, d, a.get(k, {}).get(d), b.get(k, {}).get(d))
        sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
