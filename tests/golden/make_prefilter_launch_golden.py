#!/usr/bin/env python3
"""Reads the kernel trace of `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/prefilter_launch_record.py` into,
per case of tests/prefilter_plan_cases.py, the ordered launches of its one search call: {kernel (template arguments kept, bools as
0 / 1), grid [x, y] in threads, workgroup size, lds (the trace's LDS figure: static + dynamic, rounded to the allocation granule)}.
Only the search's own kernels count (SEARCH_KERNELS): the preparation kernels and torch's are dropped; a call starts at its
query16_kernel.

  make_prefilter_launch_golden.py write DIR OUT.json          tests/golden/prefilter_launches.json, from the trace of the commit
                                                               before the planner existed (without lds: the planner states dynamic
                                                               bytes only, so LDS is compared trace against trace)
  make_prefilter_launch_golden.py write DIR OUT.json --lds    the same with lds kept (the evidence under profiles/)
  make_prefilter_launch_golden.py compare A B                 A, B: trace directories or --lds JSON files; every field of every
                                                               launch, lds included; prints a summary, exit 1 on a difference
"""
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SEARCH_KERNELS = {"query16_kernel", "init_state_kernel", "token_state_kernel", "prefilter_kernel", "bucket_kernel", "select_kernel",
                  "rescore_kernel", "rescore_lp_kernel", "rescore_bf_kernel", "token_rescore_lp_kernel", "token_rescore_bf_kernel",
                  "token_rescore_top_lp_kernel", "token_rescore_top_bf_kernel"}


def short_name(full):
    """'prefilter_kernel<2,0,1,0,1,0>' of a trace's Kernel_Name, or None when it is not a kernel of the anonymous namespace.  The
    profiler's demangler does not know the 16-bit types: a kernel with a _Float16 / __bf16 parameter stays mangled
    ('_ZN12_GLOBAL__N_116prefilter_kernelILi2ELb0E...EEvPKDF16_...'), the others come out as 'void (anonymous namespace)::name<...>(...)'."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", full)
    if m:
        rest = full[m.end():]
        base, rest = rest[:int(m.group(1))], rest[int(m.group(1)):]
        t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
        args = re.findall(r"L[ib](\d+)E", t.group(1)) if t else []
    else:
        m = re.match(r"(?:void )?\(anonymous namespace\)::(\w+)(?:<([^>]*)>)?", full)
        if not m:
            return None
        base = m.group(1)
        args = [{"true": "1", "false": "0"}.get(a.strip(), a.strip()) for a in (m.group(2) or "").split(",") if a.strip()]
    return base + (f"<{','.join(args)}>" if args else "")


def calls_of(trace_dir):
    """The search calls of a trace in dispatch order: a list of launch lists."""
    paths = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    assert len(paths) == 1, (trace_dir, paths, "expected the trace of one process")
    with open(paths[0], newline="") as f:
        rd = [{k.lower(): v for k, v in r.items()} for r in csv.DictReader(f)]
    calls = []
    for r in sorted(rd, key=lambda r: int(r["dispatch_id"])):
        kernel = short_name(r["kernel_name"])
        if kernel is None or kernel.split("<")[0] not in SEARCH_KERNELS:
            continue
        if kernel.startswith("query16_kernel"):
            calls.append([])
        calls[-1].append({"kernel": kernel, "grid": [int(r["grid_size_x"]), int(r["grid_size_y"])], "workgroup": int(r["workgroup_size_x"]),
                          "lds": int(r["lds_block_size"])})
    return calls


def launches(src):
    """{case id: [launch, ...]} of a trace directory, or of a JSON file written with --lds."""
    if os.path.isfile(src):
        with open(src) as f:
            return json.load(f)
    from tests import prefilter_plan_cases as pc
    calls = calls_of(src)
    assert len(calls) == len(pc.CASES), (len(calls), len(pc.CASES), "search calls in the trace: not one per case")
    return {c["id"]: rows for c, rows in zip(pc.CASES, calls)}


def main():
    if sys.argv[1] == "write":
        z = launches(sys.argv[2])
        if "--lds" not in sys.argv:
            for rows in z.values():
                for r in rows:
                    del r["lds"]
        with open(sys.argv[3], "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: [\n  " + ",\n  ".join(json.dumps(r) for r in v) + "\n]" for k, v in z.items())
                    + "\n}\n")
        print(f"{len(z)} cases, {sum(len(v) for v in z.values())} launches -> {sys.argv[3]}")
    else:
        a, b = launches(sys.argv[2]), launches(sys.argv[3])
        diff = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        kernels = {r["kernel"] for v in a.values() for r in v}
        print(f"{len(a)} / {len(b)} cases, {sum(len(v) for v in a.values())} / {sum(len(v) for v in b.values())} launches, {len(kernels)} "
              f"distinct kernels; kernel name, grid, workgroup size and LDS size differ in {len(diff)} cases")
        for k in diff[:20]:
            print(" ", k, a.get(k), b.get(k), sep="\n    ")
        sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
