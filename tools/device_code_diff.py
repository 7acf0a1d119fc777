#!/usr/bin/env python3
"""Compares the gfx950 device code of two builds of one HIP object file, kernel symbol by kernel symbol: unbundles the code object
of each (.hip_fatbin section -> clang-offload-bundler), disassembles it and compares the instruction text of every function
(addresses and encodings dropped; branch targets print as offsets from their function's start).  A host-only change must give the same symbol set and the
same instructions for every symbol.   usage: device_code_diff.py A.o B.o [--arch gfx950]     exit 1 on a difference"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def functions(obj, arch):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "co.elf")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(d, "copy.o")])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--output={co}",
                               f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}"])
        text = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)
    out, name, start = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            name, start = m.group(2), int(m.group(1), 16)
            out[name] = []
        elif name and line.strip():
            ins = re.sub(r"\s*//.*$", "", line).strip()                    # the address comment
            ins = re.sub(r"<[^>]*\+0x([0-9a-f]+)>", r"<+\1>", ins)          # branch targets: offset from the function's start
            ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)
            out[name].append(ins)
    for body in out.values():                  # the padding up to the next function's alignment belongs to no function
        while body and (body[-1].startswith("s_nop") or body[-1].startswith("s_code_end") or body[-1] == "..."):
            body.pop()
    return out


def main():
    arch = sys.argv[sys.argv.index("--arch") + 1] if "--arch" in sys.argv else "gfx950"
    a, b = functions(sys.argv[1], arch), functions(sys.argv[2], arch)
    only = sorted(set(a) ^ set(b))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print(f"{len(a)} / {len(b)} symbols, {sum(map(len, a.values()))} / {sum(map(len, b.values()))} instructions; in one build only: "
          f"{len(only)}; same name, different instructions: {len(differ)}")
    for k in (only + differ)[:20]:
        print(" ", k)
    sys.exit(1 if only or differ else 0)


if __name__ == "__main__":
    main()
