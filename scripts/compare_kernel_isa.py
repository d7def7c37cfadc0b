#!/usr/bin/env python3
"""Do two builds of one translation unit hold the same gfx950 code for the kernels they share?

    python scripts/compare_kernel_isa.py OLD.o NEW.o [--drop-trailing-false]

Unbundles the gfx950 code object of each hipcc object file, disassembles it (llvm-objdump -d, no addresses, no encodings) and
compares the instruction text kernel by kernel.  --drop-trailing-false: a kernel template of NEW gained one trailing `bool`
argument that defaults to false; the `Lb0E` it adds to the mangled name is removed before matching, and the `Lb1E`
instantiations count as new.  Prints one line per differing or missing kernel and a summary; exit status 1 if any shared kernel
differs.  profiles/global_latent.md records the run for the no-volume instantiations."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(\S+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and line.strip():
            out[cur].append(re.sub(r"//.*", "", line).strip())
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    drop = "--drop-trailing-false" in sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(args[0], tmp, "old"), kernels(args[1], tmp, "new")
    added = 0
    if drop:
        renamed = {}
        for k, v in new.items():
            m = re.match(r"(.*I.*)Lb([01])E(EEv.*)$", k)
            base = m.group(1) + m.group(3) if m else None
            if m and m.group(2) == "0" and base in old and k not in old:
                renamed[base] = v
            elif m and m.group(2) == "1" and base in old and k not in old:
                added += 1
            else:
                renamed[k] = v
        new = renamed
    same = differ = missing = 0
    for k, v in old.items():
        if k not in new:
            missing += 1
            print("missing in NEW:", k)
        elif v == new[k]:
            same += 1
        else:
            differ += 1
            print("differs:", k, len(v), "->", len(new[k]), "instructions")
    print(f"{len(old)} kernels in OLD: {same} identical, {differ} different, {missing} missing; {added} new instantiations in NEW")
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main())
