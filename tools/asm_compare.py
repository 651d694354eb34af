#!/usr/bin/env python
"""Are two device assembly listings (hipcc ... --cuda-device-only -S of the same translation unit at two commits) the same
instruction stream?  Comment lines, assembler directives and trailing comments are dropped, the per-build __hip_cuid_*
symbol and the function number inside basic-block labels (.LBB<function>_<block>, .Lfunc_end<function>) are masked; what is left - labels and instructions - is compared, and differences are reported per kernel.
    python tools/asm_compare.py parent.s head.s"""
import difflib
import re
import sys


def stream(path):
    out = []
    for line in open(path):
        line = re.sub(r"\s*;.*$", "", line.rstrip("\n")).rstrip()       # (no string of these listings holds a ';')
        s = line.strip()
        if s.startswith(".amdgpu_metadata"):                            # the kernels' metadata (YAML) is no instruction stream
            break
        if not s or s.startswith(".") and not s.endswith(":"):
            continue
        s = re.sub(r"__hip_cuid_\w+", "__hip_cuid_", s)
        # a basic-block label and .Lfunc_end carry their function's number in the translation unit, which moves when a kernel is added in
        # front of it: masked, the block's own number stays
        s = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", s)
        out.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s))
    return out


def by_kernel(lines):
    kernels, name = {}, "(no kernel)"
    for s in lines:
        m = re.match(r"(_Z\w+|\w+_kernel\w*):$", s)
        if m:
            name = m.group(1)
        kernels.setdefault(name, []).append(s)
    return kernels


a, b = stream(sys.argv[1]), stream(sys.argv[2])
print("lines: %d and %d" % (len(a), len(b)))
if a == b:
    print("identical")
    sys.exit(0)
ka, kb = by_kernel(a), by_kernel(b)
for name in sorted(set(ka) | set(kb)):
    if ka.get(name) != kb.get(name):
        d = list(difflib.unified_diff(ka.get(name, []), kb.get(name, []), lineterm="", n=0))
        print("DIFFERS %s: %d diff lines" % (name, len(d)))
        for s in d[:40]:
            print("    " + s)
sys.exit(1)
