#!/usr/bin/env python
"""Are two device assembly listings (hipcc ... --cuda-device-only -S of the same translation unit at two commits) the same
instruction stream?  Comment lines, assembler directives and trailing comments are dropped and the per-build __hip_cuid_*
symbol is masked; what is left - labels and instructions - is compared, and differences are reported per kernel.
    python tools/asm_compare.py parent.s head.s"""
import difflib
import re
import sys


def stream(path):
    out = []
    for line in open(path):
        line = re.sub(r"\s*;.*$", "", line.rstrip("\n")).rstrip()       # (no string of these listings holds a ';')
        s = line.strip()
        if not s or s.startswith(".") and not s.endswith(":"):
            continue
        out.append(re.sub(r"__hip_cuid_\w+", "__hip_cuid_", s))
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
