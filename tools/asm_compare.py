#!/usr/bin/env python
"""Are two device assembly listings (hipcc ... --cuda-device-only -S of the same translation unit at two commits) the same
instruction stream?  Comment lines, assembler directives and trailing comments are dropped, the per-build __hip_cuid_*
symbol and the function number inside basic-block labels (.LBB<function>_<block>, .Lfunc_end<function>) are masked; what is left - labels and instructions - is compared, and differences are reported per kernel.
    python tools/asm_compare.py parent.s head.s
Kernels are paired by (mangled) name.  Where a change renames kernels - another template signature, say - every
    --map OLD_REGEX=NEW
rewrites the parent's names (re.sub, in the order given) before the pairing, e.g. --map '(team_kernelILi\dELb\d)ELb1EEEv=\1ELNS_4RowsE3EEEv'
(profiles/scan_rows_refactor_asm_compare.txt has a full set); a kernel's own name inside its stream is rewritten with it.
The pairing of every renamed kernel is printed."""
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
        # every global label opens a section: functions, and the data symbols behind the last of them (the build's
        # __hip_cuid_, the dynamic-LDS table), which belong to no kernel - whichever happens to be the last
        m = re.match(r"([A-Za-z_$][\w$.]*):$", s)
        if m and not s.startswith(".L"):
            name = m.group(1)
        kernels.setdefault(name, []).append(s)
    return kernels


def renamed(kernels, maps):
    """the parent's kernels under the names the head gives them; -> (kernels, {new name: old name} of those that moved)"""
    out, moved = {}, {}
    for name, lines in kernels.items():
        new = name
        for pat, rep in maps:
            new = re.sub(pat, rep, new)
        if new != name:
            moved[new] = name
            lines = [s.replace(name, new) for s in lines]
        out[new] = lines
    return out, moved


args, maps = [], []
argv = sys.argv[1:]
while argv:
    arg = argv.pop(0)
    if arg == "--map":
        pat, _, rep = argv.pop(0).partition("=")
        maps.append((pat, rep))
    else:
        args.append(arg)
a, b = stream(args[0]), stream(args[1])
print("lines: %d and %d" % (len(a), len(b)))
if a == b:
    print("identical")
    sys.exit(0)
ka, kb = by_kernel(a), by_kernel(b)
ka, moved = renamed(ka, maps)
for new in sorted(moved):
    print("paired %s -> %s%s" % (moved[new], new, "" if new in kb else "   (NOT in the second listing)"))
differ = 0
for name in sorted(set(ka) | set(kb)):
    if ka.get(name) != kb.get(name):
        differ += 1
        d = list(difflib.unified_diff(ka.get(name, []), kb.get(name, []), lineterm="", n=0))
        print("DIFFERS %s: %d diff lines" % (name, len(d)))
        for s in d[:40]:
            print("    " + s)
if not differ:
    print("identical in all %d kernels and functions under this pairing" % len(kb))
sys.exit(1 if differ else 0)
