#!/usr/bin/env python3
"""Are two builds the same device code?  Compares two sets of device-only assembly files function by function.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S viennaray_amd/csrc/vr_trace.hip -o new/vr_trace.s
    tools/isa_diff.py [--rename OLD=NEW ...] old/*.s -- new/*.s

A set is split at its symbols (the `_Z...:` labels of the kernels, the names of data objects), whichever file and order
they come in.  Of a symbol's text the instructions, the local labels, the data and the .amdhsa_* resource lines count;
comments and other directives do not, `.LBB<n>_` labels lose the <n> that the function's position in its file gives
them, clang's path-hashed __hip_cuid_ symbol and the metadata behind the last object are left out.  Prints the symbols
that only one side has and those whose text differs; exit status 1 if there are any.  Text is compared, nothing else.
--rename OLD=NEW: the first set's symbol OLD counts as NEW, in its own text too — a kernel that changed its name alone."""
import re
import sys

DATA = (".byte", ".short", ".long", ".quad", ".zero", ".fill", ".ascii", ".asciz")


def symbols(paths):
    out = {}
    for path in paths:
        here, name = {}, None
        for line in open(path):
            if ".amdgpu_metadata" in line:
                break
            line = line.split(";")[0].strip()
            m = re.match(r'([A-Za-z_$][\w$.]*):$', line)
            if line == ".text":  # (back in the plain text section: the padding behind a file's last function is nobody's)
                name = None
            elif m:
                name = None if m.group(1).startswith("__hip_cuid_") else m.group(1)
                if name:
                    here[name] = []
            elif line and name and (not line.startswith(".") or line.startswith((".amdhsa_", ".L") + DATA)):
                if not line.startswith(".Lfunc_end"):
                    here[name].append(re.sub(r'\.L([A-Za-z]+)\d+_', r'.L\1_', line))
        for name, text in here.items():  # (an inline function that two files of a set emit: the same text, or it counts as differing)
            out[name] = text if out.get(name, text) == text else ["<differs between the files of one set>"]
    return out


def main():
    args, renames = sys.argv[1:], []
    while args[:1] == ["--rename"] and len(args) > 1 and "=" in args[1]:
        renames.append(args[1].split("=", 1))
        args = args[2:]
    if "--" not in args:
        sys.exit(__doc__)
    a, b = symbols(args[:args.index("--")]), symbols(args[args.index("--") + 1:])
    for old, new in renames:
        if old not in a or new in a:
            sys.exit(f"--rename {old}={new}: the first set has no {old}, or has {new} already")
        a[new] = [line.replace(old, new) for line in a.pop(old)]
        print(f"renamed in the first set: {old} -> {new}: {len(a[new])} lines")
    only = sorted(set(a) ^ set(b))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for k in only:
        print(("only in the first set:  " if k in a else "only in the second set: ") + k)
    for k in differ:
        first = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
        print(f"differs: {k}: {len(a[k])} against {len(b[k])} lines, first at line {first}")
    print(f"{len(set(a) & set(b)) - len(differ)} symbols identical, {len(differ)} differ, {len(only)} on one side only")
    sys.exit(1 if only or differ else 0)


if __name__ == "__main__":
    main()
