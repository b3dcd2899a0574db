#!/usr/bin/env python3
"""Are two builds the same device code?  Compares two sets of device-only assembly files function by function.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S viennaray_amd/csrc/vr_trace.hip -o new/vr_trace.s
    tools/isa_diff.py old/*.s -- new/*.s

A set is split at its symbols (the `_Z...:` labels of the kernels, the names of data objects), whichever file and order
they come in.  Of a symbol's text the instructions, the local labels, the data and the .amdhsa_* resource lines count;
comments and other directives do not, `.LBB<n>_` labels lose the <n> that the function's position in its file gives
them, clang's path-hashed __hip_cuid_ symbol and the metadata behind the last object are left out.  Prints the symbols
that only one side has and those whose text differs; exit status 1 if there are any.  Text is compared, nothing else."""
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
    args = sys.argv[1:]
    if "--" not in args:
        sys.exit(__doc__)
    a, b = symbols(args[:args.index("--")]), symbols(args[args.index("--") + 1:])
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
