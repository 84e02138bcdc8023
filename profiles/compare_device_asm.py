#!/usr/bin/env python3
"""Compare two sets of gfx950 device assembly kernel by kernel:  compare_device_asm.py DIR_A DIR_B

Each directory holds the .s files that `hipcc <the Makefile's FLAGS and configuration> --cuda-device-only -S file.hip -o
DIR/<file>.<config>.s` wrote for one state of csrc/.  Files are paired by name.  Two files are equal when they define the same
set of .amdhsa_kernel symbols and, for every kernel, the same body and the same .amdhsa_* descriptor block.  The order of
the kernels in the file may differ: the function index in local labels (.LBB<n>_<m>, .Lfunc_begin<n>, .Lfunc_end<n>, ...)
is replaced by a placeholder, comments are dropped (they repeat that index), and the __hip_cuid_<hash> symbol, which depends
on the path compiled from, is replaced too.
Prints one line per file (kernel count, "equal" or the differing kernels); exit status 1 if anything differs."""
import os
import re
import sys

LABEL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def norm(line):
    line = CUID.sub("__hip_cuid_X", line.split(";")[0])      # (comments go: "in Loop: Header=BB<n>_<m>" carries the index too)
    return LABEL.sub(lambda m: ".L%sN%s" % (m.group(1), m.group(3) or ""), line).rstrip()


def kernels(path):
    """name -> (body lines, descriptor lines)"""
    body, desc, cur, in_desc = {}, {}, None, False
    for raw in open(path):
        s = raw.strip()
        m = re.match(r"\.type\s+(\S+),@function", s)
        if m:
            cur = m.group(1); body[cur] = []
            continue
        m = re.match(r"\.set\s+(\S+)\.\w+,", s)       # the resource symbols behind a function (registers, scratch)
        if m and m.group(1) in desc:
            desc[m.group(1)].append(norm(s))
            continue
        if cur is None:
            continue
        if s.startswith(".amdhsa_kernel"):             # the descriptor block lies inside the function
            in_desc = True; desc[cur] = []
        elif s == ".end_amdhsa_kernel":
            in_desc = False
        elif in_desc:
            desc[cur].append(norm(s))
        elif re.match(r"\.size\s+%s," % re.escape(cur), s):
            cur = None
        elif not s.startswith(";"):                    # whole-line comments carry no code
            body[cur].append(norm(s))
    return {k: (body[k], desc[k]) for k in desc}


def main(a, b):
    bad = 0
    names = sorted(f for f in os.listdir(a) if f.endswith(".s"))
    for f in sorted(set(os.listdir(b)) - set(names)):
        if f.endswith(".s"):
            print(f"{f}: only in {b}"); bad = 1
    for f in names:
        if not os.path.exists(os.path.join(b, f)):
            print(f"{f}: only in {a}"); bad = 1
            continue
        ka, kb = kernels(os.path.join(a, f)), kernels(os.path.join(b, f))
        diff = [f"-{k}" for k in sorted(set(ka) - set(kb))] + [f"+{k}" for k in sorted(set(kb) - set(ka))]
        for k in sorted(set(ka) & set(kb)):
            if ka[k][0] != kb[k][0]: diff.append(f"body:{k}")
            if ka[k][1] != kb[k][1]: diff.append(f"descriptor:{k}")
        whole = CUID.sub("X", open(os.path.join(a, f)).read()) == CUID.sub("X", open(os.path.join(b, f)).read())
        print(f"{f}: {len(ka)} / {len(kb)} kernels, " + ("equal" + (" (whole file)" if whole else " (per kernel)") if not diff else "DIFFERENT: " + " ".join(diff)))
        bad |= bool(diff)
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
