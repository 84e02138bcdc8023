#!/usr/bin/env python3
"""How the kernels of a device assembly file address global memory, beside their register budget.

  hipcc <the flags of csrc/Makefile> --cuda-device-only -S hydro_kernels.hip -o new.s      (the same on the parent commit: parent.s)
  python profiles/addr_forms.py parent.s new.s [name filter, a regular expression] > table.md

Per kernel: instructions, global loads / stores / atomics with a scalar base (`s[a:b]` as the address operand) and without (`off`:
a 64-bit address in a vector register pair), 64-bit vector adds (v_lshl_add_u64, the instruction that forms such an address), lane
reads and writes (scalars kept in lanes of vector registers), no-ops, and VGPRs / SGPRs / scratch / LDS from the kernel descriptor.
"""
import re
import subprocess
import sys


def demangle(names):
    for tool in ("llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def short(name):
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(aa(_cool)?::DevGrid.*$", "", name)


COLS = ("insts", "g_sbase", "g_off", "add_u64", "readlane", "writelane", "nop", "vgpr", "sgpr", "scratch", "lds")


def read(path):
    kern, cur, body = {}, None, False
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = kern.setdefault(m.group(1), dict.fromkeys(COLS, 0))
            body = True
            continue
        if cur is None:
            continue
        s = line.strip()
        if body:
            if s.startswith("s_endpgm"):
                body = False
            if not s or s.startswith((";", ".")) or s.endswith(":"):
                continue
            op = s.split()[0]
            cur["insts"] += 1
            if op.startswith("global_"):
                ops = s.split(";")[0]
                cur["g_sbase" if re.search(r"\bs\[\d+:\d+\]", ops) else "g_off"] += 1
            elif op == "v_lshl_add_u64":
                cur["add_u64"] += 1
            elif op == "v_readlane_b32":
                cur["readlane"] += 1
            elif op == "v_writelane_b32":
                cur["writelane"] += 1
            elif op == "s_nop":
                cur["nop"] += 1
        else:
            for key, pat in (("vgpr", r"\.amdhsa_next_free_vgpr (\d+)"), ("sgpr", r"\.amdhsa_next_free_sgpr (\d+)"),
                             ("scratch", r"\.amdhsa_private_segment_fixed_size (\d+)"), ("lds", r"\.amdhsa_group_segment_fixed_size (\d+)")):
                m = re.search(pat, s)
                if m:
                    cur[key] = int(m.group(1))
    names = demangle(list(kern))
    return {short(names[k]): v for k, v in kern.items()}


def main():
    old, new = read(sys.argv[1]), read(sys.argv[2])
    filt = re.compile(sys.argv[3]) if len(sys.argv) > 3 else None
    print("| kernel | build | " + " | ".join(COLS) + " |\n|---|---|" + "---|"*len(COLS))
    for name in sorted(new):
        if filt and not filt.search(name):
            continue
        for tag, k in (("parent", old.get(name)), ("new", new[name])):
            if k:
                print("| `%s` | %s | " % (name, tag) + " | ".join(str(k[c]) for c in COLS) + " |")


if __name__ == "__main__":
    main()
