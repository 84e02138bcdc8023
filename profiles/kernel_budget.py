#!/usr/bin/env python3
"""Register / scratch / LDS budget of the kernels of one HIP file, from the compiler's own remarks.

  hipcc <the flags of csrc/Makefile> -Rpass-analysis=kernel-resource-usage -c hydro_kernels.hip -o /dev/null 2> new.log
  (the same on the parent commit: parent.log)
  python profiles/kernel_budget.py parent.log new.log > table.md

Prints every kernel of `new.log` whose figures differ from `parent.log`, every kernel that is new, and for a new *_dc entry the
by-value twin it shares a body with; ends with the count of kernels that kept VGPRs, scratch, LDS and occupancy.  Exit status 1
if an existing kernel changed any of the four, or a *_dc entry has scratch or a lower occupancy than its twin.
"""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "vgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"),
          ("LDS Size [bytes/block]", "lds"), ("TotalSGPRs", "sgpr"), ("SGPRs Spill", "sspill"))


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


def read(path):
    kern, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kern.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m:
                cur[key] = int(m.group(1))
    names = demangle(list(kern))
    return {short(names[k]): v for k, v in kern.items()}


def twin_of(name):
    """the by-value entry a *_dc entry shares its body with"""
    m = re.match(r"(aa::)(k_sweep_march|k_x1_edge_flux|k_correct_all|k_flux2_update)(?:_keep)?_dc<(.*)>", name)
    if m:
        return "%s%s<%s>" % m.group(1, 2, 3)
    m = re.match(r"(\(anonymous namespace\)::)(k_restrict|k_flux_correct|k_box_copy)_dc$", name)      # smr_coupling_kernels.h
    if m:
        return m.group(1) + m.group(2)
    return None


def row(name, k):
    return "| `%s` | %d | %d | %d | %d | %d | %d |" % (name, k["vgpr"], k["scratch"], k["occ"], k["lds"], k["sgpr"], k["sspill"])


def main():
    old, new = read(sys.argv[1]), read(sys.argv[2])
    head = "| kernel | VGPRs | scratch B/lane | waves/SIMD | LDS B/block | SGPRs | SGPR spills |\n|---|---|---|---|---|---|---|"
    bad, kept = 0, 0
    keys = ("vgpr", "scratch", "occ", "lds")
    changed = []
    for name, k in sorted(new.items()):
        if name in old:
            if all(old[name][f] == k[f] for f in keys):
                kept += 1
            else:
                changed.append(name)
    print("## existing entry points\n")
    print("%d of %d kept VGPRs, scratch, occupancy and LDS; %d gone.\n" % (kept, kept + len(changed), len(set(old) - set(new))))
    if changed:
        bad = 1
        print(head)
        for name in changed:
            print(row(name + " (parent)", old[name]))
            print(row(name, new[name]))
    print("\n## new entry points (a `*_dc` entry under its by-value twin)\n")
    print(head)
    for name, k in sorted(new.items()):
        if name in old:
            continue
        t = twin_of(name)
        if t:
            if t not in new:
                print("| `%s` | twin not found | | | | | |" % t)
                bad = 1
            else:
                print(row(t, new[t]))
                if k["scratch"] != 0 or k["occ"] < new[t]["occ"]:
                    bad = 1
        print(row(name, k))
    return bad


if __name__ == "__main__":
    sys.exit(main())
