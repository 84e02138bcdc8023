"""Zone-cycles per second of a 1-D run (decks/athinput.sod1d to its tlim) three ways, in one invocation on one machine:

  per_step   Grid.step() in a loop: k1d_step + bvals_mhd per step, one read-back of new_dt's maximum per step
  resident   Grid.run_until(tlim): k1d_run, the whole run in ONE launch, one read-back
  reference  oracle/_ref/athena_sod (the unmodified reference, gcc -O3, serial) on the same deck with no outputs: the rate it
             prints itself per cpu-second and per wall-second of its main loop (it prints a line per cycle, into a pipe here),
             and the rate over the wall time of the whole process; the ratios are taken against its own wall-second figure

at 128 zones (the deck's own size: 87 steps) and 1200 zones (the largest deck of the reference's tst/1D-hydro).  The three
alternate A B C A B C ...; medians over the repeats.  Every repeat of ours builds a fresh Grid (problem generator, upload, start)
outside the timed region and ends in a synchronisation inside it.  Reads nothing outside the repository.

  python profiles/rate_1d.py [--sizes 128,1200] [--repeats 7] [--out profiles/rate_1d_result.json]
"""
import argparse
import importlib
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DECK = os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.sod1d")
REFBIN = os.path.join(ROOT, "oracle", "_ref", "athena_sod")


def ours(aa, lib, n, resident):
    run = aa.config.load(DECK, [f"domain1/Nx1={n}"], "shkset1d", "ctu-noh")
    g = lib.setup_problem(aa.config.slab(run), 0, False)
    g.start()
    g.sync()
    t0 = time.perf_counter()
    if resident:
        g.run_until(run.tlim)
    else:
        while g.time < run.tlim:
            g.step()
    g.sync()
    dt = time.perf_counter() - t0
    nstep = g.nstep
    g.close()
    return nstep, dt


def reference(n):
    tmp = tempfile.mkdtemp(prefix="rate_1d_")
    try:
        t0 = time.perf_counter()
        pr = subprocess.run([REFBIN, "-i", DECK, "-d", os.path.join(tmp, "run"), f"domain1/Nx1={n}", "job/maxout=0"],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, errors="replace", cwd=tmp)
        wall = time.perf_counter() - t0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if pr.returncode != 0:
        raise RuntimeError(pr.stdout[-2000:])
    cpu = re.search(r"zone-cycles/cpu-second\s*=\s*([0-9.eE+-]+)", pr.stdout)
    own = re.search(r"zone-cycles/wall-second\s*=\s*([0-9.eE+-]+)", pr.stdout)
    cyc = re.search(r"cycle=\s*(\d+)", pr.stdout[pr.stdout.rfind("cycle="):])
    return int(cyc.group(1)), wall, float(cpu.group(1)), float(own.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,1200")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_1d_result.json"))      # (the committed record)
    a = ap.parse_args()
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    import torch
    res = {"box": torch.cuda.get_device_name(0), "deck": "decks/athinput.sod1d", "build": "default",
           "command": "python profiles/rate_1d.py --sizes %s --repeats %d" % (a.sizes, a.repeats), "sizes": {}}
    have_ref = os.path.exists(REFBIN)
    for n in (int(s) for s in a.sizes.split(",")):
        for resident in (False, True):          # warm-up: code objects loaded, first launches done
            ours(aa, lib, n, resident)
        t = {"per_step": [], "resident": [], "reference_process": [], "reference_cpu": [], "reference_own": []}
        steps = {}
        for _ in range(a.repeats):
            for key, resident in (("per_step", False), ("resident", True)):
                nstep, dt = ours(aa, lib, n, resident)
                steps[key] = nstep
                t[key].append(n * nstep / dt)
            if have_ref:
                nstep, wall, cpu, own = reference(n)
                steps["reference"] = nstep
                t["reference_process"].append(n * nstep / wall)
                t["reference_cpu"].append(cpu)
                t["reference_own"].append(own)
        r = {"zones": n, "steps": steps}
        for key, v in t.items():
            if v:
                r[key] = {"zone_cycles_per_s": v, "median": statistics.median(v)}
        if have_ref:
            ref = r["reference_own"]["median"]
            r["per_step_over_reference"] = r["per_step"]["median"] / ref
            r["resident_over_reference"] = r["resident"]["median"] / ref
        r["resident_over_per_step"] = r["resident"]["median"] / r["per_step"]["median"]
        r["us_per_step"] = {k: 1e6 * n / r[k]["median"] for k in ("per_step", "resident")}
        res["sizes"][str(n)] = r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
