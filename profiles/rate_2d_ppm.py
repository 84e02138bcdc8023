"""Wall time per step of a stand-alone 2-D Grid (decks/athinput.blast2d, default build, no outputs) through Grid.run_2d at second
and at third order (config.load(..., order_2d=3) -> aa_set_order_2d), CTU + H-correction (cour_no 0.8) and van Leer (0.4), at
200 x 300 (the reference's deck) and 1024 x 1024 zones.

Every measurement is a process of its own; the processes alternate order 2, order 3, order 2, ... (--repeats pairs), and the
medians and the spread (min .. max) of the repeats are recorded with the ratio order 3 / order 2 on the same build and box.  A
timed region starts behind a warm-up of the same path and a synchronisation and ends in one; the Grid is made outside it.

Where oracle/_ref/athena_blast_ppm is present (the unmodified reference, gcc -O3, serial, --with-order=3) it is also timed on one
core on the same deck at 200 x 300 with no outputs: the rate it prints itself per wall-second of its main loop.

  python profiles/rate_2d_ppm.py [--repeats 5] [--out profiles/rate_2d_ppm_result.json]

Reads nothing outside the repository."""
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
DECK = os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.blast2d")
REFBIN = os.path.join(ROOT, "oracle", "_ref", "athena_blast_ppm")
SIZES = [(200, 300, 500), (1024, 1024, 100)]      # Nx1, Nx2, timed steps
INTEG = [("ctu", 0.8), ("vl", 0.4)]
WARM = 32                                         # one batch at the default AA_2D_BATCH
REF_STEPS = 60


def child(order):
    """one process: every size and integrator once at this order -> a JSON line of microseconds per step"""
    sys.path.insert(0, ROOT)
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    out = {}
    for n1, n2, steps in SIZES:
        for integ, cour in INTEG:
            run = aa.config.load(DECK, [f"domain1/Nx1={n1}", f"domain1/Nx2={n2}", "time/tlim=1e30", f"time/cour_no={cour}"], "blast",
                                 integ, order_2d=order)
            g = lib.setup_problem(aa.config.slab(run), 0, False)
            assert g.order == order
            g.start()
            g.run_2d(1e30, nstep_stop=WARM)
            g.sync()
            t0 = time.perf_counter()
            g.run_2d(1e30, nstep_stop=WARM + steps)
            g.sync()
            dt = time.perf_counter() - t0
            assert g.nstep == WARM + steps and g.dt > 0.0, (g.nstep, g.dt)
            out[f"{n1}x{n2}/{integ}"] = 1e6 * dt / steps
            g.close()
    print("RATE2DPPM " + json.dumps(out))


def spawn(order):
    pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(order)], stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=300)
    if pr.returncode != 0:
        raise RuntimeError(pr.stderr[-2000:])
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("RATE2DPPM ")][-1]
    return json.loads(line[len("RATE2DPPM "):])


def reference(n1, n2):
    """the reference's third-order CTU build on one core: microseconds per step from the rate it prints for its main loop"""
    tmp = tempfile.mkdtemp(prefix="rate_2d_ppm_")
    try:
        pr = subprocess.run([REFBIN, "-i", DECK, "-d", os.path.join(tmp, "run"), f"domain1/Nx1={n1}", f"domain1/Nx2={n2}", "job/maxout=0",
                             f"time/nlim={REF_STEPS}", "time/tlim=1e30"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                            errors="replace", cwd=tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if pr.returncode != 0:
        raise RuntimeError(pr.stdout[-2000:])
    own = re.search(r"zone-cycles/wall-second\s*=\s*([0-9.eE+-]+)", pr.stdout)
    return 1e6 * n1 * n2 / float(own.group(1))


def summary(v):
    return {"us_per_step": v, "median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_2d_ppm_result.json"))      # (the committed record)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return
    runs = {2: [], 3: []}
    for _ in range(a.repeats):
        runs[2].append(spawn(2))
        runs[3].append(spawn(3))
    res = {"deck": "decks/athinput.blast2d", "build": "default", "path": "Grid.run_2d, AA_2D_BATCH default", "repeats": a.repeats,
           "warm_up_steps": WARM, "order": "ABAB: a process per order, alternating", "command": "python profiles/rate_2d_ppm.py --repeats %d" % a.repeats,
           "cases": {}}
    for n1, n2, steps in SIZES:
        for integ, cour in INTEG:
            key = f"{n1}x{n2}/{integ}"
            o2, o3 = summary([x[key] for x in runs[2]]), summary([x[key] for x in runs[3]])
            res["cases"][key] = {"zones": n1 * n2, "timed_steps": steps, "cour_no": cour, "order2": o2, "order3": o3,
                                 "order3_over_order2": o3["median"] / o2["median"],
                                 "spread_us": max(o2["max"] - o2["min"], o3["max"] - o3["min"])}
    if os.path.exists(REFBIN):
        try:
            v = [reference(200, 300) for _ in range(min(3, a.repeats))]
            r = summary(v)
            r["what"] = "oracle/_ref/athena_blast_ppm, one core, %d steps, its own zone-cycles/wall-second" % REF_STEPS
            r["over_order3_ctu"] = r["median"] / res["cases"]["200x300/ctu"]["order3"]["median"]
            res["reference_200x300_ctu"] = r
        except Exception as e:      # (the measurement of the library stands without it)
            res["reference_200x300_ctu"] = {"error": str(e)[-500:]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
