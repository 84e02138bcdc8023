"""Wall time per step of a stand-alone 3-D hydro Grid (decks/athinput.blast, CTU + H-correction, default build, no outputs):

  A  a checkout of the PARENT commit built in a directory of its own (--parent): its Grid.step() loop -- the chain's launches, the
     boundary pass and a read-back of new_dt's maxima per step
  B  this tree's Grid.run_3d: AA_3D_BATCH = K steps queued per read-back, dt and dt/dx read from the device clock (k3d_advance),
     for K in 4, 8, 16, 32, with every other knob at its default
  C  (for the record, not part of the bar) B with K = 8 and AA_CORRECT_ALL=1 at the sizes below 4e5 zones, where the default chain
     is the tile kernels and B therefore loops over aa_step: what the queued big-grid chain does where launches dominate

at 32^3, 64^3, 128^3 and 256^3 zones.  Every measurement is a process of its own; the processes alternate A B A B ... (--repeats
pairs), and the medians and the spread (min .. max) of the repeats are recorded.  A timed region starts behind a warm-up of the
same path and a synchronisation and ends in one; the Grid is made outside it.

  git worktree add ../parent HEAD~1 && python -c "import sys; sys.path.insert(0, '../parent'); \\
      import importlib; importlib.import_module('atmospheric-athena_amd.lib').build()"
  python profiles/rate_3d.py --parent ../parent [--repeats 5] [--out profiles/rate_3d_result.json]

Without --parent, A is this tree's own Grid.step() loop (the same kernels as the parent's: aa_step launches what it launched).
Reads nothing outside the repository and the --parent directory."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(32, 400), (64, 400), (128, 200), (256, 48)]      # N (N^3 zones), timed steps
KS = [4, 8, 16, 32]
WARM = 32
SMALL = 400000                                              # zones from which AA_CORRECT_ALL is on by default (api.hip)


def child(root, which):
    """one process: every size (B: every K) once -> a JSON line of microseconds per step"""
    sys.path.insert(0, root)
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    deck = os.path.join(root, "atmospheric-athena_amd", "decks", "athinput.blast")
    out = {}
    for n, steps in SIZES:
        if which == "C" and n ** 3 >= SMALL:
            continue
        for k in (KS if which == "B" else [8] if which == "C" else [0]):
            if which != "A":
                os.environ["AA_3D_BATCH"] = str(k)          # (read when the Grid is made)
            if which == "C":
                os.environ["AA_CORRECT_ALL"] = "1"
            run = aa.config.load(deck, [f"domain1/Nx{d}={n}" for d in (1, 2, 3)] + ["time/tlim=1e30"], "blast")
            g = lib.setup_problem(aa.config.slab(run), 0, False)
            g.start()
            queued = which != "A" and g.run_3d_batch() != 0
            if which != "A":
                g.run_3d(1e30, nstep_stop=WARM)
            else:
                for _ in range(WARM):
                    g.step()
            g.sync()
            g.host_syncs(True)
            t0 = time.perf_counter()
            if which != "A":
                g.run_3d(1e30, nstep_stop=WARM + steps)
            else:
                for _ in range(steps):
                    g.step()
            g.sync()
            dt = time.perf_counter() - t0
            assert g.nstep == WARM + steps and g.dt > 0.0, (g.nstep, g.dt)
            key = f"{n}^3" + (f"/K{k}" if which == "B" else "")
            out[key] = 1e6 * dt / steps
            out[key + "/host_syncs"] = g.host_syncs()
            out[key + "/queued"] = bool(queued)
            g.close()
    print("RATE3D " + json.dumps(out))


def spawn(root, which):
    pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--root", root], stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=600)
    if pr.returncode != 0:
        raise RuntimeError(pr.stderr[-2000:])
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("RATE3D ")][-1]
    print(f"{which} {line}", file=sys.stderr, flush=True)      # (progress: a run is several minutes)
    return json.loads(line[len("RATE3D "):])


def summary(v):
    return {"us_per_step": v, "median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_3d_result.json"))      # (the committed record)
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        child(a.root, a.child)
        return
    a_root = os.path.abspath(a.parent) if a.parent else ROOT
    runs = {"A": [], "B": [], "C": []}
    for _ in range(a.repeats):
        runs["A"].append(spawn(a_root, "A"))
        runs["B"].append(spawn(ROOT, "B"))
    runs["C"].append(spawn(ROOT, "C"))
    res = {"deck": "decks/athinput.blast", "build": "default", "A": "parent commit, Grid.step() loop" if a.parent else "this tree, Grid.step() loop",
           "B": "Grid.run_3d, AA_3D_BATCH = K", "C": "Grid.run_3d, AA_3D_BATCH = 8, AA_CORRECT_ALL=1 (one run)", "repeats": a.repeats, "warm_up_steps": WARM,
           "command": "python profiles/rate_3d.py%s --repeats %d" % (" --parent <parent checkout>" if a.parent else "", a.repeats), "sizes": {}}
    for n, steps in SIZES:
        key = f"{n}^3"
        r = {"zones": n ** 3, "timed_steps": steps, "A": summary([x[key] for x in runs["A"]]), "queued": runs["B"][0][f"{key}/K8/queued"]}
        for k in KS:
            r[f"B_K{k}"] = summary([x[f"{key}/K{k}"] for x in runs["B"]])
            r[f"B_K{k}"]["host_syncs"] = runs["B"][0][f"{key}/K{k}/host_syncs"]
        if key in runs["C"][0]:
            r["C_K8_us_per_step"] = runs["C"][0][key]
        best = min(KS, key=lambda k: r[f"B_K{k}"]["median"])
        b = r[f"B_K{best}"]
        r["best_K"] = best
        r["A_over_B"] = r["A"]["median"] / b["median"]
        r["spread_us"] = max(r["A"]["max"] - r["A"]["min"], b["max"] - b["min"])
        r["gain_us"] = r["A"]["median"] - b["median"]
        r["B_beats_A_by_more_than_the_spread"] = r["gain_us"] > r["spread_us"]
        # the smallest batch within the same-box spread of the best one
        r["smallest_K_within_spread_of_best"] = min(k for k in KS if r[f"B_K{k}"]["median"] - b["median"] <= r["spread_us"])
        r["B_not_slower_than_A_by_more_than_the_spread"] = all(r[f"B_K{k}"]["median"] - r["A"]["median"] <= r["spread_us"] for k in KS)
        res["sizes"][key] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
