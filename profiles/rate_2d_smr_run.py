"""Wall time per step of the reference's refined 2-D blast (decks/athinput.blast2d_smr: 200 x 300, 240^2, 320^2 zones on three
levels; CTU at cour_no = 0.8, default build, no outputs) two ways:

  A  a checkout of the PARENT commit built in a directory of its own (--parent): its Mesh.step() loop -- aa_mesh_step, with three
     CFL reductions and their read-backs per step
  B  this tree's Mesh.run_2d: AA_2D_BATCH = K steps queued per read-back, one clock on the device for all levels
     (k2d_mesh_advance), for K in 4, 8, 16, 32

Every measurement is a process of its own; a repeat is A, then B at every K, and there are --repeats of them.  A timed region is
500 steps between two synchronisations behind a warm-up of 24 steps of the same path; the Mesh is made outside it.  Before anything
is timed, one process per side runs the warm-up and the script asserts that both reach the same (time, dt, nstep) and the same root
block; every timed process reports the same of its end state, and those must agree too.

  git worktree add ../parent HEAD~1 && python -c "import sys; sys.path.insert(0, '../parent'); \\
      import importlib; importlib.import_module('atmospheric-athena_amd.lib').build()"
  python profiles/rate_2d_smr_run.py --parent ../parent [--repeats 5] [--out profiles/rate_2d_smr_run_result.json]

Without --parent, A is this tree's own Mesh.step() loop.  Reads nothing outside the repository and the --parent directory."""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [4, 8, 16, 32]
WARM, STEPS = 24, 500


def child(root, which, k, steps):
    """one process: the Mesh, the warm-up, `steps` timed steps -> a JSON line: microseconds per step and the end state"""
    sys.path.insert(0, root)
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    if which == "B":
        os.environ["AA_2D_BATCH"] = str(k)          # (read when the Mesh is made)
    deck = os.path.join(root, "atmospheric-athena_amd", "decks", "athinput.blast2d_smr")
    ov = ["time/tlim=1e30", "time/cour_no=0.8"]
    par = aa.athinput.ParTable.from_file(deck).cmdline(ov)
    run = aa.config.load(deck, ov, "blast", "ctu")
    m = lib.Mesh(aa.config.levels_2d(par, run), 0, False).start()

    def go(n):
        if which == "B":
            assert m.run_2d_batch() == k
            assert m.run_2d(1e30, nstep_stop=m.nstep + n) == n
        else:
            for _ in range(n):
                m.step()
        m.lev[0].sync()
    go(WARM)
    t0 = time.perf_counter()
    if steps:
        go(steps)
    dt = time.perf_counter() - t0
    assert m.nstep == WARM + steps and m.dt > 0.0, (m.nstep, m.dt)
    out = {"us_per_step": 1e6 * dt / steps if steps else None, "state": [m.time.hex(), m.dt.hex(), m.nstep],
           "root_sha256": hashlib.sha256(m.lev[0].download().tobytes()).hexdigest()}
    m.close()
    print("RATE2DSMR " + json.dumps(out))


def spawn(root, which, k=0, steps=STEPS):
    pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--root", root, "--k", str(k), "--steps", str(steps)],
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    if pr.returncode != 0:
        raise RuntimeError(pr.stderr[-2000:])
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("RATE2DSMR ")][-1]
    return json.loads(line[len("RATE2DSMR "):])


def summary(v):
    return {"us_per_step": v, "median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_2d_smr_run_result.json"))      # (the committed record)
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--steps", type=int, default=STEPS)
    a = ap.parse_args()
    if a.child:
        child(a.root, a.child, a.k, a.steps)
        return
    a_root = os.path.abspath(a.parent) if a.parent else ROOT
    # before anything is timed: both sides after the warm-up
    ca, cb = spawn(a_root, "A", 0, 0), spawn(ROOT, "B", KS[0], 0)
    assert (ca["state"], ca["root_sha256"]) == (cb["state"], cb["root_sha256"]), (ca, cb)
    runs = {"A": []}
    runs.update({k: [] for k in KS})
    for _ in range(a.repeats):
        runs["A"].append(spawn(a_root, "A"))
        for k in KS:
            runs[k].append(spawn(ROOT, "B", k))
    ends = {(tuple(r["state"]), r["root_sha256"]) for v in runs.values() for r in v}
    assert len(ends) == 1, ends
    res = {"deck": "decks/athinput.blast2d_smr", "integrator": "ctu", "cour_no": 0.8, "build": "default",
           "A": "parent commit, Mesh.step() loop" if a.parent else "this tree, Mesh.step() loop", "B": "Mesh.run_2d, AA_2D_BATCH = K",
           "repeats": a.repeats, "warm_up_steps": WARM, "timed_steps": STEPS, "same_state_and_root_block": True,
           "command": "python profiles/rate_2d_smr_run.py%s --repeats %d" % (" --parent <parent checkout>" if a.parent else "", a.repeats)}
    res["A_us"] = summary([r["us_per_step"] for r in runs["A"]])
    for k in KS:
        res[f"B_K{k}_us"] = summary([r["us_per_step"] for r in runs[k]])
    best = min(KS, key=lambda k: res[f"B_K{k}_us"]["median"])
    b = res[f"B_K{best}_us"]
    res["best_K"] = best
    res["A_over_B"] = res["A_us"]["median"] / b["median"]
    res["spread_us"] = max(res["A_us"]["max"] - res["A_us"]["min"], b["max"] - b["min"])
    res["gain_us"] = res["A_us"]["median"] - b["median"]
    res["B_beats_A_by_more_than_the_spread"] = res["gain_us"] > res["spread_us"]
    res["default_K"] = best if res["B_beats_A_by_more_than_the_spread"] else 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
