"""Wall time per step of decks/athinput.ioniz_sphere with K radiation sub-cycles queued per host visit (AA_ION_BATCH = K; default
build, profiling events off, the state resident), by the protocol of profiles/rate_3d.py:

  P   a checkout of the PARENT commit built in a directory of its own (--parent): Grid.step() / Mesh.step() as they were
  K1  this tree, AA_ION_BATCH=1: the per-sub-cycle loop, launch for launch the parent's
  K4, K16  this tree, AA_ION_BATCH = 4 / 16

on two cases:

  sphere80   the deck's 80^3 root alone, from the start: the burst steps (more than one sub-cycle) and, behind them, 20 stationary
             steps (one sub-cycle per step)
  smr80_52   the deck's 80^3 root with its 52^3 level-1 Domain (job/num_domains=2), Mesh.step(): the refined level sub-cycles to
             the root's time in every step

Every measurement is a process of its own; a repeat is P, K1, K4, K16 in that order, and there are --repeats of them per case
(interleaved: drift of the box reaches every leg alike).  A process makes the Grid, takes --steps steps from the start and times
every one of them between two synchronisations of the stream; it reports, per step, microseconds, the sub-cycle count(s) and the
read-backs (host_syncs), and the sha256 of the end state, which must agree over all legs.  Recorded per case and leg: per-step
medians over the repeats, the sums over the burst steps and over the last 20 steps with their min .. max over the repeats.

  python profiles/rate_ion_batch.py --parent <parent checkout> [--repeats 3] [--out profiles/rate_ion_batch_result.json]

Without --parent the P leg is left out.  Reads nothing outside the repository and the --parent directory."""
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
LEGS = {"P": None, "K1": 1, "K4": 4, "K16": 16}
CASES = {"sphere80": (["domain1/Nx1=80", "domain1/Nx2=80", "domain1/Nx3=80"], False, 60),
         "smr80_52": (["job/num_domains=2"], True, 24)}          # overrides, a Mesh, steps
QUIET = 20


def child(root, case, leg):
    sys.path.insert(0, root)
    ov, mesh, steps = CASES[case]
    os.environ.pop("AA_ION_BATCH", None)
    if LEGS[leg] is not None:
        os.environ["AA_ION_BATCH"] = str(LEGS[leg])          # (read when the Grid is made)
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    deck = os.path.join(root, "atmospheric-athena_amd", "decks", "athinput.ioniz_sphere")
    if mesh:
        par = aa.athinput.ParTable.from_file(deck).cmdline(ov)
        m = lib.Mesh(aa.config.levels(par, aa.config.from_par(par, "ioniz_sphere")), 0, False).start()
        grids = m.lev
    else:
        m = lib.setup_problem(aa.config.slab(aa.config.load(deck, ov, "ioniz_sphere")), 0, False)
        m.start()
        grids = [m]
    us, its, syncs = [], [], []
    for g in grids:
        g.sync(); g.host_syncs(True)
    for _ in range(steps):
        t0 = time.perf_counter()
        n = m.step()
        for g in grids:
            g.sync()
        us.append(1e6 * (time.perf_counter() - t0))
        its.append(n if mesh else [n])
        syncs.append(sum(g.host_syncs(True) for g in grids))
    sha = hashlib.sha256()
    for g in grids:
        sha.update(g.download().tobytes())
    out = {"us": us, "its": its, "read_backs": syncs, "dt": m.dt.hex(), "sha256": sha.hexdigest()}
    if LEGS[leg] is not None:
        out["counts"] = [list(g.ion_batch_counts()) for g in grids]
    m.close()
    print("RATEIONBATCH " + json.dumps(out))


def spawn(root, case, leg):
    pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--case", case, "--root", root],
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=280)
    if pr.returncode != 0:
        raise RuntimeError(pr.stderr[-2000:])
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("RATEIONBATCH ")][-1]
    return json.loads(line[len("RATEIONBATCH "):])


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def measure(case, parent, repeats):
    legs = [l for l in LEGS if l != "P" or parent]
    runs = {l: [] for l in legs}
    for _ in range(repeats):
        for l in legs:
            runs[l].append(spawn(parent if l == "P" else ROOT, case, l))
    ends = {(r["dt"], r["sha256"], json.dumps(r["its"])) for v in runs.values() for r in v}
    assert len(ends) == 1, (case, "the legs disagree on the end state or the sub-cycle counts")
    its = runs[legs[0]][0]["its"]
    steps = len(its)
    burst = [i for i in range(steps) if max(its[i]) > 1]
    quiet = list(range(steps - QUIET, steps))
    res = {"overrides": CASES[case][0], "steps": steps, "sub_cycles_per_step": its, "burst_steps": burst,
           "last_steps_all_one_sub_cycle": all(max(its[i]) == 1 for i in quiet), "same_end_state": True, "legs": {}}
    for l in legs:
        rs = runs[l]
        res["legs"][l] = {
            "us_per_step_median": [statistics.median(r["us"][i] for r in rs) for i in range(steps)],
            "read_backs_per_step": rs[0]["read_backs"],
            "burst_us": spread([sum(r["us"][i] for i in burst) for r in rs]) if burst else None,
            "burst_us_without_step_0": spread([sum(r["us"][i] for i in burst if i) for r in rs]) if burst else None,
            "last_%d_us_per_step" % QUIET: spread([sum(r["us"][i] for i in quiet) / QUIET for r in rs]),
            "all_us_per_step": spread([sum(r["us"][1:]) / (steps - 1) for r in rs]),
            "read_backs": sum(rs[0]["read_backs"]), "counts": rs[0].get("counts")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_ion_batch_result.json"))      # (the committed record)
    ap.add_argument("--child", default=None)
    ap.add_argument("--case", default="sphere80")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        child(a.root, a.case, a.child)
        return
    parent = os.path.abspath(a.parent) if a.parent else None
    res = {"deck": "decks/athinput.ioniz_sphere", "build": "default", "repeats": a.repeats, "timed": "every step from the start, a stream synchronisation behind each",
           "P": "parent commit" if parent else None, "command": "python profiles/rate_ion_batch.py%s --repeats %d" % (" --parent <parent checkout>" if parent else "", a.repeats),
           "cases": {}}
    if os.path.exists(a.out):      # (cases measured by an earlier call stay)
        res["cases"] = json.load(open(a.out)).get("cases", {})
    for case in a.cases.split(","):
        res["cases"][case] = measure(case, parent, a.repeats)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({c: {l: {k: v for k, v in d.items() if k.endswith("_us") or k.endswith("per_step") and not k.startswith("us_") or k == "read_backs"}
                          for l, d in r["legs"].items()} for c, r in res["cases"].items()}))


if __name__ == "__main__":
    main()
