"""Wall time per step of Driver.main / MeshRun.main WITH the decks' own history block, default build, three ways:

  A   a checkout of the PARENT commit built in a directory of its own (--parent): its main loop as shipped -- the run calls queue
      AA_2D_BATCH / AA_3D_BATCH steps per read-back, and every next time of the ``hst`` block is a stop time of the call
  A0  the same parent with AA_2D_BATCH=0 / AA_3D_BATCH=0: one step, one read-back, the history row from aa_history where due
  B   this tree with OutputSet(hst_queued=True): the block is armed on the device (k_history_dc, k_hst_row behind every queued
      step), no stop time

on  blast2d      decks/athinput.blast2d as shipped, 200 x 300, its <output1> (hst, dt = 0.001); <job>maxout = 1 keeps the other
                 blocks out of the window
    blast2d_smr  decks/athinput.blast2d_smr as shipped, three levels, its <output1> (hst, dt = 0.001), maxout = 1
    blast3d      decks/athinput.blast at 128^3 with an hst block of dt = 0.002 (a few steps apart) -- aa_run_3d

Every measurement is a process of its own that measures ONE side on all three cases; the processes alternate A A0 B A A0 B ...
(--repeats rounds); medians and the spread (min .. max) of the repeats are recorded.  A timed region is one outputs.run() of
STEPS steps (nlim) behind a warm-up run() of WARM steps on the same target and OutputSet, between two synchronisations; it
contains the history rows, their file writes and the forced row at its end.  Also recorded: the rows per step each deck really
produces, and the read-backs per step.

  mkdir ../parent && git archive HEAD~1 | tar -x -C ../parent && make -C ../parent/atmospheric-athena_amd/csrc && make -C ../parent/atmospheric-athena_amd/host
  python profiles/rate_hst_run.py --parent ../parent [--repeats 5] [--out profiles/rate_hst_run_result.json]

Reads nothing outside the repository and the --parent directory."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"blast2d": 500, "blast2d_smr": 500, "blast3d": 200}      # timed steps
WARM = 24
HST3D = "\n<output1>\nout_fmt = hst\ndt      = 0.002\n"


def child(root, side):
    """one process: every case once -> a JSON line"""
    sys.path.insert(0, root)
    pkg = "atmospheric-athena_amd"
    cfg, D, O, A, lib = (importlib.import_module(pkg + "." + m) for m in ("config", "driver", "outputs", "athinput", "lib"))
    if side == "A0":
        os.environ["AA_2D_BATCH"] = os.environ["AA_3D_BATCH"] = "0"      # (read when the Grid / Mesh is made)
    decks = os.path.join(root, pkg, "decks")
    kw = {"hst_queued": True} if side == "B" else {}
    out = {}
    for case, steps in CASES.items():
        tmp = tempfile.mkdtemp(prefix="rate_hst_")
        if case == "blast3d":
            text = open(os.path.join(decks, "athinput.blast")).read() + HST3D
            par = A.ParTable.from_text(text).cmdline(["job/maxout=1", "domain1/Nx1=128", "domain1/Nx2=128", "domain1/Nx3=128", "time/tlim=1e30"])
            t = D.Driver(cfg.from_par(par, "blast"), strict=False)
            grids = [t.eng.g]
        elif case == "blast2d":
            par = A.ParTable.from_file(os.path.join(decks, "athinput.blast2d")).cmdline(["job/maxout=1", "time/tlim=1e30"])
            t = D.Driver(cfg.from_par(par, "blast"), strict=False)
            grids = [t.eng.g]
        else:
            deck = os.path.join(decks, "athinput.blast2d_smr")
            ov = ["job/maxout=1", "time/tlim=1e30"]
            par = A.ParTable.from_file(deck).cmdline(ov)
            run = cfg.load(deck, ov, "blast", "ctu")
            t = D.MeshRun(lib.Mesh(cfg.levels_2d(par, run), 0, False), run)
            grids = list(t.mesh.lev)
        outs = O.OutputSet.from_par(par, 0.0, tmp, **kw)
        O.run(t, outs, 1e30, WARM)
        t.restarted = True                                   # (the second run() neither starts the problem again nor forces a row at its top)
        hst = os.path.join(tmp, outs.written[0])
        rows0 = len(open(hst).read().splitlines())
        for g in grids:
            g.host_syncs(True)
        grids[0].sync()
        t0 = time.perf_counter()
        O.run(t, outs, 1e30, WARM + steps)
        grids[0].sync()
        dt = time.perf_counter() - t0
        assert t.nstep == WARM + steps and t.dt > 0.0, (t.nstep, t.dt)
        rows = len(open(hst).read().splitlines()) - rows0
        out[case] = {"us_per_step": 1e6 * dt / steps, "rows_per_step": rows / steps,
                     "read_backs_per_step": sum(g.host_syncs() for g in grids) / steps}
        (t.mesh.close() if case == "blast2d_smr" else t.eng.close())
    print("RATEHST " + json.dumps(out))


def spawn(root, side):
    pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--root", root], stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=600)
    if pr.returncode != 0:
        raise RuntimeError(pr.stderr[-3000:])
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("RATEHST ")][-1]
    return json.loads(line[len("RATEHST "):])


def summary(v):
    return {"us_per_step": v, "median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_hst_run_result.json"))      # (the committed record)
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        child(a.root, a.child)
        return
    if not a.parent:
        ap.error("--parent: a built checkout of the parent commit")
    roots = {"A": os.path.abspath(a.parent), "A0": os.path.abspath(a.parent), "B": ROOT}
    runs = {s: [] for s in roots}
    for _ in range(a.repeats):
        for s in ("A", "A0", "B"):
            runs[s].append(spawn(roots[s], s))
            print(s, json.dumps({c: round(v["us_per_step"], 1) for c, v in runs[s][-1].items()}), file=sys.stderr, flush=True)
    res = {"build": "default", "repeats": a.repeats, "warm_up_steps": WARM,
           "A": "parent commit, main loop as shipped (hst times are stop times of the queued calls)",
           "A0": "parent commit, AA_2D_BATCH=0 / AA_3D_BATCH=0 (single steps)", "B": "this tree, OutputSet(hst_queued=True)",
           "command": "python profiles/rate_hst_run.py --parent <parent checkout> --repeats %d" % a.repeats, "cases": {}}
    for case, steps in CASES.items():
        r = {"timed_steps": steps}
        for s in runs:
            r[s] = summary([x[case]["us_per_step"] for x in runs[s]])
            r[s]["rows_per_step"] = statistics.median(x[case]["rows_per_step"] for x in runs[s])
            r[s]["read_backs_per_step"] = statistics.median(x[case]["read_backs_per_step"] for x in runs[s])
        best = min(("A", "A0"), key=lambda s: r[s]["median"])
        r["A_over_A0"] = r["A"]["median"] / r["A0"]["median"]
        r["A_slower_than_A0_by_more_than_the_spread"] = r["A"]["median"] - r["A0"]["median"] > max(r["A"]["max"] - r["A"]["min"], r["A0"]["max"] - r["A0"]["min"])
        r["better_of_A_A0"] = best
        r["gain_us"] = r[best]["median"] - r["B"]["median"]
        r["spread_us"] = max(r[best]["max"] - r[best]["min"], r["B"]["max"] - r["B"]["min"])
        r["B_beats_the_better_of_A_A0_by_more_than_the_spread"] = r["gain_us"] > r["spread_us"]
        r["A_over_B"] = r["A"]["median"] / r["B"]["median"]
        r["A0_over_B"] = r["A0"]["median"] / r["B"]["median"]
        res["cases"][case] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
