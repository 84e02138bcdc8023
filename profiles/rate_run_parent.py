"""The two run calls of this tree against a checkout of the PARENT commit built in a directory of its own, default build:

  1-D  Grid.run_until(tlim) on decks/athinput.sod1d at 128 and 1200 zones (k1d_run: the whole run in one launch), zone-cycles/s,
       as the first run call of a fresh Grid (rate_1d.py's "resident") and as its second, behind a call of one step: the first
       call of a Grid also makes its clock buffer
  2-D  Grid.run_2d with AA_2D_BATCH = 32 on decks/athinput.blast2d at 64 x 64 and 200 x 300 (k2d_advance behind every step),
       microseconds per step over windows of 500 steps behind 24 warm-up steps

as rate_1d.py and rate_2d_run.py time them: a fresh Grid made outside the timed region, which starts behind a synchronisation and
ends in one.  Every measurement is a process of its own that measures ONE tree; the processes alternate parent, tree, parent, ...
(--repeats pairs).  A process reports the median of five runs (1-D, behind one warm-up run per size) or of five successive windows
(2-D).  Recorded per case: both medians,
both spreads (min .. max over the processes) and whether this tree's median lies within the parent's spread or on the faster
side of it.  The records go into profiles/rate_1d_result.json and profiles/rate_2d_run_result.json under "against_parent".

  git worktree add ../parent HEAD~1 && python -c "import sys; sys.path.insert(0, '../parent'); \\
      import importlib; importlib.import_module('atmospheric-athena_amd.lib').build()"
  python profiles/rate_run_parent.py --parent ../parent [--repeats 5]

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
SIZES_1D = [128, 1200]
SIZES_2D = [(64, 64), (200, 300)]
K, WARM, STEPS, INNER = 32, 24, 500, 5


def child(root):
    sys.path.insert(0, root)
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    decks = os.path.join(root, "atmospheric-athena_amd", "decks")
    out = {}
    for n in SIZES_1D:
        for key, first in (("1d", 0), ("1d_second_call", 1)):      # (second call: the window opens behind a call of one step)
            rates = []
            for rep in range(INNER + 1):                     # (the first: warm-up)
                run = aa.config.load(os.path.join(decks, "athinput.sod1d"), [f"domain1/Nx1={n}"], "shkset1d", "ctu-noh")
                g = lib.setup_problem(aa.config.slab(run), 0, False)
                g.start()
                if first:
                    g.run_until(run.tlim, nstep_stop=first)
                g.sync()
                t0 = time.perf_counter()
                g.run_until(run.tlim)
                g.sync()
                dt = time.perf_counter() - t0
                assert g.time >= run.tlim and g.nstep > first
                rates.append(n * (g.nstep - first) / dt)
                g.close()
            out[f"{key}/{n}"] = statistics.median(rates[1:])
    os.environ["AA_2D_BATCH"] = str(K)                   # (read when the Grid is made)
    for n1, n2 in SIZES_2D:
        run = aa.config.load(os.path.join(decks, "athinput.blast2d"), [f"domain1/Nx1={n1}", f"domain1/Nx2={n2}", "time/tlim=1e30"], "blast")
        g = lib.setup_problem(aa.config.slab(run), 0, False)
        g.start()
        g.run_2d(1e30, nstep_stop=WARM)
        us = []
        for w in range(INNER):
            g.sync()
            t0 = time.perf_counter()
            g.run_2d(1e30, nstep_stop=WARM + (w + 1) * STEPS)
            g.sync()
            us.append(1e6 * (time.perf_counter() - t0) / STEPS)
        assert g.nstep == WARM + INNER * STEPS and g.dt > 0.0, (g.nstep, g.dt)
        out[f"2d/{n1}x{n2}"] = statistics.median(us)
        g.close()
    print("RATERUN " + json.dumps(out))


def spawn(root):
    pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root], stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=300)
    if pr.returncode != 0:
        raise RuntimeError(pr.stderr[-2000:])
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("RATERUN ")][-1]
    return json.loads(line[len("RATERUN "):])


def record(parent, tree, unit, higher_is_better):
    p, t = statistics.median(parent), statistics.median(tree)
    ok = (t >= min(parent)) if higher_is_better else (t <= max(parent))
    return {"unit": unit, "parent": {"values": parent, "median": p, "min": min(parent), "max": max(parent)},
            "tree": {"values": tree, "median": t, "min": min(tree), "max": max(tree)},
            "tree_within_parent_spread_or_faster": ok}


def merge(path, block):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res["against_parent"] = block
    json.dump(res, open(path, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))      # (the committed records)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        child(a.root)
        return
    if not a.parent:
        ap.error("--parent: a built checkout of the parent commit")
    runs = {"parent": [], "tree": []}
    for _ in range(a.repeats):
        runs["parent"].append(spawn(os.path.abspath(a.parent)))
        runs["tree"].append(spawn(ROOT))
    head = {"command": "python profiles/rate_run_parent.py --parent <parent checkout> --repeats %d" % a.repeats, "build": "default",
            "processes_per_tree": a.repeats}
    one = dict(head, what="Grid.run_until(tlim), decks/athinput.sod1d; median of %d runs per process; N: the first run call of a fresh Grid, N_second_call: behind a call of one step" % INNER, sizes={})
    for n in SIZES_1D:
        for key in ("1d", "1d_second_call"):
            one["sizes"][str(n) + key[2:]] = record([r[f"{key}/{n}"] for r in runs["parent"]], [r[f"{key}/{n}"] for r in runs["tree"]],
                                                    "zone-cycles/s", True)
    two = dict(head, what="Grid.run_2d, AA_2D_BATCH = %d, decks/athinput.blast2d; median of %d windows of %d steps per process, behind %d steps" % (K, INNER, STEPS, WARM), sizes={})
    for n1, n2 in SIZES_2D:
        key = f"2d/{n1}x{n2}"
        two["sizes"][f"{n1}x{n2}"] = record([r[key] for r in runs["parent"]], [r[key] for r in runs["tree"]], "us/step", False)
    os.makedirs(a.out_dir, exist_ok=True)
    merge(os.path.join(a.out_dir, "rate_1d_result.json"), one)
    merge(os.path.join(a.out_dir, "rate_2d_run_result.json"), two)
    print(json.dumps({"1d": one, "2d": two}))


if __name__ == "__main__":
    main()
