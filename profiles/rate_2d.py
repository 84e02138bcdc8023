"""Zone-updates per second of the 2-D CTU path against the 3-D one at the same number of zones.  Same process, same box, two
Grids, blocks of steps alternating A B A B ...; medians of the per-block wall time per step (the blocks end in a synchronisation:
a step's new_dt reads scalars back anyway).

  A  blast on N2 x N2 x 1 (default 4096^2) through aa_integrate_2d_ctu (csrc/hydro2d_kernels.hip)
  B  blast on N3^3 (default 256^3 = the same 1.68e7 zones) through aa_integrate_3d_ctu, unchanged by the 2-D path

  python profiles/rate_2d.py [--n2 4096] [--n3 256] [--blocks 5] [--steps 10] [--out profiles/out/rate_2d.json]

With --profile the per-kernel stage times of both Grids (aa_profile_*) over one more block are added to the result."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n2", type=int, default=4096)
    ap.add_argument("--n3", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "out", "rate_2d.json"))
    a = ap.parse_args()
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    import torch
    decks = os.path.join(ROOT, "atmospheric-athena_amd", "decks")
    # the same cour_no on both sides (0.4: the 3-D integrator takes no more than 0.5), the bubble resolved alike
    cases = {"A": (os.path.join(decks, "athinput.blast2d"), [f"domain1/Nx1={a.n2}", f"domain1/Nx2={a.n2}", "time/cour_no=0.4"], a.n2 * a.n2),
             "B": (os.path.join(decks, "athinput.blast"), [f"domain1/Nx{d}={a.n3}" for d in (1, 2, 3)], a.n3 ** 3)}
    res = {"box": torch.cuda.get_device_name(0),
           "command": "python profiles/rate_2d.py --n2 %d --n3 %d --blocks %d --steps %d" % (a.n2, a.n3, a.blocks, a.steps)}
    grids = {}
    for key, (deck, ov, _n) in cases.items():
        g = lib.setup_problem(aa.config.slab(aa.config.load(deck, ov, "blast")), 0, False)
        g.host_initial = None
        g.start()
        for _ in range(a.warmup):
            g.step()
        g.sync()
        grids[key] = g
    t = {"A": [], "B": []}
    for _ in range(a.blocks):
        for key in ("A", "B"):
            g = grids[key]
            t0 = time.perf_counter()
            for _s in range(a.steps):
                g.step()
            g.sync()
            t[key].append((time.perf_counter() - t0) / a.steps * 1e3)
    for key in ("A", "B"):
        med = statistics.median(t[key])
        res[key] = {"zones": cases[key][2], "ms_per_step": t[key], "median_ms": med, "zone_updates_per_s": cases[key][2] / (med * 1e-3)}
    res["A_over_B_rate"] = res["A"]["zone_updates_per_s"] / res["B"]["zone_updates_per_s"]
    if a.profile:
        for key in ("A", "B"):
            g = grids[key]
            g.profile_enable(True); g.profile_reset()
            for _s in range(a.steps):
                g.step()
            g.sync()
            res[key]["stages_ms_per_step"] = {k: v[0] / a.steps for k, v in g.profile().items()}
            g.profile_enable(False)
    for g in grids.values():
        g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
