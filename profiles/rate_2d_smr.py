"""Milliseconds per step of the reference's three-level 2-D blast (decks/athinput.blast2d_smr: 200 x 300, 240^2, 320^2) through
aa_mesh_step, beside the sum of its three levels run as stand-alone 2-D Grids of the same sizes (the capability before 2-D meshes
existed).  The difference is what restriction, flux correction, prolongation and the kept-flux stores cost.  Same process, same
box, blocks of steps alternating mesh / level 0 / level 1 / level 2; medians of the per-block wall time per step (a block ends
in a synchronisation: a step's new_dt reads scalars back anyway).

  python profiles/rate_2d_smr.py [--blocks 5] [--steps 20] [--warmup 5] [--limit 300] [--out profiles/out/rate_2d_smr.json]

--limit: one time limit in seconds for the whole measurement (checked between blocks; what was measured until then is kept)."""
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
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=float, default=300.0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "out", "rate_2d_smr.json"))
    a = ap.parse_args()
    t_start = time.perf_counter()
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    import torch
    deck = os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.blast2d_smr")
    par = aa.athinput.ParTable.from_file(deck)
    run = aa.config.load(deck, [], "blast")
    levels = aa.config.levels_2d(par, run)
    res = {"box": torch.cuda.get_device_name(0), "deck": "decks/athinput.blast2d_smr", "integrator": "ctu", "cour_no": run.cour_no,
           "levels": [list(g.Nx[:2]) for g in levels],
           "command": "python profiles/rate_2d_smr.py --blocks %d --steps %d --warmup %d" % (a.blocks, a.steps, a.warmup)}
    mesh = lib.Mesh(levels, 0, False).start()
    # the levels as stand-alone Grids: the same sizes and zone widths, periodic boxes of their own (nothing couples them)
    alone = []
    for g in levels:
        f = 2 ** g.level
        ov = ["job/num_domains=1", f"domain1/Nx1={g.Nx[0]}", f"domain1/Nx2={g.Nx[1]}",
              f"domain1/x1min={g.MinX[0]!r}", f"domain1/x1max={g.MinX[0] + g.Nx[0] * run.dx[0] / f!r}",
              f"domain1/x2min={g.MinX[1]!r}", f"domain1/x2max={g.MinX[1] + g.Nx[1] * run.dx[1] / f!r}"]
        s = lib.setup_problem(aa.config.slab(aa.config.load(deck, ov, "blast")), 0, False)
        s.host_initial = None
        s.start()
        alone.append(s)
    runners = [("mesh", mesh.step, mesh.lev[0].sync)] + [(f"level{l}", s.step, s.sync) for l, s in enumerate(alone)]
    for _, step, sync in runners:
        for _ in range(a.warmup):
            step()
        sync()
    t = {name: [] for name, _, _ in runners}
    for _ in range(a.blocks):
        if time.perf_counter() - t_start > a.limit:
            break
        for name, step, sync in runners:
            t0 = time.perf_counter()
            for _s in range(a.steps):
                step()
            sync()
            t[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    res["blocks_measured"] = len(t["mesh"])
    for name in t:
        res[name] = {"ms_per_step": t[name], "median_ms": statistics.median(t[name])}
    res["mesh_ms"] = res["mesh"]["median_ms"]
    res["levels_alone_sum_ms"] = sum(res[f"level{l}"]["median_ms"] for l in range(len(levels)))
    res["coupling_ms"] = res["mesh_ms"] - res["levels_alone_sum_ms"]
    if a.profile:      # the stages of every level of the mesh (the coupling kernels are booked on the Grid they write)
        for g in mesh.lev:
            g.profile_enable(True); g.profile_reset()
        for _s in range(a.steps):
            mesh.step()
        mesh.lev[0].sync()
        res["mesh_stages_ms_per_step"] = [{k: v[0] / a.steps for k, v in g.profile().items()} for g in mesh.lev]
        for g in mesh.lev:
            g.profile_enable(False)
    mesh.close()
    for s in alone:
        s.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
