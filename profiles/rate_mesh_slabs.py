"""Zone-cycles per second of the 2-level deck `bench.py --smr` uses (ioniz_sphere, root nx^3 with level 1 of nx^3 zones over its
central half) as ONE Mesh and as a Mesh cut into 2 and 4 slab stacks inside the library (lib.Mesh(..., nslab=N)) -- all slabs on
ONE device, so the cut runs do the same arithmetic plus the copies: what is recorded is the overhead per cut, not a scaling
figure (there is none until a node with several GPUs is seen).  Same process, same box: warm-up, then windows of steps
alternating the nslab values (the ABAB protocol of DESIGN section 8); medians of the per-window wall time per step (a window ends
in a synchronisation).  Also the launches and copies per step of the x3 exchange of all levels: the batched form as counted by the
library (aa_mesh_halo_counts), the per-level form (AA_MESH_HALO_BATCH=0) as the levels' own kernels would issue them.

  python profiles/rate_mesh_slabs.py [--nx 320] [--windows 3] [--steps 6] [--warmup 3] [--limit 400] [--out profiles/out/rate_mesh_slabs.json]

--limit: one time limit in seconds for the whole measurement (checked between windows; what was measured until then is kept)."""
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
    ap.add_argument("--nx", type=int, default=320)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=float, default=400.0)
    ap.add_argument("--nslab", default="1,2,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "out", "rate_mesh_slabs.json"))
    a = ap.parse_args()
    t_start = time.perf_counter()
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    import torch
    nx = a.nx
    deck = os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.ioniz_sphere")
    par = aa.athinput.ParTable.from_file(deck)
    par.cmdline(["job/num_domains=2", f"domain1/Nx1={nx}", f"domain1/Nx2={nx}", f"domain1/Nx3={nx}",
                 f"domain2/Nx1={nx}", f"domain2/Nx2={nx}", f"domain2/Nx3={nx}",
                 f"domain2/iDisp={nx // 2}", f"domain2/jDisp={nx // 2}", f"domain2/kDisp={nx // 2}"])
    run = aa.config.from_par(par, "ioniz_sphere")
    levels = aa.config.levels(par, run)
    zones = sum(g.Nx[0] * g.Nx[1] * g.Nx[2] for g in levels)
    settings = [int(n) for n in a.nslab.split(",")]
    res = {"box": torch.cuda.get_device_name(0), "devices_used": 1, "deck": f"ioniz_sphere 2-level SMR, {nx}^3 + {nx}^3 (bench.py --smr --nx {nx})",
           "zones": zones, "build": "default", "command": "python profiles/rate_mesh_slabs.py --nx %d --windows %d --steps %d --warmup %d" %
           (nx, a.windows, a.steps, a.warmup),
           "note": "all slabs on ONE device: overhead per cut, no scaling figure"}
    meshes = {}
    for n in settings:
        m = lib.Mesh(levels, 0, False, nslab=n) if n > 1 else lib.Mesh(levels, 0, False)
        for g in m.lev:
            g.host_initial = None
        m.start()
        for _ in range(a.warmup):
            m.step()
        m.lev[0].sync()
        meshes[n] = m
    t = {n: [] for n in settings}
    c0 = {n: meshes[n].halo_counts() for n in settings}
    steps_done = 0
    for _ in range(a.windows):
        if time.perf_counter() - t_start > a.limit:
            break
        for n in settings:
            m = meshes[n]
            t0 = time.perf_counter()
            for _s in range(a.steps):
                m.step()
            m.lev[0].sync()
            t[n].append((time.perf_counter() - t0) / a.steps * 1e3)
        steps_done += a.steps
    res["windows_measured"] = len(t[settings[0]])
    for n in settings:
        ms = statistics.median(t[n])
        entry = {"ms_per_step": t[n], "median_ms": ms, "zone_cycles_per_s": zones / (ms * 1e-3), "cuts": meshes[n].cuts}
        if n > 1:
            c1 = meshes[n].halo_counts()
            ex = (c1[2] - c0[n][2]) / steps_done
            entry["exchanges_of_all_levels_per_step"] = ex
            entry["batched"] = {"launches_per_step": (c1[0] - c0[n][0]) / steps_done, "copies_per_step": (c1[1] - c0[n][1]) / steps_done}
            sides = sum((g.lx3 >= 0) + (g.rx3 >= 0) for r in range(n) for g in aa.config.mesh_slabs(par, run, r, n, meshes[n].cuts).levels)
            entry["per_level"] = {"launches_per_step": 2 * sides * ex, "copies_per_step": sides * ex}      # pack + unpack per side of every piece
            entry["slower_than_one_mesh"] = ms / statistics.median(t[settings[0]]) - 1.0 if settings[0] == 1 else None
        res[f"nslab{n}"] = entry
    for m in meshes.values():
        m.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
