"""What the first-order flux correction of the van Leer integrator costs while it has nothing to correct.  Same process, same box,
two Grids of the same blast run, blocks of steps alternating A B A B ...; medians of the per-block wall time per step (the blocks
end in a synchronisation: a step's new_dt reads scalars back anyway).

  A  aa_set_fofc off: the van Leer step as it always was (the same kernels as before the switch existed)
  B  aa_set_fofc on:  + the copy of U^n in front of the predictor, the update kernel with the detection on board, one more
                      read-back of the scalars (the count of zones with d < 0: zero throughout, so nothing more is launched)

  python profiles/fofc_rate.py [--sizes 256] [--blocks 5] [--steps 10] [--out profiles/out/fofc_rate.json]

The script checks that B corrected nothing and that both Grids hold the same bits at the end."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "out", "fofc_rate.json"))
    a = ap.parse_args()
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    import torch
    res = {"box": torch.cuda.get_device_name(0), "sizes": {},
           "command": "python profiles/fofc_rate.py --sizes %s --blocks %d --steps %d" % (" ".join(str(n) for n in a.sizes), a.blocks, a.steps)}
    deck = os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.blast")
    for n in a.sizes:
        ov = [f"domain1/Nx{d}={n}" for d in (1, 2, 3)]
        grids = {}
        for key, fofc in (("A", False), ("B", True)):
            g = lib.setup_problem(aa.config.slab(aa.config.load(deck, ov, "blast", "vl", fofc=fofc)), 0, False)
            g.host_initial = None
            g.start()
            for _ in range(a.warmup):
                g.step()
            g.sync()
            grids[key] = g
        t = {"A": [], "B": []}
        fired = 0
        for _ in range(a.blocks):
            for key in ("A", "B"):
                g = grids[key]
                t0 = time.perf_counter()
                for _s in range(a.steps):
                    g.step()
                    if key == "B":
                        fired += sum(g.fofc_counts())
                g.sync()
                t[key].append((time.perf_counter() - t0) / a.steps * 1e3)
        same = bool(np.array_equal(grids["A"].rst_section(0), grids["B"].rst_section(0))) and grids["A"].dt == grids["B"].dt
        r = {"A_ms_per_step": t["A"], "B_ms_per_step": t["B"], "A_median_ms": statistics.median(t["A"]), "B_median_ms": statistics.median(t["B"]),
             "zones_corrected": int(fired), "same_density_bits_and_dt": same}
        r["B_over_A"] = r["B_median_ms"] / r["A_median_ms"]
        res["sizes"][str(n)] = r
        print(json.dumps({str(n): r}), flush=True)
        for g in grids.values():
            g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
