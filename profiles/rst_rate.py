"""The payload of a restart dump out of (and into) the resident run.  Same process, same box, alternating A B A B A B; medians.
File writing excluded everywhere.

  A  the way before the section calls: Grid.download() -- all six doubles of every zone, ghost zones included, into a fresh pageable
     block -- plus the six strided gathers np.ascontiguousarray(U[4:-4, 4:-4, 4:-4, c]) restart.write_rst takes out of it
  B  all sections through Grid.rst_section into host arrays that were touched once before (csrc/restart.hip)
  C  the yardstick of the pipeline in the same run: all sections of `vtk prim` through Grid.dump_section (profiles/dump_rate.py's B)
  R  all sections through Grid.put_rst_section (no bar)

  python profiles/rst_rate.py [--sizes 256 512] [--reps 3] [--out profiles/out/rst_rate.json]

Bars: B faster than A at every size; B's payload rate at least 0.8 x C's of the same run."""
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "out", "rst_rate.json"))
    a = ap.parse_args()
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    import torch
    res = {"box": torch.cuda.get_device_name(0), "sizes": {},
           "command": "python profiles/rst_rate.py --sizes %s --reps %d --steps %d" % (" ".join(str(n) for n in a.sizes), a.reps, a.steps)}
    for n in a.sizes:
        run = aa.config.load(os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.ioniz_sphere"),
                             [f"domain1/Nx{d}={n}" for d in (1, 2, 3)], "ioniz_sphere")
        g = lib.setup_problem(aa.config.slab(run), 0, False)
        g.host_initial = None
        g.start()
        for _ in range(a.steps):
            g.step()
        secs = g.rst_sections()
        bufs = [np.zeros(cnt, dtype=np.float64) for _label, cnt in secs]              # touched once
        nvtk = g.dump_sections("vtk")
        vbufs = [np.zeros(int(g.L.aa_dump_section_floats(g._h, 1, s)), dtype=np.float32) for s in range(nvtk)]
        g.dump_section("vtk", True, 0, vbufs[0])                                       # the bounce buffer exists from here on
        g.rst_section(0, bufs[0])
        A, B, Cc, R = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            U = g.download()
            cols = [np.ascontiguousarray(U[4:-4, 4:-4, 4:-4, c]) for c in range(g.nvar)]
            t1 = time.perf_counter()
            del U, cols
            t2 = time.perf_counter()
            for s in range(len(secs)):
                g.rst_section(s, bufs[s])
            t3 = time.perf_counter()
            for s in range(nvtk):
                g.dump_section("vtk", True, s, vbufs[s])
            t4 = time.perf_counter()
            for s in range(len(secs)):
                g.put_rst_section(s, bufs[s])
            t5 = time.perf_counter()
            A.append(t1 - t0); B.append(t3 - t2); Cc.append(t4 - t3); R.append(t5 - t4)
        bytes_b = 8 * sum(cnt for _l, cnt in secs)
        bytes_c = 4 * sum(v.size for v in vbufs)
        r = {"A_download_and_gathers_s": A, "B_rst_sections_s": B, "C_vtk_prim_sections_s": Cc, "R_put_rst_sections_s": R,
             "A_bytes_over_the_link": 8 * g.nvar * (n + 8) ** 3, "B_bytes": bytes_b, "C_bytes": bytes_c}
        for k, v in (("A", A), ("B", B), ("C", Cc), ("R", R)):
            r[k + "_median_s"] = statistics.median(v)
        r["B_GBps"] = bytes_b / r["B_median_s"] / 1e9
        r["C_GBps"] = bytes_c / r["C_median_s"] / 1e9
        r["R_GBps"] = bytes_b / r["R_median_s"] / 1e9
        r["A_over_B"] = r["A_median_s"] / r["B_median_s"]
        r["B_rate_over_C_rate"] = r["B_GBps"] / r["C_GBps"]
        r["bar_B_faster_than_A"] = bool(r["B_median_s"] < r["A_median_s"])
        r["bar_B_rate_at_least_0.8_C"] = bool(r["B_rate_over_C_rate"] >= 0.8)
        res["sizes"][str(n)] = r
        print(json.dumps({str(n): r}), flush=True)
        g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
