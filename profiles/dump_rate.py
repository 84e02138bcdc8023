"""Getting a field out of the resident run: (A) Grid.download() -- all six doubles of every zone, ghost zones included, into a
pageable numpy block: the only way before the data dumps -- against (B) aa_dump_section of all sections of `vtk prim` into host
memory (single precision, active zones, made on the device in file order).  File writing excluded in both.  Same process, same
box, alternating A B A B; medians.  Then the wall time of one complete `vtk prim` dump including the file write.

  python profiles/dump_rate.py [--sizes 256 512] [--reps 3] [--file-size 512] [--out profiles/out/dump_rate.json]

Bytes alone: B moves 4*NVAR*N^3 against 8*NVAR*(N+8)^3, a factor 2*(1+8/N)^3 (2.19 at 256^3, 2.10 at 512^3)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--file-size", type=int, default=512, help="the size at which one whole dump is written to a file (0: none)")
    ap.add_argument("--tmp", default=None, help="directory for that file (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "out", "dump_rate.json"))
    a = ap.parse_args()
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    import torch
    res = {"box": torch.cuda.get_device_name(0), "host": os.uname().nodename, "sizes": {}}
    for n in a.sizes:
        run = aa.config.load(os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.ioniz_sphere"),
                             [f"domain1/Nx{d}={n}" for d in (1, 2, 3)], "ioniz_sphere")
        g = lib.setup_problem(aa.config.slab(run), 0, False)
        g.host_initial = None
        g.start()
        for _ in range(a.steps):
            g.step()
        nsec = g.dump_sections("vtk")
        bufs = [np.empty(int(g.L.aa_dump_section_floats(g._h, 1, s)), dtype=np.float32) for s in range(nsec)]
        for b in bufs:
            b.fill(0)                                            # touched once, as a writer's buffers are after the first dump
        A, B = [], []
        g.dump_section("vtk", True, 0, bufs[0])                  # the bounce buffer exists from the first dump on
        for _ in range(a.reps):
            t0 = time.perf_counter(); U = g.download(); t1 = time.perf_counter()
            del U
            t2 = time.perf_counter()
            for s in range(nsec):
                g.dump_section("vtk", True, s, bufs[s])
            t3 = time.perf_counter()
            A.append(t1 - t0); B.append(t3 - t2)
        bytes_a = 8 * g.nvar * (n + 8) ** 3
        bytes_b = 4 * g.nvar * n ** 3
        r = {"A_download_s": A, "B_dump_sections_s": B, "A_median_s": statistics.median(A), "B_median_s": statistics.median(B),
             "A_bytes": bytes_a, "B_bytes": bytes_b}
        r["A_GBps"] = bytes_a / r["A_median_s"] / 1e9
        r["B_GBps"] = bytes_b / r["B_median_s"] / 1e9
        r["speedup"] = r["A_median_s"] / r["B_median_s"]
        if n == a.file_size:
            d = tempfile.mkdtemp(prefix="dump_rate_", dir=a.tmp)
            p = os.path.join(d, "ioniz_sphere.0000.vtk")
            W = []
            for _ in range(2):
                t0 = time.perf_counter(); g.write_dump(p, "vtk", True); t1 = time.perf_counter()
                W.append(t1 - t0)
            r["whole_dump_with_file_write_s"] = W
            r["file_bytes"] = os.path.getsize(p)
            os.remove(p); os.rmdir(d)
            t0 = time.perf_counter(); g.step(); g.sync(); t1 = time.perf_counter()
            r["one_step_s"] = t1 - t0
        res["sizes"][str(n)] = r
        print(json.dumps({str(n): r}), flush=True)
        g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
