"""Resuming on another decomposition, and writing for one: what it costs beside the parent's path.  Same process, same box, the same
state, alternating A B A B; medians; every timed call ends in a device synchronise (the put calls wait for their last piece, the
get calls for their last copy) and includes reading / writing the files, which lie in a temporary directory (page cache: they
were written moments before).

  A  Driver.from_restart from ONE file (the parent's path: whole sections through aa_rst_section_put)
  B  Driver.from_restart(regrid=True) from the same state split NGRID = 2 x 4 x 4: 32 files, every section in 32 boxes through
     aa_rst_section_put_box
  W1 Driver.write_restart, one file;  W32 the split write (rst_ngrid = NGRID) through aa_rst_section_get_box
  with B's and W32's share that is spent inside the box calls of the library (host clock around the ctypes calls)

  python profiles/regrid_rate.py [--size 512] [--reps 3] [--ngrid 2 4 4] [--tmp DIR] [--out profiles/out/regrid_rate.json]

A record, not a bar.  B is also checked against A: the two resumed Grids hold the same bits (sections compared on the host)."""
import argparse
import importlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--ngrid", type=int, nargs=3, default=[2, 4, 4])
    ap.add_argument("--tmp", default=None, help="directory for the files (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "out", "regrid_rate.json"))
    a = ap.parse_args()
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    driver = importlib.import_module("atmospheric-athena_amd.driver")
    outputs = importlib.import_module("atmospheric-athena_amd.outputs")
    import torch
    n = a.size
    ngrid = tuple(a.ngrid)
    par = aa.athinput.ParTable.from_file(os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.ioniz_sphere"))
    par.cmdline([f"domain1/Nx{d}={n}" for d in (1, 2, 3)])
    par.blocks["job"]["maxout"] = "1"
    par.blocks["output1"] = {"out_fmt": "rst", "dt": "1e300"}
    run = aa.config.from_par(par, "ioniz_sphere")
    tmp = tempfile.mkdtemp(prefix="regrid_rate_", dir=a.tmp)
    res = {"box": torch.cuda.get_device_name(0), "host": os.uname().nodename, "size": n, "ngrid": list(ngrid),
           "command": "python profiles/regrid_rate.py --size %d --reps %d --steps %d --ngrid %d %d %d" % ((n, a.reps, a.steps) + ngrid)}
    # time inside the library's box calls
    inside = {"put": 0.0, "get": 0.0}
    put_box, get_box = lib.Grid.rst_put_box, lib.Grid.rst_get_box

    def timed_put(self, *args):
        t = time.perf_counter(); put_box(self, *args); inside["put"] += time.perf_counter() - t

    def timed_get(self, *args, **kw):
        t = time.perf_counter(); r = get_box(self, *args, **kw); inside["get"] += time.perf_counter() - t
        return r

    lib.Grid.rst_put_box, lib.Grid.rst_get_box = timed_put, timed_get
    try:
        d = driver.Driver(run, strict=False)
        d.eng.g.host_initial = None
        d.start()
        for _ in range(a.steps):
            d.step()
        one, split = os.path.join(tmp, "one"), os.path.join(tmp, "split")
        W1, W32, W32in = [], [], []
        for rep in range(a.reps + 1):                    # (the first round makes the bounce buffer and the files: not counted)
            o1 = outputs.OutputSet.from_par(par, d.time, one)
            t0 = time.perf_counter(); d.write_restart(o1.rst, o1); d.eng.sync(); t1 = time.perf_counter()
            o32 = outputs.OutputSet.from_par(par, d.time, split, rst_ngrid=ngrid)
            inside["get"] = 0.0
            t2 = time.perf_counter(); d.write_restart(o32.rst, o32); d.eng.sync(); t3 = time.perf_counter()
            if rep:
                W1.append(t1 - t0); W32.append(t3 - t2); W32in.append(inside["get"])
        p1 = os.path.join(one, o1.written[-1]); p32 = os.path.join(split, "id0", os.path.basename(p1))
        res["bytes_one_file"] = os.path.getsize(p1)
        res["bytes_split_files"] = sum(os.path.getsize(os.path.join(split, w)) for w in o32.written)
        d.eng.close(); del d
        A, B, Bin = [], [], []
        secs = None
        for rep in range(a.reps + 1):
            t0 = time.perf_counter(); ra = driver.Driver.from_restart(p1, strict=False); ra.eng.sync(); t1 = time.perf_counter()
            if rep == 0:
                secs = [ra.eng.g.rst_section(s).copy() for s in range(len(ra.eng.g.rst_sections()))]
            ra.eng.close(); del ra
            inside["put"] = 0.0
            t2 = time.perf_counter(); rb = driver.Driver.from_restart(p32, strict=False, regrid=True); rb.eng.sync(); t3 = time.perf_counter()
            if rep == 0:
                same = all(np.array_equal(rb.eng.g.rst_section(s).view(np.uint64), secs[s].view(np.uint64)) for s in range(len(secs)))
                res["B_holds_the_bits_of_A"] = bool(same)
                secs = None
            rb.eng.close(); del rb
            if rep:
                A.append(t1 - t0); B.append(t3 - t2); Bin.append(inside["put"])
        res.update({"A_from_one_file_s": A, "B_from_split_files_s": B, "B_inside_put_box_s": Bin, "W1_write_one_file_s": W1,
                    "W32_write_split_s": W32, "W32_inside_get_box_s": W32in})
        for k, v in (("A", A), ("B", B), ("B_inside", Bin), ("W1", W1), ("W32", W32), ("W32_inside", W32in)):
            res[k + "_median_s"] = statistics.median(v)
        res["B_over_A"] = res["B_median_s"] / res["A_median_s"]
        res["W32_over_W1"] = res["W32_median_s"] / res["W1_median_s"]
        res["B_payload_GBps"] = res["bytes_split_files"] / res["B_median_s"] / 1e9
        res["A_payload_GBps"] = res["bytes_one_file"] / res["A_median_s"] / 1e9
    finally:
        lib.Grid.rst_put_box, lib.Grid.rst_get_box = put_box, get_box
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
