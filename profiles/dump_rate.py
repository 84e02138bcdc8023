"""Getting a field out of the resident run: (A) Grid.download() -- all six doubles of every zone, ghost zones included, into a
pageable numpy block: the only way before the data dumps -- against (B) aa_dump_section of all sections of `vtk prim` into host
memory (single precision, active zones, made on the device in file order).  File writing excluded in both.  Same process, same
box, alternating A B A B; medians.  Then the wall time of one complete `vtk prim` dump including the file write.

  python profiles/dump_rate.py [--sizes 256 512] [--reps 3] [--file-size 512] [--out profiles/out/dump_rate.json]

Bytes alone: B moves 4*NVAR*N^3 against 8*NVAR*(N+8)^3, a factor 2*(1+8/N)^3 (2.19 at 256^3, 2.10 at 512^3).

  python profiles/dump_rate.py --overlap [--sizes 256 512] [--run-steps 24] [--every 24 2] [--rounds 3] [--variants none sync overlap]

measures what a `vtk prim` dump costs the RUN: S steps with no dump, with a synchronous dump every K steps, with an overlapped one
(OutputSet(overlap=True): device snapshot, background write) -- one process, the variants alternating, medians over the rounds.
stall per dump = (wall - wall without dumps) / dumps, the wall being the loop's; what finish() then takes (the last file still being
written, once per run) is reported beside it.  A K runs max(--run-steps, 3 K) steps.
Also: the step time while a copy or a write is in flight against the step time with none; k_dump_payload (profile scope
dump_snapshot) against the dump_section scopes of one synchronous dump; the rate of the page-locked copy.  --variants none sync
is what a checkout without the overlapped route can run: the yardstick for the synchronous figures.

  python profiles/dump_rate.py --rst [--sizes 256 512] [--run-steps 24] [--every 24 2] [--rounds 3] [--variants none sync overlap]

the same scheme for the RESTART dump (double precision, every field plus EdgeFlux: 7.5 GB at 512^3): no dump, a synchronous one every
K steps (the file as Driver.write_restart writes it: header, Grid.write_rst_payload, trailer), an overlapped one
(OutputSet(overlap_rst=True): outputs.overlapped_restart), behind one untimed warm-up pass of every variant.  Also k_rst_payload (profile scope rst_snapshot; 16 bytes per zone and
field, from the shapes) and the EdgeFlux copy (rst_snapshot_ef) against the rst_gather scopes of one synchronous payload, and begin to
ready.  --variants overlap --every (no K) measures these scopes alone: with ATHENA_AMD_VARIANT naming an experiment build of the
library (csrc/Makefile `variant`) it is how non-temporal and plain stores in k_rst_payload were compared."""
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


def rst_main(a):
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    O = importlib.import_module("atmospheric-athena_amd.outputs")
    R = importlib.import_module("atmospheric-athena_amd.restart")
    athinput = importlib.import_module("atmospheric-athena_amd.athinput")
    import torch
    res = {"box": torch.cuda.get_device_name(0), "host": os.uname().nodename, "variants": a.variants, "sizes": {},
           "library": os.environ.get("ATHENA_AMD_VARIANT", "default")}
    for n in a.sizes:
        run = aa.config.load(os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.ioniz_sphere"),
                             [f"domain1/Nx{d}={n}" for d in (1, 2, 3)], "ioniz_sphere")
        g = lib.setup_problem(aa.config.slab(run), 0, False)
        g.host_initial = None
        g.start()
        for _ in range(a.steps):
            g.step()
        g.sync()
        d = tempfile.mkdtemp(prefix="rst_rate_", dir=a.tmp)
        nzone = n ** 3
        nfield = sum(1 for label, _ in g.rst_sections() if label != "EDGEFLUX")
        payload = 8 * sum(cnt for _, cnt in g.rst_sections())
        r = {"zones": nzone, "run_steps": a.run_steps, "payload_bytes": payload, "every": {}}

        def one(variant, every, nsteps=None):
            """-> (wall of the loop, seconds finish() then took, dumps, [(step seconds, something in flight at its start)])"""
            nsteps = nsteps or max(a.run_steps, 3 * every)
            par = athinput.ParTable.from_text("<job>\nproblem_id = rate\n")
            outs = O.OutputSet(par, [], None, d, 0, 1, **({"overlap_rst": True} if variant == "overlap" else {}))
            steps, dumps = [], 0
            g.sync()
            t0 = time.perf_counter()
            for s in range(nsteps):
                if variant == "overlap":
                    outs.poll()
                if variant != "none" and s % every == 0:
                    rel = "rate.0000.rst"                                   # (one name: the disk holds one file, not every dump of the run)
                    t, dt, nstep = g.mesh_state()
                    if variant == "sync":
                        with open(outs.path(rel), "wb") as f:
                            R.write_header(f, R.par_dump(par), nstep, t, dt)
                            g.write_rst_payload(f)
                            R.write_trailer(f)
                    else:
                        assert outs.overlapped_restart([g], rel, nstep, t, dt)
                    dumps += 1
                busy = variant == "overlap" and bool(outs._pending or outs._inflight)
                t1 = time.perf_counter(); g.step(); steps.append((time.perf_counter() - t1, busy))
            g.sync()
            wall = time.perf_counter() - t0
            if variant == "overlap":
                outs.finish()
            tail = time.perf_counter() - t0 - wall
            for rel in set(outs.written):
                os.remove(os.path.join(d, rel))
            return wall, tail, dumps, steps

        # warm-up, not timed: every variant once with one dump and six steps (the first steps of a fresh process, the first touch
        # of the file and of the bounce buffer, the snapshot slot's allocation)
        r["warmup_wall_s"] = {v: one(v, 10 ** 9, 6)[0] for v in a.variants}
        for every in a.every:
            walls = {v: [] for v in a.variants}; busy, idle, tails, ndumps = [], [], [], 0
            for _ in range(a.rounds):
                for v in a.variants:
                    wall, tail, nd, steps = one(v, every)
                    walls[v].append(wall)
                    if v == "overlap":
                        busy += [t for t, b in steps if b]
                        tails.append(tail)
                    if v == "none":
                        idle += [t for t, b in steps]
                    ndumps = max(ndumps, nd)
            e = {"dumps": ndumps, "steps": max(a.run_steps, 3 * every), "wall_s": walls, "wall_median_s": {v: statistics.median(w) for v, w in walls.items()}}
            if "none" in walls:
                e["wall_none_spread_s"] = max(walls["none"]) - min(walls["none"])
                e["step_plain_median_s"] = statistics.median(idle)
                e["step_plain_min_max_s"] = [min(idle), max(idle)]
                for v in walls:
                    if v != "none":
                        e[f"stall_per_dump_{v}_s"] = (e["wall_median_s"][v] - e["wall_median_s"]["none"]) / ndumps
            if tails:
                e["finish_tail_s"] = tails                   # once per run, behind the loop: the last file still being written
            if busy:
                e["step_in_flight_median_s"] = statistics.median(busy)
                e["step_in_flight_min_max_s"] = [min(busy), max(busy)]
                e["steps_in_flight"] = len(busy)
            r["every"][str(every)] = e
            print(json.dumps({str(n): {str(every): e}}), flush=True)
        # the kernels: one synchronous payload against one snapshot, by the library's event scopes
        g.profile_enable(True); g.profile_reset()
        reps = 5
        buf = np.empty(max(cnt for _, cnt in g.rst_sections()), dtype=np.float64)
        for _ in range(reps):
            for s, (_, cnt) in enumerate(g.rst_sections()):
                g.rst_section(s, buf[:cnt])
        g.sync()
        prof = g.profile()
        r["rst_gather_scopes_ms_per_payload"] = prof["rst_gather"][0] / reps
        r["rst_gather_launches_per_payload"] = prof["rst_gather"][1] / reps
        if "overlap" in a.variants:
            nbytes = g.rst_snapshot_bytes()
            T = []
            for _ in range(reps + 1):                         # (the first one makes the buffers: left out)
                g.sync()
                t0 = time.perf_counter(); sn = g.rst_snapshot(); sn.wait(); T.append(time.perf_counter() - t0); sn.release()
                if len(T) == 1:
                    g.sync(); g.profile_reset()
            g.sync()
            prof = g.profile()
            ms = prof["rst_snapshot"][0] / reps
            ef_ms = prof["rst_snapshot_ef"][0] / reps
            r["k_rst_payload_ms"] = ms
            r["k_rst_payload_bytes_per_zone"] = 16 * nfield             # 8 read + 8 written per zone and field
            r["k_rst_payload_GBps"] = 16 * nfield * nzone / (ms * 1e-3) / 1e9
            r["edgeflux_copy_ms"] = ef_ms
            r["edgeflux_copy_GBps"] = 16 * (n + 1) ** 3 / (ef_ms * 1e-3) / 1e9
            r["snapshot_payload_bytes"] = nbytes
            r["begin_to_ready_first_s"] = T[0]
            r["begin_to_ready_s"] = T[1:]
            r["pinned_copy_GBps"] = nbytes / (statistics.median(T[1:]) - (ms + ef_ms) * 1e-3) / 1e9
        g.profile_enable(False)
        os.rmdir(d)
        res["sizes"][str(n)] = r
        print(json.dumps({str(n): r}), flush=True)
        g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


def overlap_main(a):
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    O = importlib.import_module("atmospheric-athena_amd.outputs")
    athinput = importlib.import_module("atmospheric-athena_amd.athinput")
    import torch
    res = {"box": torch.cuda.get_device_name(0), "host": os.uname().nodename, "variants": a.variants, "sizes": {}}
    for n in a.sizes:
        run = aa.config.load(os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.ioniz_sphere"),
                             [f"domain1/Nx{d}={n}" for d in (1, 2, 3)], "ioniz_sphere")
        g = lib.setup_problem(aa.config.slab(run), 0, False)
        g.host_initial = None
        g.start()
        for _ in range(a.steps):
            g.step()
        g.sync()
        d = tempfile.mkdtemp(prefix="dump_rate_", dir=a.tmp)
        r = {"zones": n ** 3, "run_steps": a.run_steps, "every": {}}

        def one(variant, every):
            """-> (wall of the loop, seconds finish() then took, dumps, [(step seconds, something in flight at its start)])"""
            nsteps = max(a.run_steps, 3 * every)
            par = athinput.ParTable.from_text("<job>\nproblem_id = rate\n")
            outs = O.OutputSet(par, [], None, d, 0, 1, **({"overlap": True} if variant == "overlap" else {}))
            steps, dumps = [], 0
            g.sync()
            t0 = time.perf_counter()
            for s in range(nsteps):
                if variant == "overlap":
                    outs.poll()
                if variant != "none" and s % every == 0:
                    rel = "rate.%04d.vtk" % (dumps % 2)                 # (two names: the disk holds two files, not every dump of the run)
                    if variant == "sync":
                        g.write_dump(outs.path(rel), "vtk", True)
                    else:
                        assert outs.overlapped_dump(g, rel, "vtk", True)
                    dumps += 1
                busy = variant == "overlap" and bool(outs._pending or outs._inflight)
                t1 = time.perf_counter(); g.step(); steps.append((time.perf_counter() - t1, busy))
            g.sync()
            wall = time.perf_counter() - t0
            if variant == "overlap":
                outs.finish()
            tail = time.perf_counter() - t0 - wall
            for rel in set(outs.written):
                os.remove(os.path.join(d, rel))
            return wall, tail, dumps, steps

        for every in a.every:
            walls = {v: [] for v in a.variants}; busy, idle, tails, ndumps = [], [], [], 0
            for _ in range(a.rounds):
                for v in a.variants:
                    wall, tail, nd, steps = one(v, every)
                    walls[v].append(wall)
                    if v == "overlap":
                        busy += [t for t, b in steps if b]
                        tails.append(tail)
                    if v == "none":
                        idle += [t for t, b in steps]
                    ndumps = max(ndumps, nd)
            e = {"dumps": ndumps, "steps": max(a.run_steps, 3 * every), "wall_s": walls, "wall_median_s": {v: statistics.median(w) for v, w in walls.items()}}
            if "none" in walls:
                e["step_plain_median_s"] = statistics.median(idle)
                e["step_plain_min_max_s"] = [min(idle), max(idle)]
                for v in walls:
                    if v != "none":
                        e[f"stall_per_dump_{v}_s"] = (e["wall_median_s"][v] - e["wall_median_s"]["none"]) / ndumps
            if tails:
                e["finish_tail_s"] = tails                   # once per run, behind the loop: the last file(s) still being written
            if busy:
                e["step_in_flight_median_s"] = statistics.median(busy)
                e["steps_in_flight"] = len(busy)
            r["every"][str(every)] = e
            print(json.dumps({str(n): {str(every): e}}), flush=True)
        # the kernels: one synchronous dump against one snapshot, by the library's event scopes
        g.profile_enable(True); g.profile_reset()
        reps = 5
        for _ in range(reps):
            for s in range(g.dump_sections("vtk")):
                g.dump_section("vtk", True, s)
        g.sync()
        prof = g.profile()
        r["dump_section_scopes_ms_per_dump"] = prof["dump_section"][0] / reps
        r["dump_section_launches_per_dump"] = prof["dump_section"][1] / reps
        if "overlap" in a.variants:
            nbytes = g.dump_snapshot_bytes("vtk")
            T = []
            for _ in range(reps):
                g.sync()
                t0 = time.perf_counter(); sn = g.dump_snapshot("vtk", True); sn.wait(); T.append(time.perf_counter() - t0); sn.release()
            g.sync()
            ms = g.profile()["dump_snapshot"][0] / reps
            r["dump_snapshot_ms"] = ms
            r["dump_snapshot_bytes_per_zone"] = 8 * g.nvar + 4 * g.nvar
            r["dump_snapshot_GBps"] = (8 * g.nvar + 4 * g.nvar) * n ** 3 / (ms * 1e-3) / 1e9
            r["snapshot_payload_bytes"] = nbytes
            r["begin_to_ready_s"] = T
            r["pinned_copy_GBps"] = nbytes / (statistics.median(T) - ms * 1e-3) / 1e9
        g.profile_enable(False)
        os.rmdir(d)
        res["sizes"][str(n)] = r
        print(json.dumps({str(n): r}), flush=True)
        g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--overlap", action="store_true", help="what a dump costs the run: none / synchronous / overlapped (see the module text)")
    ap.add_argument("--rst", action="store_true", help="the same for the restart dump: none / synchronous / overlapped (see the module text)")
    ap.add_argument("--run-steps", type=int, default=24)
    ap.add_argument("--every", type=int, nargs="*", default=[24, 2], help="a dump every K steps (one K per measurement)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variants", nargs="+", default=["none", "sync", "overlap"], choices=["none", "sync", "overlap"])
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--file-size", type=int, default=512, help="the size at which one whole dump is written to a file (0: none)")
    ap.add_argument("--tmp", default=None, help="directory for that file (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "out", "dump_rate.json"))
    a = ap.parse_args()
    if a.rst:
        return rst_main(a)
    if a.overlap:
        return overlap_main(a)
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
