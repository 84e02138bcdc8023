#!/usr/bin/env python3
"""Golden fixtures for static mesh refinement on 2-D Grids (Nx3 = 1), from the REAL reference.

Runs only where the reference lies (like make_golden_2d.py).  It builds nothing new: the targets blast_smr (CTU + H-correction)
and blast_smr_vl of oracle/Makefile.ref pick the 2-D integrators by themselves on a deck with Nx3 = 1, and the reference's own
tst/2D-hydro/athinput.blast carries three <domainN> blocks.

    tests/golden/g2dsmr_<case>_<ctu|vl>_s<steps>.npz
        nlevels, nxs [nlevels][3], levels (DomainS.Level of every Grid), disp, U0_<l> / U_<l> (active zones [1][Nx2][Nx1][5] of Grid l
        at step 0 and after the steps; Grids level by level from the root, deck order inside a level), time, dt, dt0, nstep,
        integrator, overrides (for OUR deck decks/athinput.blast2d_smr), bc (the root's six flags)
    tests/golden/g2dsmr_out_A.npz       case A with <output> blocks hst + bin (cons) + vtk (prim) + rst to a short tlim: `paths` and the
                                        bytes of every file it left (file_<i>), lev1/ and lev2/ included; blocks (JSON), overrides, tlim
    tests/golden/g2dsmr_restart_A_<ctu|vl>.npz  case A's restart dump after 4 steps (seed: the file's bytes) and the state the reference reaches
                                        from it with -r at step 8

cour_no is 0.8 with CTU (the deck's own) and 0.4 with van Leer.  The cases follow the kernels' tiles (csrc/hydro2d_kernels.hip: 64
zones along x1, 7 rows along x2) and the coupling kernels' sides (csrc/smr.hip): see CASES.  Regenerate when the tile shape changes.

Fixtures are DATA; no reference text is stored.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REFBIN, ROOT, read_rst_levels      # noqa: E402

BLAST2D = os.path.join(REF, "tst/2D-hydro/athinput.blast")
RST_ONLY = ["job/maxout=1", "output1/out_fmt=rst", "output1/dt=1e300"]
INTEG = (("blast_smr", "ctu", 0.8), ("blast_smr_vl", "vl", 0.4))
OUTFLOW = [f"domain1/bc_{s}x{d}=2" for d in (1, 2) for s in "io"]


def dom(n, nx, disp=None, level=None):
    o = [f"domain{n}/Nx1={nx[0]}", f"domain{n}/Nx2={nx[1]}", f"domain{n}/Nx3=1"]
    if level is not None:
        o.append(f"domain{n}/level={level}")
    if disp:
        o += [f"domain{n}/iDisp={disp[0]}", f"domain{n}/jDisp={disp[1]}", f"domain{n}/kDisp=0"]
    return o


# name: (Grids [(level, Nx, Disp)], extra overrides, step counts, the root must differ from the unrefined run outside the children)
CASES = {
    # three levels, periodic root
    "A": ([(0, (32, 24), None), (1, (24, 16), (16, 12)), (2, (16, 16), (40, 32))], ["problem/radius=0.3"], (8, 1), True),
    # a child on the root boundary: no prolongation or correction on that side
    "B": ([(0, (32, 24), None), (1, (24, 16), (0, 12))],
          ["problem/radius=0.3", "domain1/x1min=-0.2", "domain1/x1max=0.8"] + OUTFLOW, (8,), False),
    # a child of three x1 tiles and three row tiles
    "C": ([(0, (80, 16), None), (1, (136, 16), (12, 8))], ["problem/radius=0.25"], (6,), True),
    # two Domains on one level, a few root zones apart
    "D": ([(0, (40, 24), None), (1, (16, 16), (12, 16)), (1, (20, 16), (44, 16))], ["problem/radius=0.3"], (8,), True),
    # outline on the parent's faces is+64 (tile-edge path) and is+96, rows 7 and 14 (row-tile edges), bubble across the outline
    "E": ([(0, (136, 16), None), (1, (64, 14), (128, 14))],
          ["problem/radius=0.25", "domain1/x1min=-0.8", "domain1/x1max=0.9"], (6,), True),
}


def overrides(grids, extra, cour):
    o = [f"job/num_domains={len(grids)}"]
    for n, (lev, nx, disp) in enumerate(grids, 1):
        o += dom(n, nx, disp, lev)
    return o + extra + [f"time/cour_no={cour}"]


def build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-f", "Makefile.ref", "blast_smr", "blast_smr_vl"], stdout=subprocess.DEVNULL)


def run_ref(cfg, args, keep_tree=False, restart=None):
    tmp = tempfile.mkdtemp(prefix="golden_2dsmr_")
    rundir = os.path.join(tmp, "run")
    head = ["-r", restart] if restart else ["-i", BLAST2D]
    pr = subprocess.run([os.path.join(REFBIN, "athena_" + cfg)] + head + ["-d", rundir] + args,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace", cwd=tmp)
    if pr.returncode != 0:
        raise RuntimeError(pr.stdout[-2000:] + pr.stderr[-2000:])
    return tmp, rundir


def rst_pair(cfg, args, nxs):
    tmp, rundir = run_ref(cfg, RST_ONLY + args)
    rsts = sorted(f for f in os.listdir(rundir) if f.endswith(".rst"))
    first, last = (read_rst_levels(os.path.join(rundir, r), nxs, 0, False) for r in (rsts[0], rsts[-1]))
    shutil.rmtree(tmp)
    return first, last


def step_cases():
    for cfg, integ, cour in INTEG:
        for case, (grids, extra, counts, differs) in CASES.items():
            nxs = [(nx[0], nx[1], 1) for _, nx, _ in grids]
            ov = overrides(grids, extra, cour)
            for nlim in counts:
                first, last = rst_pair(cfg, ov + [f"time/nlim={nlim}"], nxs)
                name = f"g2dsmr_{case}_{integ}_s{nlim}"
                d = dict(nlevels=len(grids), nxs=np.array(nxs), levels=np.array([g[0] for g in grids]),
                         disp=np.array([(g[2] or (0, 0)) + (0,) for g in grids]), nstep=last["nstep"], time=last["time"], dt=last["dt"],
                         dt0=first["dt"], integrator=integ, problem="blast2d_smr", overrides=np.array(ov),
                         bc=np.array([2, 2, 2, 2, 0, 0] if extra[-1] in OUTFLOW else [4, 4, 4, 4, 0, 0]))
                for l, ((U0, _), (U, _)) in enumerate(zip(first["levels"], last["levels"])):
                    assert np.all(np.isfinite(U)), (name, l)
                    assert np.abs(U[..., 1]).max() > 0 and np.abs(U[..., 2]).max() > 0 and np.all(U[..., 3] == 0.0), (name, l)
                    d[f"U0_{l}"], d[f"U_{l}"] = U0[..., :5], U[..., :5]
                assert last["nstep"] == nlim
                if differs:      # the flux correction and prolongation act: the root is not the unrefined run's outside the children
                    one = ["job/num_domains=1"] + dom(1, grids[0][1]) + extra + [f"time/cour_no={cour}", f"time/nlim={nlim}"]
                    _, flat = rst_pair(cfg, one, nxs[:1])
                    out = np.ones(nxs[0][1::-1], dtype=bool)
                    for lev, nx, disp in grids[1:]:
                        f = 2 ** lev
                        out[disp[1] // f:(disp[1] + nx[1]) // f, disp[0] // f:(disp[0] + nx[0]) // f] = False
                    nz = int((np.any(last["levels"][0][0][0] != flat["levels"][0][0][0], axis=-1) & out).sum())
                    assert nz > 0, name
                    d["root_zones_changed_outside"] = nz
                out_path = os.path.join(HERE, name + ".npz")
                np.savez_compressed(out_path, **d)
                print(f"{name}: nstep={last['nstep']} time={last['time']:.17g} dt={last['dt']:.17g} {os.path.getsize(out_path)} bytes"
                      f" changed outside: {d.get('root_zones_changed_outside', '-')}")


def output_run():
    """hst + bin (cons) + vtk (prim) + rst through <outputN> blocks on case A, to a short tlim"""
    grids, extra, _, _ = CASES["A"]
    tlim, D = 0.01, 0.005
    blocks = {"1": {"out_fmt": "hst", "dt": repr(D)}, "2": {"out_fmt": "bin", "dt": repr(D)},
              "3": {"out_fmt": "vtk", "out": "prim", "dt": repr(D)}, "4": {"out_fmt": "rst", "dt": repr(2*D)}}
    phys = overrides(grids, extra, 0.8) + [f"time/tlim={tlim!r}"]
    over = ["job/maxout=4", f"output1/dt={D!r}", f"output2/dt={D!r}", "output3/out_fmt=vtk", "output3/out=prim", f"output3/dt={D!r}",
            "output4/out_fmt=rst", "output4/out=cons", f"output4/dt={2*D!r}"] + phys
    tmp, rundir = run_ref("blast_smr", over)
    try:
        paths = sorted(os.path.relpath(os.path.join(dp, f), rundir) for dp, _, fs in os.walk(rundir) for f in fs)
        assert any(p.startswith("lev1/") for p in paths) and any(p.startswith("lev2/") for p in paths), paths
        d = dict(nxs=np.array([(nx[0], nx[1], 1) for _, nx, _ in grids]), problem="blast2d_smr", integrator="ctu", blocks=json.dumps(blocks),
                 tlim=tlim, overrides=np.array(phys), paths=np.array(paths))
        for i, rel in enumerate(paths):
            d[f"file_{i}"] = np.frombuffer(open(os.path.join(rundir, rel), "rb").read(), dtype=np.uint8)
        out = os.path.join(HERE, "g2dsmr_out_A.npz")
        np.savez_compressed(out, **d)
        print(f"g2dsmr_out_A: {len(paths)} files, {os.path.getsize(out)} bytes: {' '.join(paths)}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def restart_pair():
    """case A: the reference's dump after 4 steps, and where the reference arrives from it (-r) at step 8"""
    grids, extra, _, _ = CASES["A"]
    nxs = [(nx[0], nx[1], 1) for _, nx, _ in grids]
    for cfg, integ, cour in INTEG:
        ov = overrides(grids, extra, cour)
        tmp, rundir = run_ref(cfg, RST_ONLY + ov + ["time/nlim=4"])
        try:
            seed = os.path.join(rundir, sorted(f for f in os.listdir(rundir) if f.endswith(".rst"))[-1])
            seed_bytes = open(seed, "rb").read()
            tmp2, rundir2 = run_ref(cfg, ["time/nlim=8"], restart=seed)
            try:
                last = read_rst_levels(os.path.join(rundir2, sorted(f for f in os.listdir(rundir2) if f.endswith(".rst"))[-1]), nxs, 0, False)
            finally:
                shutil.rmtree(tmp2, ignore_errors=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        assert last["nstep"] == 8
        d = dict(nlevels=len(grids), nxs=np.array(nxs), integrator=integ, overrides=np.array(ov), seed=np.frombuffer(seed_bytes, dtype=np.uint8),
                 nstep=last["nstep"], time=last["time"], dt=last["dt"])
        for l, (U, _) in enumerate(last["levels"]):
            assert np.all(np.isfinite(U))
            d[f"U_{l}"] = U[..., :5]
        out = os.path.join(HERE, f"g2dsmr_restart_A_{integ}.npz")
        np.savez_compressed(out, **d)
        print(f"g2dsmr_restart_A_{integ}: seed {len(seed_bytes)} bytes, nstep={last['nstep']} time={last['time']:.17g} {os.path.getsize(out)} bytes")


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference tree")
    build()
    what = sys.argv[1:] or ["steps", "out", "restart"]
    if "steps" in what:
        step_cases()
    if "out" in what:
        output_run()
    if "restart" in what:
        restart_pair()


if __name__ == "__main__":
    main()
