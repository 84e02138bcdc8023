#!/usr/bin/env python3
"""Golden fixtures for 2-D Grids (Nx3 = 1: integrate_2d_ctu.c / integrate_2d_vl.c), from the REAL reference.

Runs only where the reference lies (like make_golden.py).  It builds nothing new: the existing targets blast, blast_noh,
blast_vl, shk3d and sod of oracle/Makefile.ref pick the 2-D integrators by themselves on a deck with Nx3 = 1 (integrate.c:30-77).

    tests/golden/g2d_<case>_s<steps>.npz   (not _n<steps>: those names are the whole-run vectors of make_golden.py)
                                  U0 (the reference's step-0 state, active zones [1][Nx2][Nx1][5]), U, time, dt, nstep after the
                                  steps, dt0, nx, problem, integrator ("ctu" | "ctu-noh" | "vl"), overrides (for OUR deck
                                  decks/athinput.<problem>), bc (the six flags the run had)
    tests/golden/g2d_out_blast_24x20.npz   the run with <output> blocks hst + bin (cons) + vtk (prim) + rst: `paths` and the bytes
                                  of every file it left (file_<i>), blocks (JSON), overrides, tlim
    tests/golden/g2d_v3cal.npz    the calibration of the third-momentum property (see v3_calibration)

Grid sizes follow the kernels' tiles (csrc/hydro2d_kernels.hip: 64 zones along x1, T2_R - 1 = 7 rows along x2): one below, equal
to and one above either, tiny grids, three x1 tiles, and a 67 x 35 grid with dx1 != dx2.  Regenerate when the tile shape changes.

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
from make_golden import REF, REFBIN, ROOT, read_rst      # noqa: E402

BLAST2D = os.path.join(REF, "tst/2D-hydro/athinput.blast")
SOD = os.path.join(REF, "tst/1D-hydro/athinput.sod")
RST_ONLY = ["job/maxout=1", "output1/out_fmt=rst", "output1/dt=1e300"]
RST_SOD = RST_ONLY + ["output1/out=cons"]       # (that deck's first block names out = prim, which a restart dump refuses)

# the blast bubble off centre in the 1 x 1.5 box of the reference's deck, so that it lies across the periodic x1 and x2
# boundaries and across the x1 tile edges of every grid below
BOX = ["domain1/x1min=-0.8", "domain1/x1max=0.2", "domain1/x2min=-0.3", "domain1/x2max=1.2", "problem/radius=0.35"]
SIZES = [(4, 4), (5, 7), (64, 8), (63, 6), (64, 7), (65, 8), (130, 9), (67, 35)]
SIZES_08 = [(5, 7), (65, 8), (130, 9), (67, 35)]          # CTU also at the deck's own cour_no = 0.8


def build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-f", "Makefile.ref", "blast", "blast_noh", "blast_vl", "shk3d", "sod"],
                          stdout=subprocess.DEVNULL)


def run_ref(cfg, deck, nx, extra, keep_tree=False):
    tmp = tempfile.mkdtemp(prefix="golden_2d_")
    rundir = os.path.join(tmp, "run")
    args = [os.path.join(REFBIN, "athena_" + cfg), "-i", deck, "-d", rundir,
            f"domain1/Nx1={nx[0]}", f"domain1/Nx2={nx[1]}", "domain1/Nx3=1"] + extra
    pr = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace", cwd=tmp)
    if pr.returncode != 0:
        raise RuntimeError(pr.stdout[-2000:] + pr.stderr[-2000:])
    if keep_tree:
        return tmp, rundir
    rsts = sorted(f for f in os.listdir(rundir) if f.endswith(".rst"))
    n3 = (nx[0], nx[1], 1)
    first, last = read_rst(os.path.join(rundir, rsts[0]), n3, 0, False), read_rst(os.path.join(rundir, rsts[-1]), n3, 0, False)
    shutil.rmtree(tmp)
    return first, last


def save(name, first, last, nx, problem, integrator, overrides, bc):
    assert np.all(np.isfinite(last["U"])), name
    d = dict(nx=np.array([nx[0], nx[1], 1]), U0=first["U"][..., :5], U=last["U"][..., :5], nstep=last["nstep"], time=last["time"], dt=last["dt"],
             dt0=first["dt"], problem=problem, integrator=integrator, overrides=np.array(overrides), bc=np.array(bc))
    out = os.path.join(HERE, name + ".npz")
    np.savez_compressed(out, **d)
    print(f"{name}: nstep={last['nstep']} time={last['time']:.17g} dt={last['dt']:.17g} {os.path.getsize(out)} bytes")


def blast_runs():
    for cfg, integ in (("blast", "ctu"), ("blast_noh", "ctu-noh"), ("blast_vl", "vl")):
        for cour, sizes in ((0.4, SIZES), (0.8, SIZES_08 if integ != "vl" else [])):
            for n, nx in enumerate(sizes):
                nlim = 4 + n % 3
                phys = BOX + [f"time/cour_no={cour}"]
                first, last = run_ref(cfg, BLAST2D, nx, RST_ONLY + [f"time/nlim={nlim}"] + phys)
                assert np.abs(last["U"][..., 1]).max() > 0 and np.all(last["U"][..., 3] == 0.0)
                ov = [f"domain1/Nx1={nx[0]}", f"domain1/Nx2={nx[1]}"] + phys
                save(f"g2d_blast_{integ}_c{int(10*cour)}_{nx[0]}x{nx[1]}_s{nlim}", first, last, nx, "blast2d", integ, ov, (4, 4, 4, 4, 0, 0))


def shock_tubes():
    """prob/shkset1d.c along x1 and x2 on 2-D Grids: every velocity component non-zero and different on the two sides (the third
    momentum and the sweep-frame permutations), outflow along the shock, reflecting or periodic across it, both H-correction
    settings.  Our deck is decks/athinput.shkset1d."""
    vel = ["problem/v1l=0.3", "problem/v2l=-0.2", "problem/v3l=0.25", "problem/v1r=-0.1", "problem/v2r=0.15", "problem/v3r=-0.35"]
    for cfg, integ in (("shk3d", "ctu"), ("sod", "ctu-noh")):
        for d, nx in ((1, (48, 8)), (2, (8, 48))):
            for across, tag in ((1, "refl"), (4, "per")):
                a = 3 - d                                  # the direction across the shock
                bc = [0, 0, 0, 0, 0, 0]
                bc[2*(d - 1)] = bc[2*(d - 1) + 1] = 2; bc[2*(a - 1)] = bc[2*(a - 1) + 1] = across
                phys = [f"problem/shk_dir={d}", "time/cour_no=0.4"] + vel
                for e in (1, 2):
                    phys += [f"domain1/x{e}min=-0.5", f"domain1/x{e}max=0.5"]
                phys += [f"domain1/bc_ix{e}={bc[2*(e - 1)]}" for e in (1, 2)] + [f"domain1/bc_ox{e}={bc[2*(e - 1) + 1]}" for e in (1, 2)]
                first, last = run_ref(cfg, SOD, nx, RST_SOD + ["time/nlim=12"] + phys)
                assert all(np.abs(last["U"][..., c]).max() > 0 for c in (1, 2, 3))
                ov = [f"domain1/Nx1={nx[0]}", f"domain1/Nx2={nx[1]}", "domain1/Nx3=1"] + phys
                save(f"g2d_shk_{integ}_d{d}_{tag}_{nx[0]}x{nx[1]}_s12", first, last, nx, "shkset1d", integ, ov, bc)


def v3_calibration():
    """The third momentum under van Leer has no reference target (blast.c sets no velocity), so it is pinned by a property that
    is exact in real arithmetic: a uniform v3 added to a state with v3 = 0 changes nothing in d, M1, M2 and stays uniform.
    What rounding makes of it is measured on the reference itself: athena_shk3d (the 2-D CTU path) on one shock tube with
    v3 = 0 and with v3 = 0.3 on both sides."""
    nx = (48, 8)
    runs = []
    for v3 in (0.0, 0.3):
        phys = ["problem/shk_dir=1", "time/cour_no=0.4", "problem/v1l=0.3", "problem/v2l=-0.2", "problem/v1r=-0.1", "problem/v2r=0.15",
                f"problem/v3l={v3}", f"problem/v3r={v3}", "domain1/x1min=-0.5", "domain1/x1max=0.5", "domain1/x2min=-0.5", "domain1/x2max=0.5",
                "domain1/bc_ix2=4", "domain1/bc_ox2=4"]
        runs.append(run_ref("shk3d", SOD, nx, RST_SOD + ["time/nlim=12"] + phys)[1]["U"])
    a, b = runs
    d_state = max(float(np.abs(a[..., c] - b[..., c]).max() / np.abs(a[..., c]).max()) for c in (0, 1, 2))
    d_v3 = float(np.abs(b[..., 3] / b[..., 0] - 0.3).max())
    assert np.all(a[..., 3] == 0.0)
    np.savez_compressed(os.path.join(HERE, "g2d_v3cal.npz"), D_ref_state=d_state, D_ref_v3=d_v3, v3=0.3, nx=np.array([48, 8, 1]), nstep=12)
    print(f"g2d_v3cal: D_ref(d, M1, M2) = {d_state:.3e}  D_ref(M3/d - 0.3) = {d_v3:.3e}")


def output_run():
    """hst + bin (cons) + vtk (prim) + rst through the <outputN> blocks of the reference's own 2-D deck, to a short tlim"""
    nx, tlim, D = (24, 20), 0.02, 0.005
    blocks = {"1": {"out_fmt": "hst", "dt": repr(D)}, "2": {"out_fmt": "bin", "dt": repr(D)},
              "3": {"out_fmt": "vtk", "out": "prim", "dt": repr(D)}, "4": {"out_fmt": "rst", "dt": repr(2*D)}}
    phys = ["time/cour_no=0.8", f"time/tlim={tlim!r}", "problem/radius=0.3"]
    over = ["job/maxout=4", f"output1/dt={D!r}", f"output2/dt={D!r}", "output3/out_fmt=vtk", "output3/out=prim", f"output3/dt={D!r}",
            "output4/out_fmt=rst", "output4/out=cons", f"output4/dt={2*D!r}"] + phys      # (out = cons: only then is a block a dump)
    tmp, rundir = run_ref("blast", BLAST2D, nx, over, keep_tree=True)
    try:
        paths = sorted(os.path.relpath(os.path.join(dp, f), rundir) for dp, _, fs in os.walk(rundir) for f in fs)
        d = dict(nx=np.array([nx[0], nx[1], 1]), problem="blast2d", integrator="ctu", blocks=json.dumps(blocks), tlim=tlim,
                 overrides=np.array([f"domain1/Nx1={nx[0]}", f"domain1/Nx2={nx[1]}"] + phys), paths=np.array(paths))
        for i, rel in enumerate(paths):
            d[f"file_{i}"] = np.frombuffer(open(os.path.join(rundir, rel), "rb").read(), dtype=np.uint8)
        out = os.path.join(HERE, "g2d_out_blast_24x20.npz")
        np.savez_compressed(out, **d)
        print(f"g2d_out_blast_24x20: {len(paths)} files, {os.path.getsize(out)} bytes: {' '.join(paths)}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference tree")
    build()
    blast_runs()
    shock_tubes()
    v3_calibration()
    output_run()


if __name__ == "__main__":
    main()
