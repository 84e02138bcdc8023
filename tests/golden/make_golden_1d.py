#!/usr/bin/env python3
"""Golden fixtures for 1-D Grids (Nx2 = Nx3 = 1: integrate_1d_ctu.c / integrate_1d_vl.c), from the REAL reference.

Runs only where the reference lies (like make_golden.py).  It builds nothing new: the existing targets sod, shk3d, blast_vl,
blast_ppm and blast_vl_ppm of oracle/Makefile.ref pick the 1-D integrators by themselves on a deck with Nx2 = Nx3 = 1
(integrate.c:30-47).

    tests/golden/g1d_<case>_s<steps>.npz   U0 (the reference's step-0 state, active zones [1][1][Nx1][5]), U, time, dt, nstep after the
                                  steps, dt0, nx, problem, integrator ("ctu" | "ctu-noh" | "vl"), order (2 | 3), overrides (for OUR
                                  deck decks/athinput.<sod1d | blast1d>), bc (the six flags the run had)
    tests/golden/g1d_sod_full.npz the reference's own tst/1D-hydro/athinput.sod (root Domain) to tlim: U0, U and `times`, `dts`:
                                  MeshS.time and dt after every step, from a restart dump per step
    tests/golden/g1d_out_sod_24.npz  that deck at 24 zones with <output> blocks hst + vtk (prim) + bin (cons) + rst: `paths` and
                                  the bytes of every file it left (file_<i>), blocks (JSON), overrides, tlim
    tests/golden/g1d_out_sod_24_x2.npz  the same in a root Domain of 1 x 2 x 1.5 (the deck's is 1 x 1 x 1)

Grid sizes follow the kernels (csrc/hydro1d_kernels.hip): B = 248 active zones per block of k1d_step, R = 1272 zones the resident
kernel keeps -- 4, 5, B - 1, B, B + 1, 3B + 2, R and R + 1.  Regenerate when either changes.

The 1-D CTU integrator has no H-correction: sod (built without) and shk3d (built with) must give the same bits.  That is
asserted here on every shock tube of the set, and one case is stored under both integrator names.

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
EINFELDT = os.path.join(REF, "tst/1D-hydro/athinput.einfeldt1125")
ONE_DOMAIN = ["job/num_domains=1"]
RST_ONLY = ["job/maxout=1", "output1/out_fmt=rst", "output1/dt=1e300"]
RST_SOD = RST_ONLY + ["output1/out=cons"]       # (that deck's first block names out = prim, which a restart dump refuses)

B, R = 248, 1272
VEL = ["problem/v1l=0.3", "problem/v2l=-0.2", "problem/v3l=0.25", "problem/v1r=-0.1", "problem/v2r=0.15", "problem/v3r=-0.35"]
# the blast slab off centre, so that it lies across the periodic x1 boundary and across the block edges of the grids below
BOX = ["domain1/x1min=-0.8", "domain1/x1max=0.2", "problem/radius=0.35"]


def build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-f", "Makefile.ref", "sod", "shk3d", "blast_vl", "blast_ppm", "blast_vl_ppm"],
                          stdout=subprocess.DEVNULL)


def run_ref(cfg, deck, n, extra, keep_tree=False, every_step=False):
    tmp = tempfile.mkdtemp(prefix="golden_1d_")
    rundir = os.path.join(tmp, "run")
    args = [os.path.join(REFBIN, "athena_" + cfg), "-i", deck, "-d", rundir,
            f"domain1/Nx1={n}", "domain1/Nx2=1", "domain1/Nx3=1"] + ONE_DOMAIN + extra
    pr = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace", cwd=tmp)
    if pr.returncode != 0:
        raise RuntimeError(pr.stdout[-2000:] + pr.stderr[-2000:])
    if keep_tree:
        return tmp, rundir
    rsts = sorted(f for f in os.listdir(rundir) if f.endswith(".rst"))
    n3 = (n, 1, 1)
    if every_step:
        out = [read_rst(os.path.join(rundir, f), n3, 0, False) for f in rsts]
    else:
        out = read_rst(os.path.join(rundir, rsts[0]), n3, 0, False), read_rst(os.path.join(rundir, rsts[-1]), n3, 0, False)
    shutil.rmtree(tmp)
    return out


def save(name, first, last, n, problem, integrator, order, overrides, bc, **more):
    assert np.all(np.isfinite(last["U"])), name
    d = dict(nx=np.array([n, 1, 1]), U0=first["U"][..., :5], U=last["U"][..., :5], nstep=last["nstep"], time=last["time"], dt=last["dt"],
             dt0=first["dt"], problem=problem, integrator=integrator, order=order, overrides=np.array(overrides), bc=np.array(bc), **more)
    assert d["U"].shape == (1, 1, n, 5), d["U"].shape
    out = os.path.join(HERE, name + ".npz")
    np.savez_compressed(out, **d)
    print(f"{name}: nstep={last['nstep']} time={last['time']:.17g} dt={last['dt']:.17g} {os.path.getsize(out)} bytes")


def same(a, b):
    return np.array_equal(a["U"], b["U"]) and a["time"] == b["time"] and a["dt"] == b["dt"] and a["nstep"] == b["nstep"]


def shock_tubes():
    """prob/shkset1d.c on 1-D Grids: every velocity component non-zero and different on the two sides, outflow, reflecting and
    periodic ends, cour_no 0.8 (legal with the 1-D CTU integrator) and 0.4, every size class.  Our deck is decks/athinput.sod1d."""
    cases = [(4, 2, 0.4, 4), (5, 1, 0.8, 5), (B - 1, 4, 0.8, 6), (B, 2, 0.8, 12), (B + 1, 1, 0.4, 8), (3*B + 2, 4, 0.8, 7),
             (R, 2, 0.8, 6), (R + 1, 1, 0.8, 6), (130, 2, 0.4, 9)]
    for k, (n, bc, cour, nlim) in enumerate(cases):
        phys = [f"time/cour_no={cour}", "time/tlim=10.0", f"domain1/bc_ix1={bc}", f"domain1/bc_ox1={bc}"] + VEL
        first, last = run_ref("sod", SOD, n, RST_SOD + [f"time/nlim={nlim}"] + phys)
        f3, l3 = run_ref("shk3d", SOD, n, RST_SOD + [f"time/nlim={nlim}"] + phys)
        # a finding if it ever fails: integrate_1d_ctu.c would then depend on H_CORRECTION
        assert same(first, f3) and same(last, l3), f"sod and shk3d differ on a 1-D Grid of {n} zones"
        assert all(np.abs(last["U"][..., c]).max() > 0 for c in (1, 2, 3)) and last["nstep"] == nlim
        ov = [f"domain1/Nx1={n}"] + phys
        tag = f"bc{bc}_c{int(10*cour)}_{n}_s{nlim}"
        save(f"g1d_shk_ctu-noh_{tag}", first, last, n, "sod1d", "ctu-noh", 2, ov, (bc, bc, 0, 0, 0, 0))
        if k == 3:
            save(f"g1d_shk_ctu_{tag}", f3, l3, n, "sod1d", "ctu", 2, ov, (bc, bc, 0, 0, 0, 0))
    # the strong double rarefaction of tst/1D-hydro/athinput.einfeldt1125: the Roe solver's fallback
    from importlib import import_module
    sys.path.insert(0, ROOT)
    P = import_module("atmospheric-athena_amd.athinput").ParTable.from_file(EINFELDT)
    phys = [f"problem/{k}={P.gets('problem', k)}" for k in ("gamma", "dl", "pl", "v1l", "v2l", "v3l", "dr", "pr", "v1r", "v2r", "v3r")]
    phys += [f"time/cour_no={P.gets('time', 'cour_no')}"]
    first, last = run_ref("sod", EINFELDT, 128, RST_SOD + ["time/nlim=10"])
    save("g1d_shk_ctu-noh_einfeldt1125_128_s10", first, last, 128, "sod1d", "ctu-noh", 2, ["domain1/Nx1=128"] + phys, (2, 2, 0, 0, 0, 0))


def blast_runs():
    """prob/blast.c with Nx2 = Nx3 = 1 (the over-pressured region is a slab): the van Leer integrator at second and third order,
    CTU at third order (blast_ppm is built with H-correction, which the 1-D integrator does not have).  Our deck: decks/athinput.blast1d."""
    for cfg, integ, order, cours in (("blast_vl", "vl", 2, (0.4,)), ("blast_vl_ppm", "vl", 3, (0.4,)), ("blast_ppm", "ctu", 3, (0.4, 0.8))):
        for cour in cours:
            for n in (4, 65, B + 1, 300) + ((R,) if cour == 0.4 else ()):
                phys = BOX + [f"time/cour_no={cour}"]
                first, last = run_ref(cfg, BLAST2D, n, RST_ONLY + ["time/nlim=6"] + phys)
                assert np.abs(last["U"][..., 1]).max() > 0 and np.all(last["U"][..., 2:4] == 0.0)
                save(f"g1d_blast_{integ}_o{order}_c{int(10*cour)}_{n}_s6", first, last, n, "blast1d", integ, order,
                     [f"domain1/Nx1={n}"] + phys, (4, 4, 0, 0, 0, 0))


def sod_full():
    """the reference's deck as it is (root Domain), a restart dump behind every step: 87 steps, the last dt clipped at tlim"""
    steps = run_ref("sod", SOD, 128, ["job/maxout=1", "output1/out_fmt=rst", "output1/out=cons", "output1/dt=1e-12"], every_step=True)
    # (the forced dump after the loop repeats the last state under the next number)
    seen, uniq = set(), []
    for s in steps:
        if s["nstep"] not in seen:
            seen.add(s["nstep"]); uniq.append(s)
    assert [s["nstep"] for s in uniq] == list(range(len(uniq)))
    first, last = uniq[0], uniq[-1]
    save("g1d_sod_full", first, last, 128, "sod1d", "ctu-noh", 2, [], (2, 2, 0, 0, 0, 0),
         times=np.array([s["time"] for s in uniq[1:]]), dts=np.array([s["dt"] for s in uniq[1:]]), tlim=0.25)


def output_run(name="g1d_out_sod_24", extent=()):
    """hst + vtk (prim) + bin (cons) + rst at 24 zones to tlim.  The reference's own deck has two <output> blocks and its command
    line cannot add keys, so the run reads OUR deck decks/athinput.sod1d (the same <time>, <domain1> and <problem> values, four
    blocks).  `extent`: overrides of the x2 / x3 edges -- the deck's are 0 .. 1 along all three, which cannot tell the x1 extent
    from the volume, nor a zone's dx2 = 1 from the root's x2 extent."""
    n = 24
    deck = os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.sod1d")
    blocks = {"1": {"out_fmt": "hst", "dt": "0.05"}, "2": {"out_fmt": "vtk", "out": "prim", "dt": "0.1"},
              "3": {"out_fmt": "bin", "dt": "0.1"}, "4": {"out_fmt": "rst", "dt": "0.1"}}
    over = ["job/maxout=4", "output1/dt=0.05", "output2/dt=0.1", "output3/dt=0.1", "output4/dt=0.1"]
    tmp, rundir = run_ref("sod", deck, n, over + list(extent), keep_tree=True)
    try:
        paths = sorted(os.path.relpath(os.path.join(dp, f), rundir) for dp, _, fs in os.walk(rundir) for f in fs)
        d = dict(nx=np.array([n, 1, 1]), problem="sod1d", integrator="ctu-noh", order=2, blocks=json.dumps(blocks), tlim=0.25,
                 overrides=np.array([f"domain1/Nx1={n}"] + list(extent)), paths=np.array(paths))
        for i, rel in enumerate(paths):
            d[f"file_{i}"] = np.frombuffer(open(os.path.join(rundir, rel), "rb").read(), dtype=np.uint8)
        out = os.path.join(HERE, name + ".npz")
        np.savez_compressed(out, **d)
        print(f"{name}: {len(paths)} files, {os.path.getsize(out)} bytes: {' '.join(paths)}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def output_run_extents():
    """the same run in a root Domain of 1 x 2 x 1.5: init_mesh.c:331-337 gives the zones dx2 = 2, dx3 = 1.5 (vtk SPACING, ORIGIN;
    dump_history.c:174-177 multiplies them into every zone's dVol), dump_history.c:316-321 divides by the x1 extent alone"""
    output_run("g1d_out_sod_24_x2", ["domain1/x2max=2.0", "domain1/x3min=-0.5", "domain1/x3max=1.0"])


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference tree")
    build()
    only = sys.argv[1:]
    for f in (shock_tubes, blast_runs, sod_full, output_run, output_run_extents):
        if not only or f.__name__ in only:
            f()


if __name__ == "__main__":
    main()
