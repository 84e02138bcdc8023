#!/usr/bin/env python3
"""Golden fixtures for the first-order flux correction of the van Leer integrator (configure --enable-fofc:
integrate_3d_vl.c Steps 10 and 14, FixCell), from the REAL reference.

Runs only where the reference lies (like make_golden.py).  It builds the two reference executables with
FIRST_ORDER_FLUX_CORRECTION through the existing targets of oracle/Makefile.ref, runs near-vacuum hot bubbles of
prob/blast.c (its own keys damb / drat) in which the full update leaves zones with a negative density, and stores pairs of
restart states (step A just before a cycle in which the correction fires, step B after it) together with the counts the
reference printed in every cycle of the window:

    tests/golden/fofc_blast_<nx>_s<A>_s<B>.npz   UA, UB, timeA/B, dtA/B, nstepA/B, nx, overrides, counts[B-A][2] = (negd, negP),
                                                 nstepF, timeF, dtF: step, time and dt right behind the first corrected step

A window in which the reference corrected nothing fails the script: a fixture must not pin nothing.

Fixtures are DATA; no reference text is stored.

usage: python tests/golden/make_golden_fofc.py [blast] [ion]
       ion: the bounded search for an ioniz_sphere deck on which the correction fires (prints what it finds; writes nothing
       unless one fires)
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REFBIN, ROOT, read_rst      # noqa: E402

DECK = os.path.join(ROOT, "atmospheric-athena_amd", "decks", "athinput.blast_fofc")

A = ["problem/radius=0.23", "problem/drat=1e-6", "problem/prat=1e8", "problem/pamb=1e-8", "time/cour_no=0.5",
     "domain1/x1min=-0.45", "domain1/x1max=0.55", "domain1/x2min=-0.5", "domain1/x2max=0.5", "domain1/x3min=-0.6", "domain1/x3max=0.5"]
C = ["problem/radius=0.2", "problem/drat=1e-8", "problem/prat=1e10", "problem/pamb=1e-10", "time/cour_no=0.5",
     "domain1/x1min=-0.5", "domain1/x1max=0.5", "domain1/x2min=-0.5", "domain1/x2max=0.5", "domain1/x3min=-0.5", "domain1/x3max=0.5"]
# (overrides, grid, step A, step B); C's window is found by the script: up to 8 steps around its first 4-zone cycle
WINDOWS = [(A, (16, 12, 20), 28, 36), (A, (8, 8, 8), 36, 42), (C, (16, 12, 20), None, None)]


def build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-f", "Makefile.ref", "blast_vl_fofc", "ioniz_sphere_vl_fofc"],
                          stdout=subprocess.DEVNULL)


def counts_per_cycle(stdout):
    """{cycle: (negd, negP)} from the lines `cycle=N ...` and `[Step14]: %i cells had d<0; %i cells had P<0` (a step prints its
    Step14 line after the cycle line of the state it started from); and the number of `[Step10]` lines."""
    out, cur, step10 = {}, None, 0
    for tok in re.finditer(r"cycle=(\d+) |\[Step14\]: (\d+) cells had d<0; (\d+) cells had P<0|\[Step10\]", stdout):
        if tok.group(1) is not None:
            cur = int(tok.group(1))
        elif tok.group(2) is not None:
            out[cur] = (int(tok.group(2)), int(tok.group(3)))
        else:
            step10 += 1
    return out, step10


def run(cfg, deck_text, nx, nlim, extra, nscal=0, ion=False):
    """The reference on a copy of the deck that also names an rst output block (a key can only be overridden on the command
    line if the deck names it); -> (last restart state, {cycle: counts}, Step10 lines)."""
    tmp = tempfile.mkdtemp(prefix="golden_fofc_")
    deck = os.path.join(tmp, "deck")
    with open(deck, "w") as f:
        f.write(deck_text)
    rundir = os.path.join(tmp, "run")
    args = [os.path.join(REFBIN, "athena_" + cfg), "-i", deck, "-d", rundir,
            f"domain1/Nx1={nx[0]}", f"domain1/Nx2={nx[1]}", f"domain1/Nx3={nx[2]}", f"time/nlim={nlim}"] + extra
    pr = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=tmp)
    if pr.returncode != 0:
        raise RuntimeError(pr.stdout[-2000:] + pr.stderr[-2000:])
    rsts = sorted(f for f in os.listdir(rundir) if f.endswith(".rst"))
    last = read_rst(os.path.join(rundir, rsts[-1]), nx, nscal, ion)
    shutil.rmtree(tmp)
    cnt, step10 = counts_per_cycle(pr.stdout)
    return last, cnt, step10


def blast():
    deck_text = open(DECK).read() + "\n<output1>\nout_fmt = rst\ndt      = 1e300\n"
    for ov, nx, sA, sB in WINDOWS:
        extra = ["job/maxout=1"] + ov
        if sA is None:
            _, cnt, _ = run("blast_vl_fofc", deck_text, nx, 120, extra)
            first4 = min(c for c, (nd, _) in cnt.items() if nd >= 4)
            sA, sB = first4 - 3, first4 + 3
        a, _, _ = run("blast_vl_fofc", deck_text, nx, sA, extra)
        b, cnt, step10 = run("blast_vl_fofc", deck_text, nx, sB, extra)
        assert a["nstep"] == sA and b["nstep"] == sB, (a["nstep"], b["nstep"])
        counts = np.array([cnt.get(c, (0, 0)) for c in range(sA, sB)], dtype=np.int64)
        assert counts.sum() > 0, f"no first-order flux correction in cycles {sA}..{sB - 1} of {nx}: the fixture would pin nothing"
        # the state right behind the first corrected step: its dt is new_dt of the corrected zones (restart.c keeps it in full)
        sF = sA + int(np.flatnonzero(counts.sum(axis=1))[0]) + 1
        f, _, _ = run("blast_vl_fofc", deck_text, nx, sF, extra)
        assert f["nstep"] == sF
        name = f"fofc_blast_{nx[0]}x{nx[1]}x{nx[2]}_s{sA}_s{sB}"
        np.savez_compressed(os.path.join(HERE, name + ".npz"), nx=np.array(nx), UA=a["U"], nstepA=a["nstep"], timeA=a["time"], dtA=a["dt"],
                            UB=b["U"], nstepB=b["nstep"], timeB=b["time"], dtB=b["dt"], nstepF=f["nstep"], timeF=f["time"], dtF=f["dt"], counts=counts, step10=np.array(step10),
                            overrides=np.array(ov))
        print(f"{name}: t {a['time']:.6g}->{b['time']:.6g}, (negd, negP) per cycle {counts.tolist()}, [Step10] lines {step10}, "
              f"min d at B {b['U'][..., 0].min():.3e}")


def ion_search():
    """At most a dozen short runs of ioniz_sphere with first-order flux correction and a steeper planet (np, the number density at
    the planet's surface, and rp): does Step 14 ever fire?"""
    sphere = os.path.join(REF, "tst/massloss/athinput.ioniz_sphere_hires")
    deck_text = open(sphere).read()
    tries = [((20, 16, 12), []), ((32, 32, 32), []), ((20, 16, 12), ["problem/np=6.0e10"]), ((20, 16, 12), ["problem/np=6.0e12"]),
             ((32, 32, 32), ["problem/np=6.0e10"]), ((32, 32, 32), ["problem/np=6.0e12"]), ((20, 16, 12), ["problem/rp=2.1e10", "problem/np=6.0e10"]),
             ((32, 32, 32), ["problem/rp=2.1e10", "problem/np=6.0e12"]), ((24, 24, 24), ["problem/np=6.0e14"]),
             ((32, 32, 32), ["problem/np=6.0e14", "time/cour_no=0.5"]), ((36, 36, 36), ["problem/np=6.0e12", "time/cour_no=0.5"]),
             ((20, 16, 12), ["problem/np=6.0e16", "time/cour_no=0.5"])]
    fired = []
    for nx, ov in tries:
        try:
            _, cnt, step10 = run("ioniz_sphere_vl_fofc", deck_text, nx, 12, ["job/num_domains=1", "job/maxout=1", "output1/dt=1e300"] + ov, 1, True)
        except RuntimeError as e:
            print(f"ioniz_sphere {nx} {ov}: the reference stopped: {str(e).strip().splitlines()[-1][:120]}")
            continue
        print(f"ioniz_sphere {nx} {ov}: Step14 {cnt}, [Step10] lines {step10}")
        if cnt or step10:
            fired.append((nx, ov, cnt, step10))
    print("fired:", fired if fired else "none")
    return fired


if __name__ == "__main__":
    what = sys.argv[1:] or ["blast"]
    build()
    if "blast" in what:
        blast()
    if "ion" in what:
        ion_search()
