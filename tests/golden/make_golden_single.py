"""Regenerates tests/golden/single_*.npz: the single-variable outputs (out = d | M1 .. cs2 | flux with x1 / x2 / x3 slices,
out_fmt = vtk | tab | pgm) of the UNMODIFIED reference executables athena_blast and athena_ioniz_sphere that oracle/Makefile.ref
builds.  par_cmdline cannot add keys, so every run gets a deck of its own in its temporary directory: the reference's deck with
its <outputN> blocks replaced by ours.  TEST INFRASTRUCTURE: needs the reference tree and oracle/_ref; the tests only read the
.npz files.

A fixture holds, for one run of the reference:
  nx, problem, nlim      the root Domain, OUR deck's name (decks/athinput.<problem>), the cycle limit
  overrides              what our deck needs on top to be that run (sizes, physics keys)
  blocks                 JSON: the <outputN> blocks of the run, {"N": {key: value}}; block 1 is always the restart dump
  paths                  every file the run left, relative to its run directory, sorted
  file_<i>               the bytes of paths[i] (uint8) unless it is a restart dump
  rst_<i>_U / _time / _dt / _ef
                         for paths[i] = *.rst: the active zones [k][j][i][6] (hydro runs) or EdgeFlux (the radiation run, whose
                         block reads nothing else), MeshS time and dt -- the state the outputs of the same number were made from
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REFBIN, read_rst      # noqa: E402

BLAST = os.path.join(REF, "tst/3D-hydro/athinput.blast")
BLAST2D = os.path.join(REF, "tst/2D-hydro/athinput.blast")
SPHERE = os.path.join(REF, "tst/massloss/athinput.ioniz_sphere_hires")


def deck_with(deck, blocks):
    txt = open(deck).read()
    txt = re.sub(r"(?ms)^<output\d+>.*?(?=^<)", "", txt)
    txt = re.sub(r"(?m)^maxout\s*=\s*\d+", "maxout = %d" % max(int(k) for k in blocks), txt, count=1)
    for n, kv in sorted(blocks.items(), key=lambda t: int(t[0])):
        txt += f"\n<output{n}>\n" + "".join(f"{k} = {v}\n" for k, v in kv.items())
    return txt


def run(name, exe, deck, problem, nx, nlim, blocks, phys=(), nscal=0, ion=False):
    tmp = tempfile.mkdtemp(prefix="golden_single_")
    try:
        rundir = os.path.join(tmp, "run")
        used = os.path.join(tmp, "athinput")
        open(used, "w").write(deck_with(deck, blocks))
        over = [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)] + [f"time/nlim={nlim}"] + list(phys)
        pr = subprocess.run([os.path.join(REFBIN, exe), "-i", used, "-d", rundir] + over, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True, errors="replace", cwd=tmp, timeout=900)
        if pr.returncode != 0:
            raise RuntimeError(pr.stdout[-2000:] + pr.stderr[-2000:])
        paths = sorted(os.path.relpath(os.path.join(dp, f), rundir) for dp, _, fs in os.walk(rundir) for f in fs)
        d = dict(nx=np.array(nx), problem=problem, nlim=nlim, overrides=np.array(over), blocks=json.dumps(blocks), paths=np.array(paths))
        for i, rel in enumerate(paths):
            p = os.path.join(rundir, rel)
            if rel.endswith(".rst"):
                g = read_rst(p, nx, nscal, ion)
                d[f"rst_{i}_time"], d[f"rst_{i}_dt"] = g["time"], g["dt"]
                if ion:                     # (the flux block reads nothing else: the state stays out, to keep the file small)
                    d[f"rst_{i}_ef"] = g["edgeflux"]
                else:
                    d[f"rst_{i}_U"] = g["U"]
            else:
                d[f"file_{i}"] = np.frombuffer(open(p, "rb").read(), dtype=np.uint8)
        out = os.path.join(HERE, name + ".npz")
        np.savez_compressed(out, **d)
        print(f"{name}: {len(paths)} files, {os.path.getsize(out)} bytes: {' '.join(paths)}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def B(fmt, out, **kw):
    d = {"out_fmt": fmt, "out": out, "id": kw.pop("id", out), "dt": "1e-9"}
    d.update(kw)
    return d


RST = {"out_fmt": "rst", "dt": "1e-9"}


def main():
    if not os.path.isdir(REF) or not os.path.isdir(REFBIN):
        sys.exit("needs the reference tree and oracle/_ref (make -C oracle ref)")
    # 16 x 12 x 8 over [-0.5, 0.5] x [-0.75, 0.75] x [-0.5, 0.5]: every kind of block; dt below a step, so every pass writes
    run("single_blast_16x12x8_s2", "athena_blast", BLAST, "blast", (16, 12, 8), 2, {
        "1": RST,
        "2": B("vtk", "d"),                                            # nothing reduced
        "3": B("vtk", "M2", x3="0.0"),                                 # a value on a zone face
        "4": B("tab", "P", x3="0.0"),
        "5": B("tab", "E", x2="0.0", x3="0.0"),                        # two slices: x1 is kept
        "6": B("pgm", "V1", x2="-0.1:0.2"),                            # a range, the image scaled by its own minimum and maximum
        "7": B("tab", "cs2", x1="-0.5", dat_fmt="%10.4e"),             # the first plane; another format
        "8": B("vtk", "V3", x2="0.7"),                                 # the last plane
        "9": B("tab", "M1", x1="0.3", x2=":"),                         # x3 is kept; a range over the whole extent
        "10": B("pgm", "d", id="miss", x3="5.0"),                      # misses the Grid: no file
    })
    # Nx1 = 67: a lane tail behind a full wave; dmin / dmax set and unset; a constant field at the first output (max_min == 0)
    run("single_blast_67x12x8_s2", "athena_blast", BLAST, "blast", (67, 12, 8), 2, {
        "1": RST,
        "2": B("vtk", "V1"),
        "3": B("vtk", "M3", x2="0.0"),
        "4": B("pgm", "P", x3="-0.2:0.1", dmin="0.05", dmax="5.0"),
        "5": B("tab", "V2", x1="0.0:0.3"),                             # x1 reduced over a range: the strided walk
        "6": B("pgm", "E", x1="0.1", dmin="0.2"),
        "7": B("tab", "M1", x1=":", x3="-0.5:-0.45"),                  # x2 is kept; a range of one zone
        "8": B("pgm", "d", x3="0.0"),
        "9": B("tab", "M3", x1="0.49", x2="-0.75:0.0", dat_fmt="%.17g"),
    })
    # a 2-D Grid: the output of ndim 2 is the Grid itself; one slice leaves a line
    run("single_blast2d_24x20_s3", "athena_blast", BLAST2D, "blast2d", (24, 20, 1), 3, {
        "1": RST,
        "2": B("vtk", "d"),
        "3": B("tab", "P", x2="0.0"),
        "4": B("tab", "M2", x1="-0.1:0.1"),
        "5": B("pgm", "E"),
        "6": B("tab", "V1"),
        "7": B("vtk", "V2", x3="0.0"),                                 # x3 on a 2-D Grid: still ndim 2, SPACING says so
        "8": B("tab", "cs2", x1=":0.0"),
    }, phys=["problem/radius=0.3"])
    # the headline problem's own block: the ionizing flux, behind ion steps
    run("single_ioniz_sphere_20x20x20_s3", "athena_ioniz_sphere", SPHERE, "ioniz_sphere", (20, 20, 20), 3, {
        "1": {"out_fmt": "rst", "dt": "1.0"},
        "2": {"usr_expr_flag": "1", "out_fmt": "vtk", "id": "flux", "out": "flux", "dt": "1.0"},
    }, phys=["job/num_domains=1"], nscal=1, ion=True)


if __name__ == "__main__":
    main()
