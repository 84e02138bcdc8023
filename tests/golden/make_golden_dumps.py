"""Regenerates tests/golden/dump_*.npz: the vtk / bin data dumps (and the restart dumps beside them) of the UNMODIFIED reference
executables oracle/Makefile.ref builds, driven through the <outputN> blocks of the reference's own decks by command-line
overrides.  TEST INFRASTRUCTURE: needs the reference tree and oracle/_ref; the tests only read the .npz files.
(Names end in _s<steps>: the *_n<steps>.npz files of this folder are the whole-run vectors of make_golden.py.)

A fixture holds, for one run of the reference:
  nx, problem, nlim      the root Domain, our deck's name, the cycle limit
  overrides              the command line the reference got (after -i deck -d rundir)
  blocks                 JSON: the <outputN> blocks as the run saw them (what our OutputSet is given), {"N": {key: value}}
  nranks, levels         ranks (NGrid_x3) and, for static mesh refinement, [[Nx1, Nx2, Nx3, iDisp, jDisp, kDisp], ...] of the
                         refined Domains (level l = entry l - 1)
  paths                  every file the run left, relative to its run directory, sorted
  file_<i>               the bytes of paths[i] (uint8) for *.vtk / *.bin
  rst_<i>_U<l>, rst_<i>_time / _dt / _nstep, rst_<i>_num / rst_<i>_next
                         for paths[i] = *.rst: the state of every level l it holds (active zones [k][j][i][6]), MeshS time / dt /
                         nstep, and the `num` / `time` values of <output1..maxout> in its parameter dump
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
from make_golden import REF, REFBIN, read_rst, read_rst_levels      # noqa: E402

MPIEXEC = "/opt/conda/bin/mpiexec"
BLAST = os.path.join(REF, "tst/3D-hydro/athinput.blast")
SPHERE = os.path.join(REF, "tst/massloss/athinput.ioniz_sphere_hires")


def par_values(path, maxout):
    """`num` and `time` of <output1..maxout> in the parameter dump at the head of a restart file"""
    head = open(path, "rb").read().split(b"<par_end>")[0].decode(errors="replace")
    nums, times = [], []
    for n in range(1, maxout + 1):
        m = re.search(r"(?ms)^<output%d>\s*$(.*?)(?=^<)" % n, head)
        body = m.group(1)
        nums.append(int(re.search(r"(?m)^num\s*=\s*(\S+)", body).group(1)))
        times.append(float(re.search(r"(?m)^time\s*=\s*(\S+)", body).group(1)))
    return np.array(nums), np.array(times)


def run(name, exe, deck, problem, nx, nlim, overrides, blocks, nscal=0, ion=False, nranks=1, levels=()):
    tmp = tempfile.mkdtemp(prefix="golden_dumps_")
    try:
        rundir = os.path.join(tmp, "run")
        deck_used = deck
        if nranks > 1:                      # NGrid_x3 is no key of the reference's deck: a copy of it with the line added
            txt = open(deck).read().replace("<domain1>", f"<domain1>\nNGrid_x1 = 1\nNGrid_x2 = 1\nNGrid_x3 = {nranks}", 1)
            deck_used = os.path.join(tmp, "athinput")
            open(deck_used, "w").write(txt)
        over = [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)] + [f"time/nlim={nlim}", f"job/num_domains={1 + len(levels)}"]
        for l, lv in enumerate(levels):
            over += [f"domain{l + 2}/{k}={v}" for k, v in zip(("Nx1", "Nx2", "Nx3", "iDisp", "jDisp", "kDisp"), lv)]
        over += list(overrides)
        args = [os.path.join(REFBIN, exe), "-i", deck_used, "-d", rundir] + over
        env = dict(os.environ)
        if nranks > 1:
            args = [MPIEXEC, "-n", str(nranks)] + args
        if exe.endswith("_mpi"):
            env["LD_LIBRARY_PATH"] = "/opt/conda/lib:" + env.get("LD_LIBRARY_PATH", "")
        pr = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=tmp, env=env, timeout=900)
        if pr.returncode != 0:
            raise RuntimeError(pr.stdout[-2000:] + pr.stderr[-2000:])
        paths = sorted(os.path.relpath(os.path.join(dp, f), rundir) for dp, _, fs in os.walk(rundir) for f in fs)
        d = dict(nx=np.array(nx), problem=problem, nlim=nlim, overrides=np.array(over), blocks=json.dumps(blocks),
                 nranks=nranks, levels=np.array(levels, dtype=np.int64).reshape(-1, 6), paths=np.array(paths))
        maxout = max(int(k) for k in blocks)
        n3 = nx[2] // nranks
        for i, rel in enumerate(paths):
            p = os.path.join(rundir, rel)
            if rel.endswith((".vtk", ".bin")):
                d[f"file_{i}"] = np.frombuffer(open(p, "rb").read(), dtype=np.uint8)
            elif rel.endswith(".rst"):
                if levels:
                    g = read_rst_levels(p, [tuple(nx)] + [tuple(lv[:3]) for lv in levels], nscal, ion)
                    for l, (U, _ef) in enumerate(g["levels"]):
                        d[f"rst_{i}_U{l}"] = U
                else:
                    g = read_rst(p, (nx[0], nx[1], n3), nscal, ion)
                    d[f"rst_{i}_U0"] = g["U"]
                d[f"rst_{i}_time"], d[f"rst_{i}_dt"], d[f"rst_{i}_nstep"] = g["time"], g["dt"], g["nstep"]
                d[f"rst_{i}_num"], d[f"rst_{i}_next"] = par_values(p, maxout)
        out = os.path.join(HERE, name + ".npz")
        np.savez_compressed(out, **d)
        print(f"{name}: {len(paths)} files, {os.path.getsize(out)} bytes: {' '.join(paths)}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def blast_blocks(D, fmt3, out3):
    """the three blocks of the reference's blast deck after the overrides below (the keys the dumps read)"""
    return {"1": {"out_fmt": "rst", "dt": repr(D)}, "2": {"out_fmt": "vtk", "dt": repr(D)},
            "3": {"out_fmt": fmt3, "out": out3, "dt": repr(D)}}


def blast_over(D, fmt3, out3):
    return ["job/maxout=3", "output1/out_fmt=rst", f"output1/dt={D!r}", f"output2/dt={D!r}",
            f"output3/out_fmt={fmt3}", f"output3/out={out3}", f"output3/dt={D!r}"]


def main():
    if not os.path.isdir(REF) or not os.path.isdir(REFBIN):
        sys.exit("needs the reference tree and oracle/_ref (make -C oracle ref)")
    D = 0.004
    # vtk cons + bin prim, NSCALARS = 0, Nx1 a multiple of 4
    run("dump_blast_16x12x8_s5", "athena_blast", BLAST, "blast", (16, 12, 8), 5, blast_over(D, "bin", "prim"), blast_blocks(D, "bin", "prim"))
    # odd Nx1 (ragged payload rows).  <output3> vtk prim writes the SAME file names as <output2> vtk cons and goes second:
    # the run leaves vtk prim; then bin cons beside vtk cons
    run("dump_blast_13x6x5_s3_vtkprim", "athena_blast", BLAST, "blast", (13, 6, 5), 3, blast_over(D, "vtk", "prim"), blast_blocks(D, "vtk", "prim"))
    run("dump_blast_13x6x5_s3_bincons", "athena_blast", BLAST, "blast", (13, 6, 5), 3, blast_over(D, "bin", "cons"), blast_blocks(D, "bin", "cons"))
    # the cadence: D larger than a step, so some passes of the loop write nothing and `num` and the step count part ways
    run("dump_blast_cadence_16x12x8_s8", "athena_blast", BLAST, "blast", (16, 12, 8), 8, blast_over(0.02, "bin", "prim"), blast_blocks(0.02, "bin", "prim"))
    # the headline deck's own two blocks: rst + vtk prim with specific_scalar[0], radiation on (zones with P < 0 and NaN)
    run("dump_ioniz_sphere_20x20x20_s3", "athena_ioniz_sphere", SPHERE, "ioniz_sphere", (20, 20, 20), 3,
        ["output1/dt=1.0", "output2/dt=1.0"],
        {"1": {"out_fmt": "rst", "dt": "1.0"}, "2": {"out_fmt": "vtk", "out": "prim", "dt": "1.0"}}, nscal=1, ion=True)
    # two ranks: id0/Blast.NNNN.*, id1/Blast-id1.NNNN.*, every rank its own Grid
    run("dump_blast_mpi2_16x12x8_s2", "athena_blast_mpi", BLAST, "blast", (16, 12, 8), 2, blast_over(D, "bin", "prim"), blast_blocks(D, "bin", "prim"), nranks=2)
    # static mesh refinement: root + one 8^3 patch; lev1/Blast-lev1.NNNN.*, one rst for all levels
    run("dump_blast_smr_16x12x8_s1", "athena_blast_smr", BLAST, "blast", (16, 12, 8), 1, blast_over(D, "bin", "prim"), blast_blocks(D, "bin", "prim"),
        levels=[(8, 8, 8, 12, 8, 4)])


if __name__ == "__main__":
    main()
