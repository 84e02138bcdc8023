"""Regenerates tests/golden/restart_*.npz: runs of the UNMODIFIED reference executables (oracle/Makefile.ref) that were
interrupted and continued with ``athena -r``.  TEST INFRASTRUCTURE: needs the reference tree and oracle/_ref; the tests only read
the .npz files.

Every fixture follows the dump_*.npz layout of make_golden_dumps.py (nx, problem, nlim, overrides, blocks, nranks, levels, paths,
file_<i>, rst_<i>_*) and describes the tree the RESUMED run left.  In addition:
  seed_names, seed_<i>     the restart dump(s) the run was resumed from, relative path(s) in the uninterrupted run's tree and raw bytes
  seed_nstep, seed_time, seed_dt   the cycle the seed was written at, its time and dt
  resume_overrides         the block/key=value arguments behind ``-r file``
  niter                    radiation sub-cycles of every step of the resumed run (ion radiation)
  hst_<i>                  the text of paths[i] = *.hst
  rst_<i>_EF<l>            GridS.EdgeFlux of level l of paths[i] = *.rst (ion radiation)

The generator asserts what the issue states of the reference alone: no NaN word in any restart payload, and the uninterrupted
run's later files equal the resumed run's (dumps byte for byte; restart dumps in U, EdgeFlux, time, dt, nstep and the num / time
values of every block; the resumed .hst is the tail of the uninterrupted one, without a header)."""
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
from make_golden_dumps import BLAST, MPIEXEC, SPHERE, par_values     # noqa: E402


def execute(exe, args, nranks, cwd):
    env = dict(os.environ)
    cmd = [os.path.join(REFBIN, exe)] + args
    if nranks > 1:
        cmd = [MPIEXEC, "-n", str(nranks)] + cmd
    if exe.endswith("_mpi"):
        env["LD_LIBRARY_PATH"] = "/opt/conda/lib:" + env.get("LD_LIBRARY_PATH", "")
    pr = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, env=env, timeout=900)
    if pr.returncode != 0:
        raise RuntimeError(pr.stdout[-2000:] + pr.stderr[-2000:])
    assert "Neg or NaN" not in pr.stdout + pr.stderr
    return pr


def tree(rundir):
    return sorted(os.path.relpath(os.path.join(dp, f), rundir) for dp, _, fs in os.walk(rundir) for f in fs)


def read_state(p, nx, nranks, levels, nscal, ion):
    """-> ([(U, edgeflux)] per level, time, dt, nstep)"""
    if levels:
        g = read_rst_levels(p, [tuple(nx)] + [tuple(lv[:3]) for lv in levels], nscal, ion)
        lv = g["levels"]
    else:
        g = read_rst(p, (nx[0], nx[1], nx[2] // nranks), nscal, ion)
        lv = [(g["U"], g["edgeflux"])]
    return lv, g["time"], g["dt"], g["nstep"]


def case(name, exe, deck, problem, nx, nlim, overrides, blocks, seed_num, resume_overrides=(), nscal=0, ion=False, nranks=1, levels=()):
    tmp = tempfile.mkdtemp(prefix="golden_restart_")
    try:
        full, res, seeds = (os.path.join(tmp, d) for d in ("full", "resumed", "seeds"))
        deck_used = deck
        if nranks > 1:                      # NGrid_x3 is no key of the reference's deck: a copy of it with the line added
            txt = open(deck).read().replace("<domain1>", f"<domain1>\nNGrid_x1 = 1\nNGrid_x2 = 1\nNGrid_x3 = {nranks}", 1)
            deck_used = os.path.join(tmp, "athinput")
            open(deck_used, "w").write(txt)
        over = [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)] + [f"time/nlim={nlim}", f"job/num_domains={1 + len(levels)}"]
        for l, lv in enumerate(levels):
            over += [f"domain{l + 2}/{k}={v}" for k, v in zip(("Nx1", "Nx2", "Nx3", "iDisp", "jDisp", "kDisp"), lv)]
        over += list(overrides)
        execute(exe, ["-i", deck_used, "-d", full] + over, nranks, tmp)
        # the seed file(s), all in ONE directory: rank r reads <dir of rank 0's file>/<basename>-id<r>.NNNN.rst (main.c:265-288)
        seed_rel = [p for p in tree(full) if p.endswith(".%04d.rst" % seed_num)]
        assert len(seed_rel) == nranks, seed_rel
        os.makedirs(seeds)
        for p in seed_rel:
            shutil.copy(os.path.join(full, p), os.path.join(seeds, os.path.basename(p)))
        seed0 = [p for p in seed_rel if "-id" not in os.path.basename(p)]
        assert len(seed0) == 1
        pr = execute(exe, ["-r", os.path.join(seeds, os.path.basename(seed0[0])), "-d", res] + list(resume_overrides), nranks, tmp)
        niter = [int(m) for m in re.findall(r"Radiation done in (\d+) iterations", pr.stdout + pr.stderr)]
        paths = tree(res)
        nlim_res = nlim
        for a in resume_overrides:
            if a.startswith("time/nlim="):
                nlim_res = int(a.split("=")[1])
        d = dict(nx=np.array(nx), problem=problem, nlim=nlim_res, overrides=np.array(over), blocks=json.dumps(blocks),
                 nranks=nranks, levels=np.array(levels, dtype=np.int64).reshape(-1, 6), paths=np.array(paths),
                 seed_names=np.array(seed_rel), resume_overrides=np.array(list(resume_overrides), dtype=str),
                 niter=np.array(niter, dtype=np.int64), seed_nstep=read_state(os.path.join(full, seed_rel[0]), nx, nranks, levels, nscal, ion)[3])
        for i, p in enumerate(seed_rel):
            d[f"seed_{i}"] = np.frombuffer(open(os.path.join(full, p), "rb").read(), dtype=np.uint8)
        _lv, d["seed_time"], d["seed_dt"], _n = read_state(os.path.join(full, seed_rel[0]), nx, nranks, levels, nscal, ion)
        maxout = max(int(k) for k in blocks)
        same_as_full = nlim_res == nlim
        for i, rel in enumerate(paths):
            p = os.path.join(res, rel); q = os.path.join(full, rel)
            if rel.endswith((".vtk", ".bin")):
                b = open(p, "rb").read()
                d[f"file_{i}"] = np.frombuffer(b, dtype=np.uint8)
                if same_as_full:
                    assert b == open(q, "rb").read(), rel           # (no NaN word in these runs: plain equality is the rule)
            elif rel.endswith(".hst"):
                d[f"hst_{i}"] = open(p).read()
                rows = d[f"hst_{i}"].splitlines()
                assert not any(r.startswith("#") for r in rows), rel
                if same_as_full:
                    assert open(q).read().splitlines()[-len(rows):] == rows, rel
            elif rel.endswith(".rst"):
                lv, time, dt, nstep = read_state(p, nx, nranks, levels, nscal, ion)
                for l, (U, ef) in enumerate(lv):
                    assert not np.isnan(U).any() and (ef is None or not np.isnan(ef).any()), rel
                    d[f"rst_{i}_U{l}"] = U
                    if ef is not None:
                        d[f"rst_{i}_EF{l}"] = ef
                d[f"rst_{i}_time"], d[f"rst_{i}_dt"], d[f"rst_{i}_nstep"] = time, dt, nstep
                d[f"rst_{i}_num"], d[f"rst_{i}_next"] = par_values(p, maxout)
                if same_as_full:
                    lq, tq, dq, nq = read_state(q, nx, nranks, levels, nscal, ion)
                    assert (tq, dq, nq) == (time, dt, nstep), rel
                    for (U, ef), (Uq, efq) in zip(lv, lq):
                        assert np.array_equal(U, Uq) and (ef is None or np.array_equal(ef, efq)), rel
                    nq_, xq_ = par_values(q, maxout)
                    assert np.array_equal(nq_, d[f"rst_{i}_num"]) and np.array_equal(xq_, d[f"rst_{i}_next"]), rel
        if same_as_full:                    # the resumed run left every file the uninterrupted one wrote after the seed
            later = [p for p in tree(full) if p.endswith(".hst") or int(p.rsplit(".", 2)[1]) > seed_num]
            assert later == paths, (later, paths)
        out = os.path.join(HERE, name + ".npz")
        np.savez_compressed(out, **d)
        print(f"{name}: seed(s) {' '.join(seed_rel)} ({sum(d[f'seed_{i}'].size for i in range(nranks))} bytes) at nstep {int(d['seed_nstep'])}; "
              f"{len(paths)} files, {os.path.getsize(out)} bytes: {' '.join(paths)}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def blast_over(D, Dh):
    return ["job/maxout=3", "output1/out_fmt=rst", f"output1/dt={D!r}", f"output2/dt={D!r}",
            "output3/out_fmt=hst", "output3/out=cons", f"output3/dt={Dh!r}"]


def blast_blocks(D, Dh):
    return {"1": {"out_fmt": "rst", "dt": repr(D)}, "2": {"out_fmt": "vtk", "dt": repr(D)},
            "3": {"out_fmt": "hst", "out": "cons", "dt": repr(Dh)}}


def main():
    if not os.path.isdir(REF) or not os.path.isdir(REFBIN):
        sys.exit("needs the reference tree and oracle/_ref (make -C oracle ref)")
    nx = (16, 12, 8)
    case("restart_blast_16x12x8_s3_s8", "athena_blast", BLAST, "blast", nx, 8, blast_over(0.02, 0.01), blast_blocks(0.02, 0.01), 1)
    case("restart_blast_16x12x8_s3_s11", "athena_blast", BLAST, "blast", nx, 8, blast_over(0.02, 0.01), blast_blocks(0.02, 0.01), 1,
         resume_overrides=["time/nlim=11"])
    case("restart_blast_mpi2_16x12x8_s3_s8", "athena_blast_mpi", BLAST, "blast", nx, 8, blast_over(0.02, 0.01), blast_blocks(0.02, 0.01), 1,
         nranks=2)
    case("restart_blast_smr_16x12x8_s2_s5", "athena_blast_smr", BLAST, "blast", nx, 5, blast_over(0.004, 0.004), blast_blocks(0.004, 0.004), 2,
         levels=[(8, 8, 8, 12, 8, 4)])
    zoom = [f"domain1/x{d}{m}={s}1.5e10" for d in (1, 2, 3) for m, s in (("min", "-"), ("max", ""))]
    case("restart_ioniz_sphere_24x20x16_s6_s10", "athena_ioniz_sphere", SPHERE, "ioniz_sphere", (24, 20, 16), 10,
         ["output1/dt=2e-4", "output2/dt=2e-4"] + zoom,
         {"1": {"out_fmt": "rst", "dt": "2e-4"}, "2": {"out_fmt": "vtk", "out": "prim", "dt": "2e-4"}}, 1, nscal=1, ion=True)


if __name__ == "__main__":
    main()
