"""Regenerates tests/golden/meshdrv_*.npz: runs of the UNMODIFIED reference built with --enable-mpi --enable-smr
(oracle/Makefile.ref: athena_blast_smr_mpi, athena_ioniz_sphere_smr_mpi) on two ranks, with ``NGrid_x3 = 2`` in EVERY <domainN>
and the refined Domain centred on the root's cut -- the reference counterpart of driver.MeshDriver on two ranks.  TEST
INFRASTRUCTURE: needs the reference tree and oracle/_ref; the tests only read the .npz files.  It runs only executables under
oracle/_ref and stores only what they wrote.

The key layout is that of make_golden_dumps.py (nx, problem, nlim, overrides, blocks, nranks, levels, paths, file_<i>,
rst_<i>_*) and make_golden_restart.py (seed_names, seed_<i>, seed_nstep / _time / _dt, resume_overrides, hst_<i>,
rst_<i>_EF<l>), with nranks = 2 AND levels both set: a restart dump of rank r holds the Grids of r, root first, and level l of
rank r has (Nx1, Nx2, Nx3 / 2) zones.  In addition:
  niter            [steps][levels] radiation sub-cycles of every step of the (resumed) run, as rank 0 printed them
  size_<i>         the size of paths[i] where its bytes are not kept (`lean` fixtures: dumps are compared by size there)
A `lean` fixture keeps the state (U, EdgeFlux) of the LAST restart dump of every rank only; time, dt, nstep and the blocks'
num / time values are kept for all of them.

The generator asserts what is stated of the reference alone: no NaN in any restart payload; the tree of the first blast run
is the one listed in main(); a resumed .hst holds rows only; with radiation both levels do more than one sub-cycle in every
stored step."""
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
from make_golden import REF, REFBIN, read_rst_levels                 # noqa: E402
from make_golden_dumps import BLAST, MPIEXEC, SPHERE, par_values     # noqa: E402

NRANKS = 2


def deck_copy(deck, path, ndom, blocks):
    """the reference's deck with NGrid_x3 = NRANKS in every <domainN> and `blocks` as its only <outputN> blocks (neither can
    be given on the command line: par_cmdline refuses a block or key the deck does not hold)"""
    txt = open(deck).read()
    txt = re.sub(r"(?m)^NGrid_x[123]\s*=.*\n", "", txt)
    txt = re.sub(r"(?ms)^<output\d+>.*?(?=^<)", "", txt)
    for n in range(1, ndom + 1):
        txt = txt.replace(f"<domain{n}>", f"<domain{n}>\nNGrid_x1 = 1\nNGrid_x2 = 1\nNGrid_x3 = {NRANKS}", 1)
    txt = re.sub(r"(?m)^maxout\s*=.*$", "maxout = %d" % max(int(k) for k in blocks), txt, count=1)
    for n, kv in sorted(blocks.items(), key=lambda t: int(t[0])):
        txt += f"\n<output{n}>\n" + "".join(f"{k} = {v}\n" for k, v in kv.items())
    open(path, "w").write(txt)


def execute(exe, args, cwd):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/conda/lib:" + env.get("LD_LIBRARY_PATH", "")
    cmd = [MPIEXEC, "-prepend-rank", "-n", str(NRANKS), os.path.join(REFBIN, exe)] + args
    pr = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, env=env, timeout=1800)
    if pr.returncode != 0:
        raise RuntimeError(pr.stdout[-2000:] + pr.stderr[-2000:])
    assert "Neg or NaN" not in pr.stdout + pr.stderr
    return pr


def tree(rundir):
    return sorted(os.path.relpath(os.path.join(dp, f), rundir) for dp, _, fs in os.walk(rundir) for f in fs)


def sub_cycles(pr, nlev):
    """[steps][levels] as rank 0 printed them, root first (mpiexec -prepend-rank tags every line with its rank)"""
    n = [int(m) for m in re.findall(r"(?m)^\[0\].*Radiation done in (\d+) iterations", pr.stdout + pr.stderr)]
    assert n and len(n) % nlev == 0, len(n)
    return np.array(n, dtype=np.int64).reshape(-1, nlev)


def store_tree(d, rundir, paths, nxs, nscal, ion, maxout, lean):
    last = {}
    for rel in paths:
        if rel.endswith(".rst"):
            last[rel.split("/")[0]] = rel                   # (sorted: the highest number of every rank stays)
    for i, rel in enumerate(paths):
        p = os.path.join(rundir, rel)
        if rel.endswith((".vtk", ".bin")):
            if lean:
                d[f"size_{i}"] = os.path.getsize(p)
            else:
                d[f"file_{i}"] = np.frombuffer(open(p, "rb").read(), dtype=np.uint8)
        elif rel.endswith(".hst"):
            d[f"hst_{i}"] = open(p).read()
        elif rel.endswith(".rst"):
            g = read_rst_levels(p, nxs, nscal, ion)
            for l, (U, ef) in enumerate(g["levels"]):
                assert not np.isnan(U).any() and (ef is None or not np.isnan(ef).any()), rel
                if lean and last[rel.split("/")[0]] != rel:
                    continue
                d[f"rst_{i}_U{l}"] = U
                if ef is not None:
                    d[f"rst_{i}_EF{l}"] = ef
            d[f"rst_{i}_time"], d[f"rst_{i}_dt"], d[f"rst_{i}_nstep"] = g["time"], g["dt"], g["nstep"]
            d[f"rst_{i}_num"], d[f"rst_{i}_next"] = par_values(p, maxout)
            if lean:
                d[f"size_{i}"] = os.path.getsize(p)


def case(name, exe, deck, problem, nx, level1, nlim, blocks, overrides=(), nscal=0, ion=False, seed_num=None, resumed_name=None,
         resume_overrides=(), lean=False, want_tree=None, keep_full=True):
    """One uninterrupted run to `nlim` (stored as `name` if keep_full) and, with seed_num, the run resumed from the restart
    dumps of that number (stored as `resumed_name`)."""
    tmp = tempfile.mkdtemp(prefix="golden_meshdrv_")
    try:
        full, res, seeds = (os.path.join(tmp, x) for x in ("full", "resumed", "seeds"))
        deck_used = os.path.join(tmp, "athinput")
        deck_copy(deck, deck_used, 2, blocks)
        levels = [tuple(level1)]
        over = [f"domain1/Nx{a + 1}={nx[a]}" for a in range(3)] + [f"time/nlim={nlim}", "job/num_domains=2"]
        over += [f"domain2/{k}={v}" for k, v in zip(("Nx1", "Nx2", "Nx3", "iDisp", "jDisp", "kDisp"), level1)]
        over += list(overrides)
        assert nx[2] % NRANKS == 0 and level1[2] % NRANKS == 0 and level1[5] + level1[2] // 2 == nx[2], "level 1 centred on the cut"
        nxs = [(nx[0], nx[1], nx[2] // NRANKS), (level1[0], level1[1], level1[2] // NRANKS)]
        maxout = max(int(k) for k in blocks)
        pr = execute(exe, ["-i", deck_used, "-d", full] + over, tmp)
        paths = tree(full)
        if want_tree is not None:
            assert paths == sorted(want_tree), (paths, sorted(want_tree))
        base = dict(nx=np.array(nx), problem=problem, overrides=np.array(over), blocks=json.dumps(blocks), nranks=NRANKS,
                    levels=np.array(levels, dtype=np.int64).reshape(-1, 6))
        if keep_full:
            d = dict(base, nlim=nlim, paths=np.array(paths))
            if ion:
                d["niter"] = sub_cycles(pr, 2)
            store_tree(d, full, paths, nxs, nscal, ion, maxout, lean)
            out = os.path.join(HERE, name + ".npz")
            np.savez_compressed(out, **d)
            print(f"{name}: {len(paths)} files, {os.path.getsize(out)} bytes: {' '.join(paths)}")
        if seed_num is None:
            return
        seed_rel = [p for p in paths if p.endswith(".%04d.rst" % seed_num)]
        assert len(seed_rel) == NRANKS, seed_rel
        os.makedirs(seeds)
        for p in seed_rel:
            shutil.copy(os.path.join(full, p), os.path.join(seeds, os.path.basename(p)))
        seed0 = [p for p in seed_rel if "-id" not in os.path.basename(p)]
        assert len(seed0) == 1
        pr = execute(exe, ["-r", os.path.join(seeds, os.path.basename(seed0[0])), "-d", res] + list(resume_overrides), tmp)
        paths = tree(res)
        nlim_res = nlim
        for a in resume_overrides:
            if a.startswith("time/nlim="):
                nlim_res = int(a.split("=")[1])
        g0 = read_rst_levels(os.path.join(full, seed0[0]), nxs, nscal, ion)
        d = dict(base, nlim=nlim_res, paths=np.array(paths), seed_names=np.array(seed_rel),
                 resume_overrides=np.array(list(resume_overrides), dtype=str), seed_nstep=g0["nstep"], seed_time=g0["time"],
                 seed_dt=g0["dt"])
        for i, p in enumerate(seed_rel):
            d[f"seed_{i}"] = np.frombuffer(open(os.path.join(full, p), "rb").read(), dtype=np.uint8)
        niter = np.zeros((0, 2), dtype=np.int64)
        if ion:
            niter = sub_cycles(pr, 2)
            assert len(niter) == nlim_res - int(g0["nstep"]) and niter.min() > 1, niter       # both levels sub-cycle in every stored step
        d["niter"] = niter
        store_tree(d, res, paths, nxs, nscal, ion, maxout, lean)
        for i, rel in enumerate(paths):
            if rel.endswith(".hst"):
                assert not any(r.startswith("#") for r in d[f"hst_{i}"].splitlines()), rel
        assert not any(p.endswith(".hst") and not p.startswith("id0/") for p in paths), paths
        out = os.path.join(HERE, resumed_name + ".npz")
        np.savez_compressed(out, **d)
        print(f"{resumed_name}: seeds {' '.join(seed_rel)} at nstep {int(g0['nstep'])}; niter {niter.tolist()}; {len(paths)} files, "
              f"{os.path.getsize(out)} bytes: {' '.join(paths)}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def blast_tree():
    t = ["id0/Blast.hst", "id0/lev1/Blast-lev1.hst"]
    for r, base in ((0, "Blast"), (1, "Blast-id1")):
        for n in range(4):
            t += [f"id{r}/{base}.{n:04d}.rst", f"id{r}/{base}.{n:04d}.vtk", f"id{r}/lev1/{base}-lev1.{n:04d}.vtk"]
        for n in range(2):
            t += [f"id{r}/{base}.{n:04d}.bin", f"id{r}/lev1/{base}-lev1.{n:04d}.bin"]
    return t


def main():
    if not os.path.isdir(REF) or not os.path.isdir(REFBIN):
        sys.exit("needs the reference tree and oracle/_ref (make -C oracle ref)")
    blocks = {"1": {"out_fmt": "rst", "dt": "0.004"}, "2": {"out_fmt": "vtk", "out": "prim", "dt": "0.004"},
              "3": {"out_fmt": "hst", "dt": "0.002"}, "4": {"out_fmt": "bin", "dt": "0.01"}}
    case("meshdrv_blast_mpi2_s4", "athena_blast_smr_mpi", BLAST, "blast", (16, 12, 16), (16, 12, 16, 8, 6, 8), 4, blocks,
         seed_num=2, resumed_name="meshdrv_restart_blast_mpi2_s3_s7", resume_overrides=["time/nlim=7"], want_tree=blast_tree())
    # the sphere of test_gpu_dropin_mpi.py (32^3 root, rp = 2.1e10) cut down in x2 and x3 at the same zone size, so that two
    # seed files and two restart dumps in full precision fit a small fixture; the rays keep their 32 zones on both levels.
    # Output intervals far below a step: every pass of the loop writes.
    sblocks = {"1": {"out_fmt": "rst", "dt": "1e-4"}, "2": {"out_fmt": "vtk", "out": "prim", "dt": "1e-4"},
               "3": {"out_fmt": "hst", "dt": "1e-4"}}
    case(None, "athena_ioniz_sphere_smr_mpi", SPHERE, "ioniz_sphere", SPHERE_NX, SPHERE_L1, 2, sblocks, SPHERE_OVER,
         nscal=1, ion=True, seed_num=2, resumed_name="meshdrv_restart_ioniz_sphere_mpi2", resume_overrides=["time/nlim=4"],
         lean=True, keep_full=False)


SPHERE_NX = (32, 16, 16)
SPHERE_L1 = (32, 24, 16, 16, 4, 8)
SPHERE_OVER = ["domain1/x2min=-3.75e10", "domain1/x2max=3.75e10", "domain1/x3min=-3.75e10", "domain1/x3max=3.75e10", "problem/rp=2.1e10"]

if __name__ == "__main__":
    main()
