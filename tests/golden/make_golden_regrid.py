"""Regenerates tests/golden/regrid_*.npz: restart dumps of the UNMODIFIED reference's MPI executables (oracle/Makefile.ref targets
blast_mpi and ioniz_sphere_mpi) on decompositions this package never runs on -- x1 cuts among them -- and what the reference made
of them when it was continued with ``athena -r``.  TEST INFRASTRUCTURE: needs the reference tree and oracle/_ref; the tests only
read the .npz files.

A fixture holds (names as in make_golden_restart.py where they mean the same):
  nx, problem, nlim, overrides, blocks, nranks, ngrid, resume_overrides
  seed_names, seed_<i>             the restart dumps of all ranks the run was resumed from (relative paths, rank order; raw bytes)
  seed_nstep, seed_time, seed_dt   rank 0's
  paths                            every file the RESUMED run left
  niter                            radiation sub-cycles of every step of the resumed run (the same on every rank)
  final_<r>_U, final_<r>_EF, final_time, final_dt, final_nstep
                                   the last restart dump of the resumed run, per rank
and three findings about the reference alone:
  vtkhead_<r>                      rank r's first vtk file up to its first SCALARS line: DIMENSIONS and ORIGIN are the Grid as the
                                   reference cut it
  seed_join_equal                  the seeds joined by the Grids' displacements (EdgeFlux by the rule of restart.box_pieces) equal
                                   the seed the ONE-rank executable wrote for the same deck, bit for bit -- U, EdgeFlux, time, dt
  seed_join_u_equal, seed_join_ef_equal, seed_join_time_equal    ... the parts of that finding
  ef_shared_equal, ef_shared_differ      whether the EdgeFlux entries two neighbouring files hold for their common face agree
                                         ([x1, x2, x3] counts of differing entries)"""
import json
import os
import re
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REFBIN, read_rst      # noqa: E402
from make_golden_dumps import BLAST, SPHERE        # noqa: E402
from make_golden_restart import blast_blocks, blast_over, execute, tree      # noqa: E402


def boxes(nx, ngrid):
    """init_mesh.c:575-653, written out once more (the package's restart.grid_boxes is what the tests check against the vtk headers)"""
    sz, dp = [], []
    for d in range(3):
        q, r = divmod(nx[d], ngrid[d])
        s = [q + r] + [q] * (ngrid[d] - 1)
        sz.append(s); dp.append([sum(s[:i]) for i in range(ngrid[d])])
    return [((dp[0][l], dp[1][m], dp[2][n]), (sz[0][l], sz[1][m], sz[2][n]))
            for n in range(ngrid[2]) for m in range(ngrid[1]) for l in range(ngrid[0])]


def rank_of(rel):
    m = re.search(r"-id(\d+)\.", os.path.basename(rel))
    return int(m.group(1)) if m else 0


def join(states, bx, nx, ion):
    U = np.zeros((nx[2], nx[1], nx[0], 6)); ef = np.zeros((nx[2] + 1, nx[1] + 1, nx[0] + 1)) if ion else None
    differ = [0, 0, 0]
    for st, (lo, n) in zip(states, bx):
        U[lo[2]:lo[2] + n[2], lo[1]:lo[1] + n[1], lo[0]:lo[0] + n[0]] = st["U"]
    if ion:
        # lower Grids first, so that the shared entry is the upper Grid's; and what the two files say about it
        seen = np.zeros(ef.shape, dtype=bool)
        for st, (lo, n) in zip(states, bx):
            sl = tuple(slice(lo[d], lo[d] + n[d] + 1) for d in (2, 1, 0))
            e = st["edgeflux"]
            for d in range(3):                # the lower face plane of this Grid against what the Grid below it wrote there
                if lo[d] == 0:
                    continue
                ax = 2 - d
                mine = np.take(e, 0, axis=ax); theirs = np.take(ef[sl], 0, axis=ax); known = np.take(seen[sl], 0, axis=ax)
                differ[d] += int(np.count_nonzero((mine.view(np.uint64) != theirs.view(np.uint64)) & known))
            ef[sl] = e; seen[sl] = True
    return U, ef, differ


def case(name, exe, exe1, deck, problem, nx, ngrid, nlim, overrides, blocks, seed_num, nscal=0, ion=False, seed_step=None):
    nranks = ngrid[0] * ngrid[1] * ngrid[2]
    tmp = tempfile.mkdtemp(prefix="golden_regrid_")
    try:
        full, res, seeds, one = (os.path.join(tmp, d) for d in ("full", "resumed", "seeds", "one"))
        # (the sphere's deck names its own cuts: those lines go)
        txt = re.sub(r"(?m)^\s*(NGrid_x[123]|AutoWithNProc)\s*=.*\n", "", open(deck).read())
        txt = txt.replace("<domain1>", f"<domain1>\nNGrid_x1 = {ngrid[0]}\nNGrid_x2 = {ngrid[1]}\nNGrid_x3 = {ngrid[2]}", 1)
        deck_used = os.path.join(tmp, "athinput")
        open(deck_used, "w").write(txt)
        over = [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)] + [f"time/nlim={nlim}", "job/num_domains=1"] + list(overrides)
        execute(exe, ["-i", deck_used, "-d", full] + over, nranks, tmp)
        execute(exe1, ["-i", deck, "-d", one] + over, 1, tmp)
        seed_rel = sorted((p for p in tree(full) if p.endswith(".%04d.rst" % seed_num)), key=rank_of)
        assert len(seed_rel) == nranks and [rank_of(p) for p in seed_rel] == list(range(nranks)), seed_rel
        os.makedirs(seeds)
        for p in seed_rel:
            shutil.copy(os.path.join(full, p), os.path.join(seeds, os.path.basename(p)))
        pr = execute(exe, ["-r", os.path.join(seeds, os.path.basename(seed_rel[0])), "-d", res], nranks, tmp)
        niter = [int(m) for m in re.findall(r"Radiation done in (\d+) iterations", pr.stdout + pr.stderr)]
        if niter:                           # every rank prints every step's count, in no order: one value or none at all
            assert len(set(niter)) == 1 and len(niter) % nranks == 0, niter
            niter = niter[:len(niter) // nranks]
        paths = tree(res)
        bx = boxes(nx, ngrid)
        states = [read_rst(os.path.join(full, p), n, nscal, ion) for p, (_lo, n) in zip(seed_rel, bx)]
        assert all(not np.isnan(s["U"]).any() for s in states)
        if seed_step is not None:
            assert states[0]["nstep"] == seed_step, states[0]["nstep"]
        d = dict(nx=np.array(nx), problem=problem, nlim=nlim, overrides=np.array(over), blocks=json.dumps(blocks), nranks=nranks,
                 ngrid=np.array(ngrid), levels=np.zeros((0, 6), dtype=np.int64), paths=np.array(paths), seed_names=np.array(seed_rel),
                 resume_overrides=np.array([], dtype=str), niter=np.array(niter, dtype=np.int64),
                 seed_nstep=states[0]["nstep"], seed_time=states[0]["time"], seed_dt=states[0]["dt"])
        for i, p in enumerate(seed_rel):
            d[f"seed_{i}"] = np.frombuffer(open(os.path.join(full, p), "rb").read(), dtype=np.uint8)
        # finding 1: the Grids as the reference cut them
        for r in range(nranks):
            vtk = sorted(p for p in tree(full) if p.startswith(f"id{r}/") and p.endswith(".vtk"))[0]
            b = open(os.path.join(full, vtk), "rb").read()
            d[f"vtkhead_{r}"] = b[:b.index(b"SCALARS")].decode()
        # finding 2: the joined seeds against the one-rank executable's seed
        one_seed = [p for p in tree(one) if p.endswith(".%04d.rst" % seed_num)]
        assert len(one_seed) == 1
        s1 = read_rst(os.path.join(one, one_seed[0]), nx, nscal, ion)
        U, ef, differ = join(states, bx, nx, ion)
        ueq = bool(np.array_equal(U.view(np.uint64), s1["U"].view(np.uint64)))
        eeq = bool(not ion or np.array_equal(ef.view(np.uint64), s1["edgeflux"].view(np.uint64)))
        teq = bool((s1["time"], s1["dt"], s1["nstep"]) == (states[0]["time"], states[0]["dt"], states[0]["nstep"]))
        d["seed_join_u_equal"], d["seed_join_ef_equal"], d["seed_join_time_equal"] = ueq, eeq, teq
        d["seed_join_equal"] = ueq and eeq and teq
        # finding 3: the entries neighbouring files share
        d["ef_shared_differ"] = np.array(differ); d["ef_shared_equal"] = bool(sum(differ) == 0)
        # the last restart dump of the resumed run
        last = max(int(p.rsplit(".", 2)[1]) for p in paths if p.endswith(".rst"))
        fin = sorted((p for p in paths if p.endswith(".%04d.rst" % last)), key=rank_of)
        assert len(fin) == nranks
        for r, (p, (_lo, n)) in enumerate(zip(fin, bx)):
            st = read_rst(os.path.join(res, p), n, nscal, ion)
            d[f"final_{r}_U"] = st["U"]
            if ion:
                d[f"final_{r}_EF"] = st["edgeflux"]
            if r == 0:
                d["final_time"], d["final_dt"], d["final_nstep"] = st["time"], st["dt"], st["nstep"]
        out = os.path.join(HERE, name + ".npz")
        np.savez_compressed(out, **d)
        print(f"{name}: {nranks} seeds at nstep {int(d['seed_nstep'])}, resumed to {int(d['final_nstep'])}; joined seeds equal the one-rank "
              f"seed: U {ueq} EdgeFlux {eeq} time/dt {teq}; shared EdgeFlux entries that differ (x1, x2, x3): {differ}; "
              f"{os.path.getsize(out)} bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def rst_time(exe1, deck, nx, nlim, tmp_root):
    """the time of the one-rank run after `nlim` steps"""
    tmp = tempfile.mkdtemp(prefix="golden_regrid_probe_", dir=tmp_root)
    over = [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)] + [f"time/nlim={nlim}"] + blast_over(1e300, 1e300)
    execute(exe1, ["-i", deck, "-d", tmp] + over, 1, tmp)
    last = sorted(p for p in tree(tmp) if p.endswith(".rst"))[-1]
    return read_rst(os.path.join(tmp, last), nx, 0, False)["time"]


def main():
    if not os.path.isdir(REF) or not os.path.isdir(REFBIN):
        sys.exit("needs the reference tree and oracle/_ref (make -C oracle ref)")
    only = sys.argv[1:]
    global case
    every = case
    case = lambda name, *a, **k: every(name, *a, **k) if not only or name in only else None      # noqa: E731
    case("regrid_blast_x1x3_16x12x8_s3_s8", "athena_blast_mpi", "athena_blast", BLAST, "blast", (16, 12, 8), (2, 1, 2), 8,
         blast_over(0.02, 0.01), blast_blocks(0.02, 0.01), 1, seed_step=3)
    # 22 x 12 x 9 on 4 x 1 x 2: Grids of 7, 5, 5, 5 zones along x1 and 5, 4 along x3; an output interval that puts 0001.rst at cycle 3
    nx = (22, 12, 9)
    probe = tempfile.mkdtemp(prefix="golden_regrid_")
    try:
        D = 0.5 * (rst_time("athena_blast", BLAST, nx, 2, probe) + rst_time("athena_blast", BLAST, nx, 3, probe))
    finally:
        shutil.rmtree(probe, ignore_errors=True)
    D = float("%.6g" % D)
    case("regrid_blast_uneven_22x12x9_s3_s6", "athena_blast_mpi", "athena_blast", BLAST, "blast", nx, (4, 1, 2), 6,
         blast_over(D, D), blast_blocks(D, D), 1, seed_step=3)
    zoom = [f"domain1/x{d}{m}={s}1.5e10" for d in (1, 2, 3) for m, s in (("min", "-"), ("max", ""))]
    case("regrid_ioniz_sphere_x1x2_24x20x16_s6_s10", "athena_ioniz_sphere_mpi", "athena_ioniz_sphere", SPHERE, "ioniz_sphere", (24, 20, 16),
         (2, 2, 1), 10, ["output1/dt=2e-4", "output2/dt=2e-4"] + zoom,
         {"1": {"out_fmt": "rst", "dt": "2e-4"}, "2": {"out_fmt": "vtk", "out": "prim", "dt": "2e-4"}}, 1, nscal=1, ion=True, seed_step=6)


if __name__ == "__main__":
    main()
