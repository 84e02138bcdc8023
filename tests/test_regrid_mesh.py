"""Resuming a refined run on other cuts than those that wrote the restart dumps (``MeshDriver.from_restart(..., regrid=True)``),
and writing the restart dumps of a refined mesh for other cuts (``OutputSet.from_par(..., rst_mesh_ngrid=...)``), on the CPU.

Fixtures: tests/golden/regridmesh_*.npz (tests/golden/make_golden_regrid_mesh.py) -- seeds of the reference built with MPI and
static mesh refinement on four ranks, every <domainN> cut by its own NGrid_x*: x1 cuts, Grids of 7, 5, 5, 5 zones, ranks without a
Grid of the root, two Domains on a level.  The engine is the oracle (test infrastructure; bit for bit on the blast deck), so what is
tested is the layer above it: restart.mesh_grid_boxes / scan_mesh_sources, the per-Domain boxes, the runners and the writer.  The
generator asserted that the reference's blast runs on these cuts and on 1 x 1 x 2 agree bit for bit: everything here is exact."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import meshfix                                         # noqa: E402
import regridmeshfix                                   # noqa: E402
from dumpfix import pkg                                # noqa: E402
from regridmeshfix import RMFixture, bits              # noqa: E402
from test_mesh_driver_outputs import OutputMeshEngine  # noqa: E402
from test_restart_resume import RestartOracleEngine    # noqa: E402

# x3 cuts (root planes) that no seed was written on: the seeds cut the root at plane 8 (blast2_*) and 9 (blast3_uneven)
CUTS = {"blast2_x1x3": (0, 6, 16), "blast2_noroot": (0, 6, 16), "blast3_uneven": (0, 10, 18)}


# ---- 1. the Grids of a decomposition, against the seed files themselves -----------------------------------------------------------
@pytest.mark.parametrize("name", regridmeshfix.CASES)
def test_mesh_grid_boxes_against_the_seeds(name, tmp_path):
    R = pkg("restart")
    fx = RMFixture(name)
    table = R.mesh_grid_boxes(list(zip(fx.Nxs, fx.ngrid)), fx.nranks)
    assert table == fx.dealt()
    seed = fx.write_seeds(str(tmp_path / "seed"))
    head = R.read_head(seed)
    assert R.par_mesh_ngrid(head["par"]) == fx.ngrid and (head["nstep"], head["time"], head["dt"]) == (fx.seed_nstep, fx.seed_time, fx.seed_dt)
    sources = R.scan_mesh_sources(seed, fx.Nxs, fx.nscal, fx.ion)          # every file indexes cleanly with the sizes predicted
    assert [[(s["rank"], s["disp"], s["nx"]) for s in dom] for dom in sources] == table
    for r in range(fx.nranks):                                             # the entry index: the Grid's place among its rank's Grids
        mine = sorted((n, s["entry"]) for n, dom in enumerate(sources) for s in dom if s["rank"] == r)
        assert [e for _n, e in mine] == list(range(len(mine)))
    if name == "blast2_noroot":
        assert sorted(s["rank"] for s in sources[0]) == [0, 1] and sorted(s["rank"] for s in sources[1]) == [2, 3]
    joined = fx.joined_seeds()
    for n, (Nx, dom) in enumerate(zip(fx.Nxs, sources)):
        for e in (False, True) if fx.ion else (False,):                    # every zone, and every face, from exactly one file
            dims = [v + e for v in Nx]
            cover = np.zeros(dims[::-1], dtype=int)
            for _src, _slo, dlo, ext in R.box_pieces(dom, Nx, (0, 0, 0), dims, e):
                cover[dlo[2]:dlo[2] + ext[2], dlo[1]:dlo[1] + ext[1], dlo[0]:dlo[0] + ext[0]] += 1
            assert np.all(cover == 1), (n, e)
        # the whole Domain and a box that straddles its Grids, against the numpy join
        for lo, nb in (((0, 0, 0), Nx), ((1, 2, 3), tuple(v - 3 for v in Nx))):
            U, ef = R.read_state_boxes(dom, Nx, lo, nb, fx.nscal)
            Uj, efj = joined[n]
            assert np.array_equal(bits(U), bits(Uj[lo[2]:lo[2] + nb[2], lo[1]:lo[1] + nb[1], lo[0]:lo[0] + nb[0]])), (n, lo)
            assert (ef is None) == (not fx.ion)
            if fx.ion:
                assert np.array_equal(bits(ef), bits(efj[lo[2]:lo[2] + nb[2] + 1, lo[1]:lo[1] + nb[1] + 1, lo[0]:lo[0] + nb[0] + 1])), (n, lo)


def test_mesh_grid_boxes_rules():
    R = pkg("restart")
    # the count runs on from Domain to Domain and wraps: 4 + 2 + 2 Grids on 4 ranks
    t = R.mesh_grid_boxes([((16, 24, 16), (1, 2, 2)), ((12, 16, 20), (1, 1, 2)), ((6, 8, 8), (1, 2, 1))], 4)
    assert [[b[0] for b in dom] for dom in t] == [[0, 1, 2, 3], [0, 1], [2, 3]]
    assert t[2][1][1:] == ((0, 4, 0), (6, 4, 8))
    # the whole remainder on the first Grid of a direction, in a refined Domain too
    assert [b[2][0] for b in R.mesh_grid_boxes([((8, 8, 8), (1, 1, 1)), ((23, 8, 8), (4, 1, 1))], 5)[1]] == [8, 5, 5, 5]
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected a number of files that divides the 8 Grids"):
        R.mesh_grid_boxes([((16, 12, 16), (2, 1, 2)), ((16, 12, 16), (1, 2, 2))], 5)
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected at least 4 files"):
        R.mesh_grid_boxes([((16, 12, 16), (2, 1, 2)), ((16, 12, 16), (1, 2, 2))], 2)
    assert R.mesh_nproc([(2, 1, 2), (1, 2, 2)]) == 4 and R.mesh_nproc([(1, 1, 2), (1, 1, 2)]) == 2
    assert R.mesh_nproc([(1, 1, 2), (1, 1, 2)], 4) == 4 and R.mesh_nproc([(1, 2, 2), (1, 1, 2), (1, 2, 1)]) == 4
    for bad in (3, 1, 8):
        with pytest.raises(ValueError):
            R.mesh_nproc([(1, 1, 2), (1, 1, 2)], bad)


# ---- 2. what is refused ----------------------------------------------------------------------------------------------------------
def test_wrong_files_are_refused(tmp_path):
    R = pkg("restart"); D = pkg("driver")
    fx = RMFixture("blast2_x1x3")
    scan = lambda seed, f=fx: R.scan_mesh_sources(seed, f.Nxs, f.nscal, f.ion)      # noqa: E731
    nr = RMFixture("blast2_noroot")
    # a number of files that does not divide the number of Grids: one missing (of 4 Grids on 4 ranks), and one too many
    seed = nr.write_seeds(str(tmp_path / "few"), skip=(3,))
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected a number of files that divides the 4 Grids of the mesh, found 3"):
        scan(seed, nr)
    seed = fx.write_seeds(str(tmp_path / "many"))
    extra = os.path.join(str(tmp_path / "many"), fx.seed_names[3].replace("id3", "id4"))
    os.makedirs(os.path.dirname(extra))
    open(extra, "wb").write(fx.seed_bytes(3))
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected a number of files that divides the 8 Grids of the mesh, found 5"):
        scan(seed)
    # a Domain with more Grids than files (the reference's first check, init_mesh.c:564-567): one file missing, two missing
    for skip in ((3,), (2, 3)):
        seed = fx.write_seeds(str(tmp_path / ("short%d" % len(skip))), skip=skip)
        with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected at least 4 files for the NGrid = 2 x 1 x 2 of Domain 0.*found %d" % (4 - len(skip))):
            scan(seed)
    # a count the rules allow, but not the one that wrote the files: 1x1x2 / 1x1x2 written on 4 ranks, two files present
    seed = nr.write_seeds(str(tmp_path / "half"), skip=(2, 3))
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected "):
        scan(seed, nr)
    # a file of another size: rank 1's replaced by rank 1's of other cuts, and a truncated one
    seed = fx.write_seeds(str(tmp_path / "size"))
    open(os.path.join(str(tmp_path / "size"), fx.seed_names[1]), "wb").write(nr.seed_bytes(1))
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected "):
        scan(seed)
    seed = fx.write_seeds(str(tmp_path / "cut"))
    open(os.path.join(str(tmp_path / "cut"), fx.seed_names[2]), "wb").write(fx.seed_bytes(2)[:-4000])
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected "):
        D.MeshDriver.from_restart(seed, engine_factory=OutputMeshEngine, regrid=True)
    # another mesh than the table's
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected 3 Domains"):
        R.scan_mesh_sources(fx.write_seeds(str(tmp_path / "doms")), fx.Nxs + [(8, 8, 8)], fx.nscal, fx.ion)


def test_single_level_regrid_still_refuses_a_refined_file(tmp_path):
    seed = RMFixture("blast2_x1x3").write_seeds(str(tmp_path / "seed"))
    with pytest.raises(pkg("restart").RestartError, match=r"num_domains = 2.*regrid"):
        pkg("driver").Driver.from_restart(seed, engine_factory=RestartOracleEngine, regrid=True)


def test_without_the_keyword_other_cuts_are_refused_as_before(tmp_path):
    seed = RMFixture("blast2_x1x3").write_seeds(str(tmp_path / "seed"))
    with pytest.raises(pkg("restart").RestartError, match=r"\[restart_grids\]: Expected "):
        pkg("driver").MeshDriver.from_restart(seed, engine_factory=OutputMeshEngine)


# ---- 3. MeshDriver resumed on other cuts: the reference's continued run, bit for bit -----------------------------------------------
def job_regrid(rank, world, seed, overrides, rundir, engine, cuts):
    """``-r seed overrides`` with regrid on this rank's slabs; the run to the table's nlim; the last dump read back without the keyword.
    engine: "oracle", or the `strict` of the HIP library"""
    D = pkg("driver")
    factory, strict = (OutputMeshEngine, None) if engine == "oracle" else (None, engine)
    d = D.MeshDriver.from_restart(seed, overrides, engine_factory=factory, rank=rank, nranks=world, device=0, strict=strict, cuts=cuts, regrid=True)
    assert d.restarted
    slabs = [(g.level, g.disp[2] - (d.domains[l].disp[2] if l else 0), g.Nx[2]) for l, g in enumerate(d.cfg.levels)]
    loaded = [d.eng.download(l)[4:-4, 4:-4, 4:-4].copy() for l in range(d.nl)]
    before = (d.time, d.dt, d.nstep)
    ngrid = pkg("restart").par_mesh_ngrid(d.par)
    auto = any(d.par.exist(f"domain{n}", "AutoWithNProc") for n in range(1, d.NL + 1))
    outs = pkg("outputs").OutputSet.from_par(d.par, d.time, rundir, rank, world)
    d.main(outs)
    final = [d.eng.download(l)[4:-4, 4:-4, 4:-4].copy() for l in range(d.nl)]
    if world > 1:
        d.dist.barrier()                    # rank 0's file is every rank's table
    last = max(int(p.rsplit(".", 2)[1]) for p in outs.written if p.endswith(".rst"))
    path0 = os.path.join(rundir, "id0" if world > 1 else "", "Blast.%04d.rst" % last)
    r = D.MeshDriver.from_restart(path0, engine_factory=factory, rank=rank, nranks=world, device=0, strict=strict, cuts=cuts)
    again = [r.eng.download(l)[4:-4, 4:-4, 4:-4].copy() for l in range(r.nl)]
    info = dict(slabs=slabs, loaded=loaded, before=before, ngrid=ngrid, auto=auto, final=final, again=again, niter=list(d.niter_trace),
                state=(d.time, d.dt, d.nstep), state_again=(r.time, r.dt, r.nstep))
    for e in (d.eng, r.eng):
        if hasattr(e, "close"):
            e.close()
    return info


def check_regrid_job(fx, res, world, exact=True, tol=None):
    """what every rank of job_regrid returned, against the fixture"""
    seeds, final = fx.joined_seeds(), fx.final()
    nv = 5 + fx.nscal
    for rank, r in enumerate(res):
        assert r["before"] == (fx.seed_time, fx.seed_dt, fx.seed_nstep)
        assert not r["auto"] and all(g[:2] == (1, 1) and 1 <= g[2] <= world for g in r["ngrid"]), r["ngrid"]
        assert r["state"][2] == fx.final_nstep == fx.nlim
        for (level, k0, n3), U0, U1, U2 in zip(r["slabs"], r["loaded"], r["final"], r["again"]):
            assert np.array_equal(bits(U0[..., :nv]), bits(seeds[level][0][k0:k0 + n3])), (rank, level)
            assert np.array_equal(bits(U2), bits(U1)), (rank, level)
            ref = final[level][0][k0:k0 + n3]
            if exact:
                assert np.array_equal(bits(U1[..., :nv]), bits(ref)), (rank, level)
            else:
                scale = np.abs(final[level][0]).max(axis=(0, 1, 2))
                assert np.all(U1[..., :nv][..., scale == 0] == 0)
                err = (np.abs(U1[..., :nv] - ref)[..., scale > 0] / scale[scale > 0]).max(axis=(0, 1, 2))
                print(f"{fx.name} rank {rank} level {level}: max error / field maximum {err}")
                assert err.max() < tol, (rank, level, err)
        if exact:
            assert r["state"] == (fx.final_time, fx.final_dt, fx.final_nstep)
        else:
            assert abs(r["state"][0] / fx.final_time - 1) < 1e-12 and abs(r["state"][1] / fx.final_dt - 1) < 1e-12
        assert r["state_again"] == r["state"]
    # the refined level lies on both ranks
    if world == 2:
        assert all(len(r["slabs"]) == len(fx.domains) for r in res)


@pytest.mark.parametrize("name", regridmeshfix.CONTINUED_BLAST)
def test_one_rank_resumes_from_seeds_of_other_cuts(name, tmp_path):
    fx = RMFixture(name)
    seed = fx.write_seeds(str(tmp_path / "seed"))
    res = [job_regrid(0, 1, seed, fx.resume_overrides, str(tmp_path / "run"), "oracle", None)]
    assert res[0]["ngrid"] == [(1, 1, 1)] * len(fx.domains)
    check_regrid_job(fx, res, 1)


@pytest.mark.parametrize("name", regridmeshfix.CONTINUED_BLAST)
def test_two_ranks_resume_from_seeds_of_other_cuts(name, tmp_path):
    fx = RMFixture(name)
    seed = fx.write_seeds(str(tmp_path / "seed"))
    res = meshfix.run_ranks(job_regrid, (seed, fx.resume_overrides, str(tmp_path / "run"), "oracle", CUTS[name]))
    assert all(r["ngrid"] == [(1, 1, 2)] * len(fx.domains) for r in res)
    check_regrid_job(fx, res, 2)


# ---- 4. written for other cuts, on the host path ---------------------------------------------------------------------------------
def split_write(d, rundir, fx):
    """the state of runner `d` written for fx's cuts under the seed's own number -> the files written"""
    outs = pkg("outputs").OutputSet.from_par(d.par, d.time, rundir, rst_mesh_ngrid=fx.ngrid, rst_mesh_nproc=fx.nranks)
    outs.rst.num -= 1                       # the table carries the NEXT number; the seed itself is this one
    d.write_restart(outs.rst, outs)
    return list(outs.written)


def test_split_dump_equals_the_reference_seeds(tmp_path):
    """the reference's 2x1x2 / 1x2x2 seeds joined on one rank, and written back without a step for those cuts and for 1x1x2 / 1x1x2
    on four ranks (ranks 2 and 3 without a root Grid): the bytes behind <par_end> are the files of BOTH seed sets (the generator
    asserted that the two join to the same bits)"""
    O = pkg("outputs")
    fx, nr = RMFixture("blast2_x1x3"), RMFixture("blast2_noroot")
    seed = fx.write_seeds(str(tmp_path / "seed"))
    d = pkg("driver").MeshDriver.from_restart(seed, engine_factory=OutputMeshEngine, regrid=True)
    for f in (fx, nr):
        rundir = str(tmp_path / f.name)
        regridmeshfix.check_split_files(f, rundir, split_write(d, rundir, f))
    # what is refused: more than one rank; a rank count the rules do not allow; cuts for another number of Domains; a 2-D mesh
    for kw in (dict(rank=0, nranks=2, rst_mesh_ngrid=fx.ngrid), dict(rst_mesh_ngrid=fx.ngrid, rst_mesh_nproc=3),
               dict(rst_mesh_ngrid=fx.ngrid, rst_mesh_nproc=2), dict(rst_mesh_ngrid=fx.ngrid[:1]), dict(rst_mesh_ngrid=[(2, 0, 1), (1, 1, 1)]),
               dict(rst_mesh_nproc=4)):
        with pytest.raises(ValueError):
            O.OutputSet.from_par(d.par, d.time, str(tmp_path / "no"), **kw)
    flat = meshfix.deck_par("blast2d_smr", [], {"1": {"out_fmt": "rst", "dt": "1"}})
    nd = flat.geti("job", "num_domains")
    with pytest.raises(ValueError, match="2-D"):
        O.OutputSet.from_par(flat, 0.0, str(tmp_path / "no"), rst_mesh_ngrid=[(1, 1, 1)] * nd)


# ---- 5. the reference takes the files -----------------------------------------------------------------------------------------------
def check_reference_takes_split_files(d, tmp_path):
    """runner `d` holds blast2_x1x3 as loaded: its state written for blast2_noroot's cuts (four ranks, two without a root Grid), the
    reference's own MPI + SMR build continued from those files to step 7, and its final files, joined by rules A to C: the
    fixture's final state bit for bit"""
    nr = RMFixture("blast2_noroot")
    rundir = str(tmp_path / "ours")
    written = split_write(d, rundir, nr)
    assert sorted(written) == sorted(nr.seed_names)
    finals = regridmeshfix.reference_continues([os.path.join(rundir, rel) for rel in nr.seed_names], nr.nlim, str(tmp_path / "ref"))
    assert [nr.head(b) for b in finals] == [(nr.final_nstep, nr.final_time, nr.final_dt)] * nr.nranks
    for (U, _), (Uf, _) in zip(nr.join_files(finals), nr.final()):
        assert np.array_equal(bits(U), bits(Uf))


@pytest.mark.skipif(not regridmeshfix.reference_available(), reason="oracle/_ref/athena_blast_smr_mpi or mpiexec not on this box")
def test_the_reference_continues_from_split_files_of_the_host_path(tmp_path):
    seed = RMFixture("blast2_x1x3").write_seeds(str(tmp_path / "seed"))
    d = pkg("driver").MeshDriver.from_restart(seed, engine_factory=OutputMeshEngine, regrid=True)
    check_reference_takes_split_files(d, tmp_path)
