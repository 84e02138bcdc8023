"""Resuming a run on another decomposition than the one that wrote the restart dumps (``Driver.from_restart(..., regrid=True)``),
and writing restart dumps for other cuts (``OutputSet.from_par(..., rst_ngrid=...)``), on the CPU.

Fixtures: tests/golden/regrid_*.npz (tests/golden/make_golden_regrid.py) -- seeds of the reference's MPI executables on
NGrid = 2 x 1 x 2, 4 x 1 x 2 (uneven: 7, 5, 5, 5 zones along x1 and 5, 4 along x3) and 2 x 2 x 1 (ion radiation), x1 cuts among
them -- and the restart_*.npz fixtures of test_restart_resume.py.  Everything is exact: the reference's one-rank and two-rank
runs of the blast deck agree bit for bit, so a run resumed on other cuts leaves the very tree the other fixture holds."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import regridfix                                       # noqa: E402
import restartfix                                      # noqa: E402
from dumpfix import pkg                                # noqa: E402
from regridfix import GFixture, bits                   # noqa: E402
from restartfix import RFixture                        # noqa: E402
from test_distributed_gloo import _free_port           # noqa: E402
from test_restart_resume import RestartOracleEngine    # noqa: E402

ONE, MPI2, X1X3 = "restart_blast_16x12x8_s3_s8", "restart_blast_mpi2_16x12x8_s3_s8", "regrid_blast_x1x3_16x12x8_s3_s8"


# ---- 1. the Grids of a decomposition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", regridfix.FIXTURES)
def test_grid_boxes_against_the_vtk_headers(name):
    """sizes, displacements and rank order as the reference's ranks state them in their own vtk files"""
    fx = GFixture(name)
    boxes = pkg("restart").grid_boxes(fx.nx, fx.ngrid)
    assert [b[0] for b in boxes] == list(range(fx.nranks))
    assert [(b[1], b[2]) for b in boxes] == fx.vtk_boxes()


def test_grid_boxes_puts_the_whole_remainder_on_the_first_grid():
    R = pkg("restart")
    b = R.grid_boxes((22, 12, 9), (4, 1, 2))
    assert [x[2][0] for x in b[:4]] == [7, 5, 5, 5] and [x[1][0] for x in b[:4]] == [0, 7, 12, 17]
    assert [b[0][2][2], b[4][2][2]] == [5, 4] and b[4][1] == (0, 0, 5)
    assert [x[2][0] for x in R.grid_boxes((23, 8, 8), (4, 1, 1))] == [8, 5, 5, 5]          # NOT 6, 6, 6, 5
    assert R.grid_boxes((16, 12, 8), (2, 2, 1))[2] == (2, (0, 6, 0), (8, 6, 8))            # x1 fastest, then x2
    with pytest.raises(R.RestartError):
        R.grid_boxes((16, 12, 8), (0, 1, 1))


# ---- 2. resumed on other cuts: the other fixture's tree, bit for bit --------------------------------------------------------
@pytest.mark.parametrize("seeds", [MPI2, X1X3])
def test_one_rank_resumes_from_the_seeds_of_other_cuts(seeds, tmp_path):
    fx = RFixture(ONE)
    src = RFixture(seeds) if seeds == MPI2 else GFixture(seeds)
    seed = src.write_seeds(str(tmp_path / "seed"))
    d = pkg("driver").Driver.from_restart(seed, fx.resume_overrides, engine_factory=RestartOracleEngine, regrid=True)
    assert d.restarted and (d.nstep, d.time, d.dt) == (fx.seed_nstep, fx.seed_time, fx.seed_dt)
    assert [d.par.geti("domain1", f"NGrid_x{k}") for k in (1, 2, 3)] == [1, 1, 1] and not d.par.exist("domain1", "AutoWithNProc")
    rundir = str(tmp_path / "run")
    d.main(pkg("outputs").OutputSet.from_par(d.par, d.time, rundir))
    assert d.nstep == fx.nlim
    restartfix.compare_resumed_tree(fx, rundir)
    # the dump describes itself: it is read back without the keyword
    last = [p for p in fx.paths if p.endswith(".rst")][-1]
    assert pkg("restart").par_ngrid(pkg("restart").read_head(os.path.join(rundir, last))["par"]) == (1, 1, 1)
    r = pkg("driver").Driver.from_restart(os.path.join(rundir, last), engine_factory=RestartOracleEngine)
    assert np.array_equal(bits(r.eng.download()[4:-4, 4:-4, 4:-4]), bits(d.eng.download()[4:-4, 4:-4, 4:-4]))


def test_without_the_keyword_other_cuts_are_refused_as_before(tmp_path):
    seed = RFixture(MPI2).write_seeds(str(tmp_path / "seed"))
    with pytest.raises(pkg("restart").RestartError, match=r"\[restart_grids\]: Expected "):
        pkg("driver").Driver.from_restart(seed, engine_factory=RestartOracleEngine)


def _rank_main(rank, world, port, seed, rundir, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    d = pkg("driver").Driver.from_restart(seed, (), engine_factory=RestartOracleEngine, rank=rank, nranks=world, regrid=True)
    outs = pkg("outputs").OutputSet.from_par(d.par, d.time, rundir, rank, world)
    d.main(outs)
    q.put((rank, d.nstep, outs.basename, [d.par.geti("domain1", f"NGrid_x{k}") for k in (1, 2, 3)]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_resume_from_the_one_rank_seed(tmp_path):
    import torch.multiprocessing as mp
    fx = RFixture(MPI2)
    seed = RFixture(ONE).write_seeds(str(tmp_path / "seed"))
    rundir = str(tmp_path / "run")
    ctx = mp.get_context("spawn")
    q = ctx.Queue(); port = _free_port()
    ps = [ctx.Process(target=_rank_main, args=(r, 2, port, seed, rundir, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(0, fx.nlim, "Blast", [1, 1, 2]), (1, fx.nlim, "Blast-id1", [1, 1, 2])]
    restartfix.compare_resumed_tree(fx, rundir)


# ---- 3. the join, and what is refused ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["regrid_blast_uneven_22x12x9_s3_s6", "regrid_ioniz_sphere_x1x2_24x20x16_s6_s10"])
def test_read_state_boxes_equals_a_numpy_join(name, tmp_path):
    R = pkg("restart")
    fx = GFixture(name)
    seed = fx.write_seeds(str(tmp_path / "seed"), by_rank=True)
    sources = R.scan_sources(seed, fx.nx, fx.nscal, fx.ion)
    assert [(s["rank"], s["disp"], s["nx"]) for s in sources] == [(r, b[0], b[1]) for r, b in enumerate(fx.vtk_boxes())]
    states = fx.seed_states(str(tmp_path))
    # the whole Domain, the Grids of this package's own cuts (x3 slabs, x2 x x3 pencils), and a box inside one source Grid
    dests = [((0, 0, 0), fx.nx)] + [(b[1], b[2]) for ng in ((1, 1, 2), (1, 2, 2), (1, 3, 1)) for b in R.grid_boxes(fx.nx, ng)]
    dests.append(((1, 2, 1), (3, 2, 2)))
    for lo, n in dests:
        U, ef = R.read_state_boxes(sources, fx.nx, lo, n, fx.nscal)
        Uj, efj = regridfix.join(states, fx.vtk_boxes(), fx.nx, lo, n)
        assert np.array_equal(bits(U), bits(Uj)), (lo, n)
        assert (ef is None) == (not fx.ion) and (ef is None or np.array_equal(bits(ef), bits(efj))), (lo, n)
    # every zone and every face comes from exactly one file
    for e in (False, True):
        cover = np.zeros([v + e for v in fx.nx][::-1], dtype=int)
        for _src, _slo, dlo, ext in R.box_pieces(sources, fx.nx, (0, 0, 0), [v + e for v in fx.nx], e):
            cover[dlo[2]:dlo[2] + ext[2], dlo[1]:dlo[1] + ext[1], dlo[0]:dlo[0] + ext[0]] += 1
        assert np.all(cover == 1)


def test_wrong_files_are_refused(tmp_path):
    R = pkg("restart"); D = pkg("driver")
    fx = GFixture(X1X3)
    # a file missing, and one too many
    seed = fx.write_seeds(str(tmp_path / "few"), skip=(3,))
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected 4 files"):
        R.scan_sources(seed, fx.nx, fx.nscal, fx.ion)
    seed = fx.write_seeds(str(tmp_path / "many"))
    open(os.path.join(os.path.dirname(seed), "Blast-id4.0001.rst"), "wb").write(fx.seed_bytes(3))
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected 4 files"):
        R.scan_sources(seed, fx.nx, fx.nscal, fx.ion)
    # a file of another size: rank 1's replaced by one of the uneven run (another box), and a truncated one
    seed = fx.write_seeds(str(tmp_path / "size"))
    open(os.path.join(os.path.dirname(seed), "Blast-id1.0001.rst"), "wb").write(GFixture("regrid_blast_uneven_22x12x9_s3_s6").seed_bytes(1))
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected "):
        R.scan_sources(seed, fx.nx, fx.nscal, fx.ion)
    seed = fx.write_seeds(str(tmp_path / "cut"))
    open(os.path.join(os.path.dirname(seed), "Blast-id2.0001.rst"), "wb").write(fx.seed_bytes(2)[:-4000])
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected "):
        D.Driver.from_restart(seed, engine_factory=RestartOracleEngine, regrid=True)
    # a file of a refined mesh
    smr = RFixture("restart_blast_smr_16x12x8_s2_s5").write_seeds(str(tmp_path / "smr"))
    with pytest.raises(R.RestartError, match=r"num_domains = 2.*regrid"):
        D.Driver.from_restart(smr, engine_factory=RestartOracleEngine, regrid=True)


# ---- 4. written for other cuts ---------------------------------------------------------------------------------------------------
def test_split_dump_equals_the_reference_seeds(tmp_path):
    """the reference's 2 x 1 x 2 seeds read, and written back for 2 x 1 x 2 without a step: the bytes behind <par_end> are the seed
    files', the tables agree as parsed in NGrid_x*, problem_id, every block's num and <time> time"""
    A = pkg("athinput"); O = pkg("outputs")
    fx = GFixture(X1X3)
    seed = fx.write_seeds(str(tmp_path / "seed"))
    d = pkg("driver").Driver.from_restart(seed, engine_factory=RestartOracleEngine, regrid=True)
    rundir = str(tmp_path / "run")
    outs = O.OutputSet.from_par(d.par, d.time, rundir, rst_ngrid=fx.ngrid)
    outs.rst.num -= 1                       # the table carries the NEXT number; the seed itself is this one
    d.write_restart(outs.rst, outs)
    assert sorted(outs.written) == sorted(fx.seed_names)
    for i, rel in enumerate(fx.seed_names):
        head, payload = regridfix.split_payload(open(os.path.join(rundir, rel), "rb").read())
        rhead, rpayload = regridfix.split_payload(fx.seed_bytes(i))
        assert payload == rpayload, rel
        a, b = A.ParTable.from_text(head), A.ParTable.from_text(rhead)
        for k in (1, 2, 3):
            assert a.geti("domain1", f"NGrid_x{k}") == b.geti("domain1", f"NGrid_x{k}") == fx.ngrid[k - 1]
            assert a.geti(f"output{k}", "num") == b.geti(f"output{k}", "num") and a.getd(f"output{k}", "time") == b.getd(f"output{k}", "time")
        assert a.gets("job", "problem_id") == b.gets("job", "problem_id") == "Blast" + ("-id%d" % i if i else "")
        assert a.getd("time", "time") == b.getd("time", "time")
    with pytest.raises(ValueError):
        O.OutputSet.from_par(d.par, d.time, rundir, 0, 2, rst_ngrid=(2, 1, 2))
