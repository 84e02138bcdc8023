"""A refined run resumed on other cuts than those that wrote its restart dumps (``MeshRun.from_restart(..., regrid=True)``,
``MeshDriver.from_restart(..., regrid=True)``), and the restart dumps of a refined mesh written for other cuts
(``OutputSet.from_par(..., rst_mesh_ngrid=...)``), on an MI355X: the per-Domain boxes go to and from the resident levels through
aa_rst_section_put_box / _get_box (csrc/restart.hip), levels of a Mesh included.

Fixtures: tests/golden/regridmesh_*.npz (see test_regrid_mesh.py) -- four-rank seeds of the reference built with MPI and static
mesh refinement, every <domainN> cut by its own NGrid_x*, and its own continued runs.  Loading is exact in both libraries (no
arithmetic); the continued blast runs are exact in the strict library and within the project's hydro bars (1e-11 of each field's
maximum, 1e-12 in dt: test_gpu_parity.py, test_gpu_2d.py) in the default one; the sphere within the bars test_gpu_smr_slabs.py
holds between decompositions of this problem (1e-9 in d, E, s, 1e-4 in the momenta), with the reference's own sub-cycle counts.

The figures measured for the sphere stand in the docstring of its test and in DESIGN.md section 7."""
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
from test_regrid_mesh import CUTS, check_reference_takes_split_files, check_regrid_job, job_regrid, split_write      # noqa: E402

pytestmark = pytest.mark.gpu
TOL_U, TOL_DT = 1e-11, 1e-12          # default library, hydro


def active(U):
    return U[4:-4, 4:-4, 4:-4]


def resume(name, strict, tmp_path, continued=True, **kw):
    fx = RMFixture(name)
    seed = fx.write_seeds(str(tmp_path / "seed"))
    m = pkg("driver").MeshRun.from_restart(seed, fx.resume_overrides if continued and fx.continued else (), strict=strict, regrid=True, **kw)
    return fx, m


def check_loaded(fx, m):
    """every level as downloaded: the active zones are the joined seeds', EdgeFlux the join rule's, bit for bit"""
    assert m.restarted and (m.nstep, m.time, m.dt) == (fx.seed_nstep, fx.seed_time, fx.seed_dt)
    assert [g.cfg.Nx for g in m.mesh.lev] == fx.Nxs
    nv = 5 + fx.nscal
    for n, (g, (U, ef)) in enumerate(zip(m.mesh.lev, fx.joined_seeds())):
        assert np.array_equal(bits(active(g.download())[..., :nv]), bits(U)), n
        if fx.ion:
            assert np.array_equal(bits(g.download_edgeflux()), bits(ef)), n
    R = pkg("restart")
    assert R.par_mesh_ngrid(m.par) == [(1, 1, 1)] * len(fx.domains)
    assert not any(m.par.exist(f"domain{n + 1}", "AutoWithNProc") for n in range(len(fx.domains)))


def run_to_nlim(m, rundir):
    """outputs.run by hand, keeping the sub-cycle counts of every step -> (them, the OutputSet)"""
    outs = pkg("outputs").OutputSet.from_par(m.par, m.time, rundir)
    m.start()
    niter = []
    while m.time < m.run.tlim and m.nstep < m.run.nlim:
        outs.data_output(m, 0)
        niter.append(list(m.step()))
    outs.data_output(m, 1)
    return niter, outs


def errors(fx, m):
    """[nd][nvar] max |U - fixture's final| / the field's maximum, per Domain"""
    nv = 5 + fx.nscal
    out = []
    for g, (Uf, _ef) in zip(m.mesh.lev, fx.final()):
        U = active(g.download())[..., :nv]
        scale = np.abs(Uf).max(axis=(0, 1, 2))
        assert np.all(U[..., scale == 0] == 0)
        scale[scale == 0] = 1.0
        out.append(np.abs(U - Uf).max(axis=(0, 1, 2)) / scale)
    return np.array(out)


def check_final_blast(fx, m, strict):
    assert m.nstep == fx.final_nstep == fx.nlim
    if strict:
        assert (m.time, m.dt) == (fx.final_time, fx.final_dt)
        for n, (g, (Uf, _)) in enumerate(zip(m.mesh.lev, fx.final())):
            assert np.array_equal(bits(active(g.download())[..., :5]), bits(Uf)), n
    else:
        err = errors(fx, m)
        print(f"{fx.name} default library: max error / field maximum per Domain {err.max(axis=1)}")
        assert abs(m.time / fx.final_time - 1) < TOL_DT and abs(m.dt / fx.final_dt - 1) < TOL_DT
        assert err.max() < TOL_U, err


# ---- 1. load: every case, both libraries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", regridmeshfix.CASES)
def test_load_equals_the_joined_seeds(name, strict, tmp_path):
    fx, m = resume(name, strict, tmp_path)
    try:
        check_loaded(fx, m)
        if name == "blast2dom":
            assert m.mesh.domain_numbers() == [(0, 0), (1, 0), (1, 1)]
    finally:
        m.mesh.close()


# ---- 2. continued on one GPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", regridmeshfix.CONTINUED_BLAST)
def test_blast_continued_on_one_gpu(name, strict, tmp_path):
    D = pkg("driver")
    fx, m = resume(name, strict, tmp_path)
    try:
        _niter, outs = run_to_nlim(m, str(tmp_path / "run"))
        check_final_blast(fx, m, strict)
        # its own last dump -- one file, NGrid_x* = 1 in every <domainN> -- is read back without the keyword, to the same bits
        last = [p for p in outs.written if p.endswith(".rst")][-1]
        r = D.MeshRun.from_restart(os.path.join(str(tmp_path / "run"), last), strict=strict)
        try:
            assert (r.time, r.dt, r.nstep) == (m.time, m.dt, m.nstep)
            for a, b in zip(r.mesh.lev, m.mesh.lev):
                assert np.array_equal(bits(active(a.download())), bits(active(b.download())))
        finally:
            r.mesh.close()
    finally:
        m.mesh.close()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_sphere_continued_on_one_gpu(strict, tmp_path):
    """Measured on an MI355X at step 4, max error / field maximum over both levels (d, M1, M2, M3, E, s):
      strict  [9.6e-16, 1.6e-13, 1.3e-09, 6.3e-08, 2.2e-16, 9.2e-16]
      default [9.6e-16, 1.6e-13, 1.3e-09, 6.3e-08, 2.2e-16, 9.2e-16]      (M1: 1.6067e-13 against 1.6061e-13)
    beside D_ref, the reference's own spread between its 1x2x2 / 1x2x2 and 1x1x2 / 1x1x2 runs:
              [1.0e-15, 1.6e-13, 1.4e-09, 6.7e-08, 2.4e-16, 9.8e-16]
    and the sub-cycle counts of both steps are the fixture's, [4, 4]."""
    fx, m = resume("sphere2_x2x3", strict, tmp_path)
    try:
        niter, _outs = run_to_nlim(m, str(tmp_path / "run"))
        assert m.nstep == fx.final_nstep
        err = errors(fx, m)
        print(f"sphere2_x2x3 {'strict' if strict else 'default'}: sub-cycles {niter} (fixture {fx.niter}); max error / field maximum "
              f"{err.max(axis=0)}; D_ref {fx.z['D_ref'].max(axis=0)}; time / fixture's - 1 = {m.time / fx.final_time - 1:.2e}, "
              f"dt / fixture's - 1 = {m.dt / fx.final_dt - 1:.2e}")
        assert niter == fx.niter
        assert err[:, [0, 4, 5]].max() < 1e-9 and err[:, 1:4].max() < 1e-4, err
    finally:
        m.mesh.close()


# ---- 3. continued on two ranks: MeshDriver, both on one device ----------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_blast_continued_on_two_ranks(strict, tmp_path):
    """cuts (0, 6, 16): the refined level (root planes 4 .. 12) lies on both ranks, and no seed was cut there.  Every rank reads the
    boxes of its slabs, runs to step 7, and reads its own last dump back without the keyword (job_regrid)."""
    name = "blast2_x1x3"
    fx = RMFixture(name)
    seed = fx.write_seeds(str(tmp_path / "seed"))
    res = meshfix.run_ranks(job_regrid, (seed, fx.resume_overrides, str(tmp_path / "run"), strict, CUTS[name]))
    assert all(r["ngrid"] == [(1, 1, 2), (1, 1, 2)] for r in res)
    check_regrid_job(fx, res, 2, exact=strict, tol=TOL_U)


# ---- 4. slabs inside the library --------------------------------------------------------------------------------------------------------
def test_blast_loaded_and_continued_on_in_library_slabs(tmp_path):
    """the level handles are composites, which take whole sections only: a section is joined on the host and goes in whole"""
    fx, m = resume("blast2_x1x3", True, tmp_path, nslab=2)
    try:
        assert m.mesh.nslab == 2 and m.mesh.cuts is not None
        check_loaded(fx, m)
        run_to_nlim(m, str(tmp_path / "run"))
        check_final_blast(fx, m, True)
    finally:
        m.mesh.close()


# ---- 5. written for other cuts, from the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_split_dump_equals_the_reference_seeds(strict, tmp_path):
    """as test_regrid_mesh.py, the boxes coming from the device (rst_get_box per Grid): the payload of both seed sets"""
    fx, m = resume("blast2_x1x3", strict, tmp_path, continued=False)
    try:
        for f in (fx, RMFixture("blast2_noroot")):
            rundir = str(tmp_path / f.name)
            regridmeshfix.check_split_files(f, rundir, split_write(m, rundir, f))
    finally:
        m.mesh.close()


def test_sphere_split_dump_round_trip(tmp_path):
    """EDGEFLUX of both levels with its n + 1 faces per Grid, x1 cuts.  The seeds' own bytes cannot come back: where two Grids
    share a face, the seed files hold two entries for it, the join keeps the upper Grid's, and the lower Grid's is gone.  What
    holds: the files written for the seeds' cuts have the seeds' sizes, and join to the same state."""
    fx, m = resume("sphere2_x1", False, tmp_path)
    try:
        rundir = str(tmp_path / "run")
        written = split_write(m, rundir, fx)
        assert sorted(written) == sorted(fx.seed_names)
        for i, rel in enumerate(fx.seed_names):
            assert len(regridmeshfix.split_payload(open(os.path.join(rundir, rel), "rb").read())[1]) == len(regridmeshfix.split_payload(fx.seed_bytes(i))[1])
        r = pkg("driver").MeshRun.from_restart(os.path.join(rundir, fx.seed_names[0]), strict=False, regrid=True)
        try:
            check_loaded(fx, r)
        finally:
            r.mesh.close()
    finally:
        m.mesh.close()


# ---- 6. the reference takes our files -----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not regridmeshfix.reference_available(), reason="oracle/_ref/athena_blast_smr_mpi or mpiexec not on this box")
def test_the_reference_continues_from_split_files_of_the_device(tmp_path):
    fx, m = resume("blast2_x1x3", True, tmp_path, continued=False)
    try:
        check_reference_takes_split_files(m, tmp_path)
    finally:
        m.mesh.close()


# ---- 7. what is refused ---------------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path):
    D = pkg("driver"); O = pkg("outputs"); R = pkg("restart")
    # a 2-D mesh: its own dump is read as before, and refused under regrid and rst_mesh_ngrid
    par = meshfix.deck_par("blast2d_smr", ["time/nlim=1"], {"1": {"out_fmt": "rst", "dt": "1e300"}})
    run = pkg("config").from_par(par, "blast")
    nd = par.geti("job", "num_domains")
    m = D.MeshRun(pkg("lib").Mesh(pkg("config").levels_2d(par, run), 0, True), run)
    try:
        outs = O.OutputSet.from_par(par, 0.0, str(tmp_path / "flat"))
        m.start()
        outs.data_output(m, 1)
        flat = os.path.join(str(tmp_path / "flat"), outs.written[-1])
    finally:
        m.mesh.close()
    r = D.MeshRun.from_restart(flat, [], "blast", strict=True)
    r.mesh.close()
    with pytest.raises(R.RestartError, match="2-D"):
        D.MeshRun.from_restart(flat, [], "blast", strict=True, regrid=True)
    with pytest.raises(ValueError, match="2-D"):
        O.OutputSet.from_par(par, 0.0, str(tmp_path / "no"), rst_mesh_ngrid=[(1, 1, 1)] * nd)
    # rst_mesh_ngrid on two ranks; on a Mesh cut into slabs inside the library
    fx, m = resume("blast2_x1x3", True, tmp_path, nslab=2)
    try:
        with pytest.raises(ValueError, match="one-rank"):
            O.OutputSet.from_par(m.par, m.time, str(tmp_path / "no"), 0, 2, rst_mesh_ngrid=fx.ngrid)
        with pytest.raises(ValueError, match="slabs inside the library"):
            split_write(m, str(tmp_path / "no"), fx)
    finally:
        m.mesh.close()
    # without the keyword the seeds of other cuts are refused as before
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected "):
        D.MeshRun.from_restart(fx.write_seeds(str(tmp_path / "again")), strict=True)
