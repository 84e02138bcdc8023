"""Outputs, history and restart of driver.MeshDriver on the device path: two ranks (both on cuda:0, messages staged through the
host because gloo moves host tensors, as in test_gpu_smr_slabs.py) with the HIP engine -- the dump payloads (csrc/dump.hip), the
history sums (aa_history) and the restart sections (csrc/restart.hip) of slab Grids of a refined level.

Against the reference's two-rank trees (tests/golden/meshdrv_*.npz, see test_mesh_driver_outputs.py) in the strict library, bit
for bit; against this package's own uninterrupted runs in both libraries, bit for bit; against the one-process MeshRun dumps,
plane by plane; and the radiation sphere against the reference's resumed run within the bars of test_gpu_restart.py."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dumpfix                                         # noqa: E402
import meshfix                                         # noqa: E402
from dumpfix import pkg                                # noqa: E402
from meshfix import MFixture                           # noqa: E402
from restartfix import tree                            # noqa: E402
from test_distributed_smr_gloo import BLAST_ALIGNED    # noqa: E402
from test_mesh_driver_outputs import BLAST, BLAST_RESUMED, STEADY, job_resume, job_run, resume_equals_full      # noqa: E402

pytestmark = pytest.mark.gpu
SPHERE = "meshdrv_restart_ioniz_sphere_mpi2"


# ---- 6. the reference's trees, strict library ------------------------------------------------------------------------------------
def test_main_leaves_the_reference_tree(tmp_path):
    fx = MFixture(BLAST)
    rundir = str(tmp_path / "run")
    res = meshfix.run_ranks(job_run, (dict(fixture=BLAST), rundir, True, None))
    assert [r["basename"] for r in res] == ["Blast", "Blast-id1"] and all(r["nstep"] == fx.nlim for r in res)
    meshfix.compare_tree(fx, rundir)


@pytest.mark.parametrize("by_rank", [False, True])
def test_resume_from_the_reference_seeds_leaves_its_resumed_tree(by_rank, tmp_path):
    fx = MFixture(BLAST_RESUMED)
    seed = fx.write_seeds(str(tmp_path / "seed"), by_rank=by_rank)
    rundir = str(tmp_path / "run")
    res = meshfix.run_ranks(job_resume, (seed, fx.resume_overrides, rundir, True, None))
    assert [(r["basename"], r["nstep"]) for r in res] == [("Blast", fx.nlim), ("Blast-id1", fx.nlim)]
    assert all(r["before"] == (fx.seed_time, fx.seed_dt, fx.seed_nstep) for r in res)
    meshfix.compare_tree(fx, rundir)
    for rel in ("id0/Blast.hst", "id0/lev1/Blast-lev1.hst"):
        assert not open(os.path.join(rundir, rel)).read().startswith("#")


# ---- 7. our own files: resumed equals uninterrupted, both libraries -----------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True])
def test_resumed_from_our_own_files_equals_the_uninterrupted_run(strict, tmp_path):
    resume_equals_full(STEADY, None, strict, 1, tmp_path)


# ---- 8. the payload of slab Grids against the one-process MeshRun ---------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [None, (0, 4, 16)])
def test_slab_dumps_are_the_planes_of_the_one_process_dumps(cuts, tmp_path):
    """strict library, blast with level 1 over root planes 4 .. 12; cuts = (0, 4, 16): the level begins exactly at the cut, so the
    flux correction of root plane 3 crosses it.  Every section of a rank's file is the x3 planes of its slab in the MeshRun file
    of that level, byte for byte (MeshRun's dumps are pinned to the reference by test_gpu_dumps.py)."""
    blocks = {"1": {"out_fmt": "vtk", "out": "prim", "dt": "0.004"}, "2": {"out_fmt": "bin", "dt": "0.004"}}
    spec = dict(problem="blast", overrides=list(BLAST_ALIGNED) + ["time/nlim=3"], blocks=blocks)
    par = meshfix.deck_par(spec["problem"], spec["overrides"], spec["blocks"])
    run = pkg("config").from_par(par, "blast")
    whole = pkg("config").levels(par, run)
    one_dir, two_dir = str(tmp_path / "one"), str(tmp_path / "two")
    mesh = pkg("lib").Mesh(whole, 0, True)
    try:
        one = pkg("driver").MeshRun(mesh, run)
        one.main(pkg("outputs").OutputSet.from_par(par, 0.0, one_dir))
        nstep_one = one.nstep
    finally:
        mesh.close()
    res = meshfix.run_ranks(job_run, (spec, two_dir, True, cuts))
    assert nstep_one == 3 and all(r["nstep"] == 3 for r in res)
    seen = grids = 0
    for rank in (0, 1):
        slabs = pkg("config").mesh_slabs(par, run, rank, 2, cuts).levels
        base = "Blast" if rank == 0 else "Blast-id1"
        for g in slabs:
            l = g.level
            grids += 1
            k0 = g.disp[2] - (whole[l].disp[2] if l else 0)
            for ext, prim in (("vtk", True), ("bin", False)):
                nums = sorted(int(p.rsplit(".", 2)[1]) for p in tree(one_dir) if p.endswith("." + ext) and ("lev1" in p) == (l == 1))
                assert len(nums) >= 3
                for num in nums:
                    a = open(os.path.join(two_dir, f"id{rank}", pkg("dumps").fname(base, l, 0, num, ext)), "rb").read()
                    b = open(os.path.join(one_dir, pkg("dumps").fname("Blast", l, 0, num, ext)), "rb").read()
                    sa = dumpfix.sections(a, g.Nx, 0, ext, prim); sb = dumpfix.sections(b, whole[l].Nx, 0, ext, prim)
                    plane = g.Nx[0] * g.Nx[1]
                    for (oa, na), (ob, nb) in zip(sa, sb):
                        w = 4 * (na // (plane * g.Nx[2])) * plane            # bytes of one x3 plane of this section
                        assert na == (w // 4) * g.Nx[2] and nb == (w // 4) * whole[l].Nx[2]
                        assert a[oa:oa + 4 * na] == b[ob + w * k0:ob + w * (k0 + g.Nx[2])], (rank, l, ext, num)
                        seen += 1
    assert grids == (4 if cuts is None else 3) and seen == grids * (3 + 5) * len(nums)       # (cuts (0, 4, 16): rank 0 holds the root only)


# ---- 9. the radiation sphere, both libraries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True])
def test_sphere_resumed_from_the_reference_seeds(strict, tmp_path):
    """Both levels sub-cycle (4 iterations each in both stored steps, asserted when the fixture was made).  The sub-cycle counts
    are the fixture's; restart-dump fields within 1e-9 of each field's maximum in the strict library and 1e-8 in the default
    one, time and dt to 1e-12 (the bars of test_gpu_restart.py); dumps by size; .hst rows with the net momenta to 1e-2 of the
    largest (the bar of test_history.py for this problem)."""
    fx = MFixture(SPHERE)
    seed = fx.write_seeds(str(tmp_path / "seed"))
    rundir = str(tmp_path / "run")
    res = meshfix.run_ranks(job_resume, (seed, fx.resume_overrides, rundir, strict, None))
    for r in res:
        print("sub-cycles", r["niter"], "fixture", fx.niter)
        assert r["nstep"] == fx.nlim and r["before"][2] == fx.seed_nstep
        assert r["niter"] == fx.niter
    meshfix.compare_tree(fx, rundir, tol=1e-9 if strict else 1e-8, mom_rtol=1e-2)
