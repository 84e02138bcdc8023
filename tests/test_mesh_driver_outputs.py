"""Outputs, history and restart of driver.MeshDriver (static mesh refinement over several ranks), on the CPU: two ranks over gloo
with the oracle as the per-rank engine (test infrastructure).

Fixtures: tests/golden/meshdrv_*.npz -- two-rank runs of the UNMODIFIED reference built with MPI and static mesh refinement
(tests/golden/make_golden_meshdriver.py): the tree of an uninterrupted blast run with rst, vtk, hst and bin blocks, and the tree
a run resumed with ``-r`` left.  Blast on the oracle is bit for bit, so what is tested is the layer above the engine: one file
per level and rank with the slab's own header, history summed over the ranks of a level and written by the lowest of them under
id0/, one restart file per rank holding several Grids, the reader, and the start sequence of a restarted run."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import meshfix                                         # noqa: E402
from dumpfix import pkg                                # noqa: E402
from meshfix import MFixture                           # noqa: E402
from restartfix import parse_hst, tree                 # noqa: E402
from test_distributed_smr_gloo import OracleMeshEngine, dom      # noqa: E402
from test_history import check_rows                    # noqa: E402

BLAST, BLAST_RESUMED = "meshdrv_blast_mpi2_s4", "meshdrv_restart_blast_mpi2_s3_s7"
# root 12x12x24, level 1 over root planes 4 .. 12: with the cut at plane 12 rank 1 holds no zones of level 1, and the flux
# correction of root plane 12 (outside the level's upper boundary) crosses the cut
LONE = dict(problem="blast", overrides=["job/num_domains=2", "time/nlim=7"] + dom(1, (12, 12, 24)) + dom(2, (12, 12, 16), (6, 6, 8)),
            blocks={"1": {"out_fmt": "rst", "dt": "0.008"}, "2": {"out_fmt": "vtk", "dt": "0.008"}, "3": {"out_fmt": "hst", "dt": "0.004"}})
LONE_CUTS = (0, 12, 24)
# The blast fixture's deck with output intervals LONGER than a step (about 0.003).  With shorter ones a block's next time lags
# behind the run, the pass of the loop that wrote the seed fires again after the resume (in the reference too: the resumed
# fixture holds it), and the resumed run's numbers run ahead of the uninterrupted run's.
STEADY = dict(fixture=BLAST, overrides=["time/nlim=8", "output1/dt=0.008", "output2/dt=0.008", "output3/dt=0.004", "output4/dt=0.012"])


def history_in_order(U_active, dx, nscal):
    """dump_history.c:171-202: the sums zone by zone in the reference's order (cumsum adds one zone after the other)"""
    dVol = 1.0
    for a in range(3):
        dVol *= dx[a]
    U = U_active.reshape(-1, U_active.shape[-1])
    d, M1, M2, M3, E = (U[:, c] for c in range(5))
    d1 = 1.0 / d
    terms = [dVol * d, dVol * E, dVol * M1, dVol * M2, dVol * M3,
             dVol * 0.5 * (M1 * M1) * d1, dVol * 0.5 * (M2 * M2) * d1, dVol * 0.5 * (M3 * M3) * d1,
             dVol * U[:, 5] if nscal else 0.0 * d]
    return np.array([np.cumsum(t)[-1] for t in terms])


class OutputMeshEngine(OracleMeshEngine):
    """OracleMeshEngine with the optional engine methods of MeshDriver's writers and of from_restart"""

    def history(self, l):
        s = self.lev[l]; run = s.grid.run
        return history_in_order(s.active, [run.dx[a] / float(1 << s.grid.level) for a in range(3)], run.nscal)

    def edgeflux(self, l):
        return self.lev[l].edgeflux.copy()

    def load_state(self, l, U_active, edgeflux):
        s = self.lev[l]
        s.active[..., :U_active.shape[-1]] = U_active
        if edgeflux is not None:
            s.edgeflux[...] = edgeflux


# ---- what a rank does (module level: spawn finds them by name).  engine: "oracle", or the `strict` of the HIP library --------
def _factory(engine):
    return (OutputMeshEngine, None) if engine == "oracle" else (None, engine)


def _spec_par(spec):
    if "fixture" in spec:
        return MFixture(spec["fixture"]).par().cmdline(list(spec.get("overrides", ())))
    return meshfix.deck_par(spec["problem"], spec["overrides"], spec["blocks"])


def _finish(d, outs, extra=()):
    info = dict(time=d.time, dt=d.dt, nstep=d.nstep, basename=outs.basename, written=list(outs.written), niter=list(d.niter_trace),
                nl=d.nl, U=[d.eng.download(l)[4:-4, 4:-4, 4:-4].copy() for l in range(d.nl)], **dict(extra))
    if hasattr(d.eng, "close"):
        d.eng.close()
    return info


def job_run(rank, world, spec, rundir, engine, cuts):
    """an uninterrupted run of the deck `spec` to its nlim, with its <outputN> blocks"""
    par = _spec_par(spec)
    run = pkg("config").from_par(par, spec.get("problem"))
    factory, strict = _factory(engine)
    d = pkg("driver").MeshDriver(par, run, factory, rank, world, device=0, strict=strict, cuts=cuts)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, rundir, rank, world)
    d.main(outs)
    return _finish(d, outs)


def job_resume(rank, world, seed, overrides, rundir, engine, cuts):
    """``-r seed overrides``"""
    factory, strict = _factory(engine)
    d = pkg("driver").MeshDriver.from_restart(seed, overrides, engine_factory=factory, rank=rank, nranks=world, device=0, strict=strict,
                                              cuts=cuts)
    assert d.restarted and d.par is not None
    before = (d.time, d.dt, d.nstep)
    d.start()
    assert (d.time, d.dt, d.nstep) == before and d.dtl == [d.dt] * d.NL      # no new_dt: the file's dt is the next step's
    outs = pkg("outputs").OutputSet.from_par(d.par, d.time, rundir, rank, world)
    d.main(outs)
    return _finish(d, outs, dict(before=before))


def job_refused(rank, world, seed, cuts):
    try:
        pkg("driver").MeshDriver.from_restart(seed, engine_factory=OutputMeshEngine, rank=rank, nranks=world, cuts=cuts)
    except pkg("restart").RestartError as e:
        return str(e)
    return "read"


def resume_equals_full(spec, cuts, engine, seed_num, tmp_path, base="Blast"):
    """run to nlim, resume from our own restart dumps number `seed_num` (as the ranks wrote them), compare; -> both results"""
    full, res = str(tmp_path / "full"), str(tmp_path / "resumed")
    a = meshfix.run_ranks(job_run, (spec, full, engine, cuts))
    seed = os.path.join(full, "id0", "%s.%04d.rst" % (base, seed_num))
    b = meshfix.run_ranks(job_resume, (seed, [], res, engine, cuts))
    for ra, rb in zip(a, b):
        assert 0 < rb["before"][2] < ra["nstep"]
        assert (rb["time"], rb["dt"], rb["nstep"]) == (ra["time"], ra["dt"], ra["nstep"])
        assert rb["nl"] == ra["nl"] and all(np.array_equal(x, y) for x, y in zip(ra["U"], rb["U"]))
    meshfix.compare_resumed_with_full(full, res, seed)
    return a, b, full


# ---- 1. the reference's tree ------------------------------------------------------------------------------------------------
def test_main_leaves_the_reference_tree(tmp_path):
    fx = MFixture(BLAST)
    rundir = str(tmp_path / "run")
    res = meshfix.run_ranks(job_run, (dict(fixture=BLAST), rundir, "oracle", None))
    assert [r["basename"] for r in res] == ["Blast", "Blast-id1"] and all(r["nstep"] == fx.nlim for r in res)
    meshfix.compare_tree(fx, rundir)
    # the slabs are the reference's Grids: root planes 0-7 / 8-15, level-1 planes 8-15 / 16-23
    g = fx.grids()
    assert [(g[(r, l)].disp[2], g[(r, l)].Nx[2]) for r in (0, 1) for l in (0, 1)] == [(0, 8), (8, 8), (8, 8), (16, 8)]
    # history goes under id0/ only, level 1 with the writer's problem_id; `written` of the writer names it
    assert [p for p in fx.paths if p.endswith(".hst")] == ["id0/Blast.hst", "id0/lev1/Blast-lev1.hst"]
    assert "Blast.hst" in res[0]["written"] and "lev1/Blast-lev1.hst" in res[0]["written"]
    assert not any(w.endswith(".hst") for w in res[1]["written"])
    par = fx.par(); run = fx.run_config(par)
    whole = pkg("config").levels(par, run)[1]
    vol = float(np.prod([whole.Nx[a] * run.dx[a] / 2.0 for a in range(3)]))
    line = open(os.path.join(rundir, "id0", "lev1", "Blast-lev1.hst")).readline()
    assert line == "# Athena history dump for level=1 domain=0 volume=%e\n" % vol, line      # the whole Domain of level 1, not the slab


# ---- 2. resumed from the reference's seeds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_rank", [False, True])
def test_resume_from_the_reference_seeds_leaves_its_resumed_tree(by_rank, tmp_path):
    fx = MFixture(BLAST_RESUMED)
    seed = fx.write_seeds(str(tmp_path / "seed"), by_rank=by_rank)
    rundir = str(tmp_path / "run")
    res = meshfix.run_ranks(job_resume, (seed, fx.resume_overrides, rundir, "oracle", None))
    assert [(r["basename"], r["nstep"]) for r in res] == [("Blast", fx.nlim), ("Blast-id1", fx.nlim)]
    assert all(r["before"] == (fx.seed_time, fx.seed_dt, fx.seed_nstep) for r in res)
    meshfix.compare_tree(fx, rundir)
    got = tree(rundir)
    # no file of a forced first output (the seed was number 0002), the numbering continues, rows only in the .hst files
    assert not any(".0002.rst" in p or ".0002.vtk" in p or ".0000." in p for p in got)
    assert sorted(fx.where(p)[2] for p in got if p.startswith("id1/") and p.endswith(".rst")) == [3, 4, 5]
    assert sorted(fx.where(p)[2] for p in got if p.startswith("id0/lev1/") and p.endswith(".bin")) == [1, 2]
    for rel in ("id0/Blast.hst", "id0/lev1/Blast-lev1.hst"):
        assert not open(os.path.join(rundir, rel)).read().startswith("#")


# ---- 3. our own files: resumed equals uninterrupted ---------------------------------------------------------------------------
def test_resumed_from_our_own_files_equals_the_uninterrupted_run(tmp_path):
    resume_equals_full(STEADY, None, "oracle", 1, tmp_path)


# ---- 4. a rank without zones of the refined level --------------------------------------------------------------------------------
class _OracleMeshForMeshRun:
    """what driver.MeshRun asks of a Mesh for its history, on the oracle's one-process Mesh"""

    class _Level:
        def __init__(self, sim): self.sim, self.cfg = sim, sim.grid

        def history(self):
            run = self.cfg.run
            return history_in_order(self.sim.active, [run.dx[a] / float(1 << self.cfg.level) for a in range(3)], run.nscal)

    def __init__(self, mesh):
        self.m = mesh
        self.lev = [self._Level(s) for s in mesh.lev]

    time = property(lambda s: s.m.time)
    dt = property(lambda s: s.m.dt)
    nstep = property(lambda s: s.m.nstep)

    def state(self): return self.m.time, self.m.dt, self.m.nstep
    def domain_numbers(self): return [(l, 0) for l in range(len(self.lev))]
    def start(self): self.m.start()
    def step(self): return self.m.step()


def test_a_rank_without_the_refined_level(tmp_path):
    import orc
    a, _b, full = resume_equals_full(LONE, LONE_CUTS, "oracle", 1, tmp_path)
    assert [r["nl"] for r in a] == [2, 1]
    got = tree(full)
    assert any(p.startswith("id0/lev1/") for p in got) and not any(p.startswith("id1/lev1") for p in got)
    # rank 1's restart dump holds one Grid, rank 0's two: the reader takes exactly those sizes
    R = pkg("restart")
    R.scan_rst(os.path.join(full, "id1", "Blast-id1.0001.rst"), [(12, 12, 12)], 0, False)
    R.scan_rst(os.path.join(full, "id0", "Blast.0001.rst"), [(12, 12, 12), (12, 12, 16)], 0, False)
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected "):
        R.scan_rst(os.path.join(full, "id1", "Blast-id1.0001.rst"), [(12, 12, 12), (12, 12, 16)], 0, False)
    # the history of both levels against the one-process MeshRun on the same deck
    par = meshfix.deck_par(LONE["problem"], LONE["overrides"], {"1": LONE["blocks"]["3"]})
    run = pkg("config").from_par(par, "blast")
    one = pkg("driver").MeshRun(_OracleMeshForMeshRun(orc.Mesh(pkg("config").levels(par, run)).problem()), run)
    one.main(pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path / "one")))
    for rel in ("Blast.hst", "lev1/Blast-lev1.hst"):
        head, rows = parse_hst(open(os.path.join(full, "id0", rel)).read())
        head1, rows1 = parse_hst(open(os.path.join(str(tmp_path / "one"), rel)).read())
        assert head == head1 and len(rows) >= 3
        check_rows(rows, rows1)


# ---- 5. a file of other cuts or another number of ranks is refused ---------------------------------------------------------------
def test_other_cuts_or_rank_count_are_refused_when_reading(tmp_path):
    fx = MFixture(BLAST_RESUMED)
    seed = fx.write_seeds(str(tmp_path / "seed"))
    assert meshfix.run_ranks(job_refused, (seed, None)) == ["read", "read"]                      # (the cuts it was written for)
    for msg in meshfix.run_ranks(job_refused, (seed, (0, 6, 16))):                               # other cuts
        assert msg.startswith("[restart_grids]: Expected "), msg
    msg = job_refused(0, 1, seed, None)                                                          # one rank reads rank 0's file
    assert msg.startswith("[restart_grids]: Expected "), msg


# ---- a process that resumes never ran the problem generator -------------------------------------------------------------------------
def job_sphere_constants(rank, world, restart_only):
    """PlanetPot at a few points and the pinned zones of a small sphere Grid, after the problem generator or after
    problem_read_restart alone (lib.setup_problem(initial=False) calls the latter)"""
    import ctypes as C
    lib = pkg("lib"); cfg = pkg("config")
    run = cfg.load(os.path.join(meshfix.dumpfix.DECKS, "athinput.ioniz_sphere"), [f"domain1/Nx{a + 1}=12" for a in range(3)], "ioniz_sphere")
    g = cfg.slab(run)
    p = lib.params_from_grid(g)
    H = lib.host(); pr = run.prob
    args = (pr["cs"], pr.get("rp", 1.2e10), pr.get("mp", 1.0e30), pr.get("np", 6.0e8))
    if restart_only:
        assert H.aa_problem_ioniz_sphere_restart(C.byref(p), *args) == 0
    else:
        U = np.zeros((20, 20, 20, 6))
        assert H.aa_problem_ioniz_sphere(C.byref(p), *args, U.ctypes.data_as(C.POINTER(C.c_double))) == 0
    n = H.aa_ioniz_sphere_pinned(C.byref(p), None, None)
    idx = np.zeros(max(n, 1), dtype=np.int64); val = np.zeros((max(n, 1), 6))
    H.aa_ioniz_sphere_pinned(C.byref(p), idx.ctypes.data_as(C.POINTER(C.c_longlong)), val.ctypes.data_as(C.POINTER(C.c_double)))
    pot = [H.aa_planet_pot(x, 0.5 * x, -0.25 * x) for x in (1.0e9, 1.0e10, 5.0e10)]
    return n, idx[:n].tolist(), val[:n].tolist(), pot


def test_sphere_constants_without_the_problem_generator():
    """each in a process of its own: the constants are file-scope statics of the host library"""
    gen = meshfix.run_ranks(job_sphere_constants, (False,), world=1)[0]
    rst = meshfix.run_ranks(job_sphere_constants, (True,), world=1)[0]
    assert gen[0] > 0 and gen == rst
