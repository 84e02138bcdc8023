"""How a 2-D run reaches aa_run_2d: Grid.can_run_2d, the local engine's can_batch / run_local, Driver.may_batch / advance and
outputs.run -- with stand-ins for the library and the engine.  No GPU (tests/test_gpu_2d_run.py runs the real thing)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import twodfix               # noqa: E402
from twodfix import pkg      # noqa: E402

BLAST2D = os.path.join(twodfix.DECKS, "athinput.blast2d")
OV = ["domain1/Nx1=24", "domain1/Nx2=20", "time/tlim=0.02", "job/maxout=0"]


class _Cfg:
    def __init__(self, level=0): self.level = level


class _FakeGrid:
    """what HipEngine.can_batch / run_local ask of lib.Grid"""

    def __init__(self, ndim, batch=16, can2=True, can1=True):
        self.ndim, self.batch, self.can2, self.can1, self.calls = ndim, batch, can2, can1, []

    def run_2d_batch(self): return self.batch
    def can_run_2d(self): return self.can2
    def can_run_until(self): return self.can1
    def run_2d(self, *a): self.calls.append(("run_2d",) + a); return 7
    def run_until(self, *a): self.calls.append(("run_until",) + a); return 9


def _engine(g):
    D = pkg("driver")
    e = D.HipEngine.__new__(D.HipEngine)      # (the routing alone: no device, no library)
    e.g = g
    return e


def test_grid_can_run_2d_follows_the_refusals_of_aa_run_2d():
    lib = pkg("lib")

    class G:
        def __init__(self, ndim, npin=0, in_mesh=False, level=0):
            self.ndim, self.npin, self.in_mesh, self.cfg = ndim, npin, in_mesh, _Cfg(level)
    can = lib.Grid.can_run_2d
    assert can(G(2))
    assert not can(G(1)) and not can(G(3))
    assert not can(G(2, npin=1))
    assert not can(G(2, in_mesh=True)) and not can(G(2, level=1))


def test_the_local_engine_routes_by_dimension():
    e2 = _engine(_FakeGrid(2))
    assert e2.can_batch()
    assert e2.run_local(0.5, 1.0, 40) == 7 and e2.g.calls == [("run_2d", 0.5, 1.0, 40)]
    assert not _engine(_FakeGrid(2, batch=0)).can_batch()          # AA_2D_BATCH=0
    assert not _engine(_FakeGrid(2, can2=False)).can_batch()       # pinned zones, a level of a Mesh
    assert not _engine(_FakeGrid(2, can2=False, can1=True)).can_batch()
    e1 = _engine(_FakeGrid(1, batch=0))
    assert e1.can_batch()                                          # (a 1-D Grid does not ask the 2-D knob)
    assert e1.run_local(0.5, 1.0, 40) == 9 and e1.g.calls == [("run_until", 0.5, 1.0, 40)]
    assert not _engine(_FakeGrid(3, can1=False)).can_batch()


class _FakeEngine:
    """a local engine of Driver: the state advances by dt = 0.003 per step"""

    def __init__(self, grid, batch=True):
        self.cfg, self.batch, self.calls = grid, batch, []
        self.time, self.dt, self.nstep = 0.0, 0.003, 0

    def start_local(self): self.calls.append("start")
    def mesh_state(self): return self.time, self.dt, self.nstep
    def set_mesh_state(self, t, dt, n): self.time, self.dt, self.nstep = t, dt, n
    def can_batch(self): return self.batch

    def _one(self):
        self.nstep += 1; self.time += self.dt

    def step_local(self):
        self.calls.append("step"); self._one(); return 0

    def run_local(self, t_stop, tlim, nstep_stop):
        n = 0
        while self.time < t_stop and self.nstep != nstep_stop:
            self._one(); n += 1
        self.calls.append(("run", t_stop, tlim, nstep_stop, n))
        return n


def _driver(batch=True, ov=()):
    cfg = pkg("config"); D = pkg("driver"); A = pkg("athinput")
    par = A.ParTable.from_file(BLAST2D).cmdline(OV + list(ov))
    run = cfg.from_par(par, "blast")
    assert tuple(run.rootNx) == (24, 20, 1)
    return D.Driver(run, engine_factory=lambda g: _FakeEngine(g, batch)), par


def test_driver_advance_hands_a_2d_stretch_to_run_local(tmp_path):
    O = pkg("outputs")
    d, par = _driver(ov=["time/nlim=-1"])
    assert d.may_batch()
    d.main(O.OutputSet.from_par(par, 0.0, str(tmp_path)))
    runs = [c for c in d.eng.calls if c != "start"]
    assert len(runs) == 1 and runs[0][0] == "run" and runs[0][1:3] == (0.02, 0.02)      # one stretch: t_stop = tlim, the deck's tlim
    assert runs[0][3] == 1 << 20 and runs[0][4] == d.nstep == 7                        # (no nlim: 2^20 steps ahead at the most)
    assert d.niter_trace == [0] * 7 and d.time == d.eng.time
    # nlim ends the call
    d, par = _driver(ov=["time/nlim=3"])
    d.main(O.OutputSet.from_par(par, 0.0, str(tmp_path)))
    assert [c for c in d.eng.calls if c != "start"] == [("run", 0.02, 0.02, 3, 3)] and d.nstep == 3
    assert "aa_run_2d" in type(d).advance.__doc__ and "aa_run_2d" in type(d).may_batch.__doc__


def test_a_driver_that_may_not_batch_takes_single_steps(tmp_path, monkeypatch):
    O = pkg("outputs")
    d, par = _driver(batch=False)                       # the engine says no (AA_2D_BATCH=0, pinned zones)
    assert not d.may_batch()
    d.main(O.OutputSet.from_par(par, 0.0, str(tmp_path)))
    assert d.eng.calls == ["start"] + ["step"] * 7
    d, par = _driver()                                  # a distributed Driver never asks its engine
    d.distributed = True
    monkeypatch.setattr(d.eng, "can_batch", lambda: pytest.fail("can_batch() asked by a distributed Driver"))
    assert not d.may_batch()
    d, par = _driver()                                  # an engine without the two calls
    monkeypatch.delattr(type(d.eng), "can_batch")
    assert not d.may_batch()


def test_the_knob_and_the_call_are_documented():
    """AA_2D_BATCH is read in aa_create and named where the knobs are listed; aa_run_2d stands in the public header"""
    root = twodfix.ROOT
    api = open(os.path.join(root, "atmospheric-athena_amd", "csrc", "api.hip")).read()
    assert 'getenv("AA_2D_BATCH")' in api
    hdr = open(os.path.join(root, "include", "athena_amd.h")).read()
    assert "int aa_run_2d(aa_grid *g, double t_stop, double tlim, int nstep_stop, int *nsteps_done);" in hdr
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "AA_2D_BATCH" in open(os.path.join(root, doc)).read(), doc
    # the sources bench.py fingerprints know nothing of the device clocks and of the header that holds their rule
    for f in ("grid.h", "hydro_kernels.hip", "hydro_dev.h", "ion_kernels.hip", "ion_pass.hip", "ion_dev.h"):
        text = open(os.path.join(root, "atmospheric-athena_amd", "csrc", f)).read()
        for word in ("Run2D", "RunClock", "time_step.h"):
            assert word not in text, (f, word)
