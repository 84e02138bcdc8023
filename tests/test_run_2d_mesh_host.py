"""How a refined 2-D run reaches aa_mesh_run_2d, without a GPU (tests/test_gpu_2d_smr_run.py runs the real thing):
  * csrc/time_step.h run_advance_levels -- the arithmetic of k2d_mesh_advance, one wavefront behind every queued mesh step -- built
    with the host compilers as C99 and as C++ (fixtures/mesh_advance_probe.c) and run over a scripted table, against literals derived
    by hand from new_dt.c / main.c beside each row AND against a Python restatement on driver.fold_levels / driver.pick_dt;
  * lib.Mesh.can_run_2d, driver.MeshRun.may_batch / advance and outputs.run on a stand-in for the Mesh."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import twodfix               # noqa: E402
from twodfix import pkg      # noqa: E402

SRC = os.path.join(HERE, "fixtures", "mesh_advance_probe.c")
CSRC = os.path.join(twodfix.ROOT, "atmospheric-athena_amd", "csrc")
DECK = os.path.join(twodfix.DECKS, "athinput.blast2d_smr")
INF, NAN = float("inf"), float("nan")

# two Grids, ndir = 2: root dx = 1, level 1 dx = 0.5
T1 = 1.0 + 0.05
DX2 = [(1.0, 1.0), (0.5, 0.5)]
# id, (dt, time, nstep), t_stop, tlim, cour_no, nstep_stop, [max_v per Grid], [dx per Grid] -> (dt, time, nstep, live)
ROWS = [
    # new_dt.c:33 the root's max_v1 = 4 is carried: level 1 divides it by ITS dx, 4/0.5 = 8 (its own 1/0.5 = 2; the root 4/1 = 4);
    # :168-170 0.5/8 = 0.0625 against 2*0.05 = 0.1; main.c:618 nstep 3 -> 4, time 1 + 0.05
    ("carried_maximum_decides", (0.05, 1.0, 3), 10.0, 100.0, 0.5, 99, [(4.0, 1.0), (1.0, 1.0)], DX2, (0.0625, T1, 4, 1)),
    # ... and the finer level's own where it is the larger: MAX(4/0.5, 5/0.5) = 10, 0.5/10 = 0.05 < 2*0.05
    ("fine_maximum_decides", (0.05, 1.0, 3), 10.0, 100.0, 0.5, 99, [(4.0, 1.0), (1.0, 5.0)], DX2, (0.05, T1, 4, 1)),
    # nothing moves: max_dti = 0, CourNo/0 = +inf, MIN(2*0.25, inf) = 0.5
    ("all_zero_maxima_factor_two", (0.25, 1.0, 3), 10.0, 100.0, 0.5, 99, [(0.0, 0.0), (0.0, 0.0)], DX2, (0.5, 1.25, 4, 1)),
    # ... and on the step that makes nstep 0 the CFL step itself, +inf, which the clip cuts to tlim - time = 100 - 1.25
    ("all_zero_maxima_nstep_0", (0.25, 1.0, -1), 10.0, 100.0, 0.5, 99, [(0.0, 0.0), (0.0, 0.0)], DX2, (98.75, 1.25, 0, 1)),
    # :167-168 nstep == 0 takes the CFL step as it is: 0.5/8 = 0.0625 although 2*0.01 = 0.02 is smaller
    ("nstep_0_no_factor_two", (0.01, 0.0, -1), 10.0, 100.0, 0.5, 99, [(4.0, 1.0), (1.0, 1.0)], DX2, (0.0625, 0.01, 0, 1)),
    # a NaN maximum on the LAST Grid: the carry takes it ((1 > NaN) is false: MAX gives its second operand), NaN/0.5, MAX(8, NaN) =
    # NaN, 0.5/NaN, MIN(2 dt, NaN) = NaN; NaN > 0 is false: the loop stops
    ("nan_maximum_on_the_last_grid_stops", (0.05, 1.0, 3), 10.0, 100.0, 0.5, 99, [(4.0, 1.0), (1.0, NAN)], DX2, (NAN, T1, 4, 0)),
    # ... on the root the same MAX drops it again: the carry of level 1 is (NaN > 1) ? NaN : 1 = 1, and its fold MAX(NaN, 4/0.5) = 8
    ("nan_maximum_on_the_root_is_dropped", (0.05, 1.0, 3), 10.0, 100.0, 0.5, 99, [(4.0, NAN), (1.0, 1.0)], DX2, (0.0625, T1, 4, 1)),
    # :183-185 time = 99.95 < 100 and 100 - 99.95 < 0.0625: dt = tlim - time (the subtraction's own rounding)
    ("clip_at_tlim", (0.05, 99.9, 3), 1000.0, 100.0, 0.5, 99, [(4.0, 1.0), (1.0, 1.0)], DX2, (100.0 - (99.9 + 0.05), 99.9 + 0.05, 4, 1)),
    # main.c:519 the three ways the loop ends: time reaches t_stop (1.05 < 1.05 is false) ...
    ("stops_at_t_stop", (0.05, 1.0, 3), T1, 100.0, 0.5, 99, [(4.0, 1.0), (1.0, 1.0)], DX2, (0.0625, T1, 4, 0)),
    ("goes_on_below_t_stop", (0.05, 1.0, 3), 1.0500001, 100.0, 0.5, 99, [(4.0, 1.0), (1.0, 1.0)], DX2, (0.0625, T1, 4, 1)),
    # ... nstep reaches nstep_stop ...
    ("stops_at_nstep_stop", (0.05, 1.0, 3), 10.0, 100.0, 0.5, 4, [(4.0, 1.0), (1.0, 1.0)], DX2, (0.0625, T1, 4, 0)),
    # ... or dt is not positive: MIN(2*0, 0.0625) = 0
    ("stops_at_dt_0", (0.0, 1.0, 3), 10.0, 100.0, 0.5, 99, [(4.0, 1.0), (1.0, 1.0)], DX2, (0.0, 1.0, 4, 0)),
    # three Grids, two of them on level 1 (dx = 0.5 each): the carry runs through the Grids in the Mesh's order, so the second
    # Domain of the level also sees the first one's 6: MAX(2/1, 6/0.5, 6/0.5) = 12, 0.6/12 = 0.05
    ("two_domains_on_a_level", (0.05, 1.0, 3), 10.0, 100.0, 0.6, 99, [(2.0, 1.0), (1.0, 6.0), (1.0, 1.0)],
     [(1.0, 1.0), (0.5, 0.5), (0.5, 0.5)], (0.6 / 12.0, T1, 4, 1)),
]


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def build(tmp, lang):
    so = os.path.join(str(tmp), f"mesh_advance_{lang}.so")
    cc = ["g++", "-x", "c++"] if lang == "cxx" else ["gcc", "-std=c99"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, SRC, "-o", so])
    L = C.CDLL(so)
    D, I, dp, ip = C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.probe_advance_levels.restype = None
    L.probe_advance_levels.argtypes = [dp, ip, D, D, D, I, I, I, dp, dp]
    return L


@pytest.fixture(scope="module", params=["c99", "cxx"])
def probe(request, tmp_path_factory):
    return build(tmp_path_factory.mktemp("mesh_advance"), request.param)


def restated(clock, t_stop, tlim, cour_no, nstep_stop, max_v, dx):
    """aa_mesh_step's bookkeeping and aa_mesh_new_dt as driver.py states the rule"""
    D = pkg("driver")
    dt, time, nstep = clock
    nstep += 1; time += dt
    v3 = [x for v in max_v for x in (v[0], v[1], 0.0)]
    max_dti = D.fold_levels(v3, [(d[0], d[1], 1.0) for d in dx], 2)
    dt_cfl = INF if max_dti == 0 else cour_no / max_dti
    dt = D.pick_dt(nstep, dt, dt_cfl, time, tlim)
    return dt, time, nstep, int(time < t_stop and nstep != nstep_stop and dt > 0.0)


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_advance_levels(probe, row):
    name, clock, t_stop, tlim, cour_no, nstep_stop, max_v, dx, want = row
    n = len(dx)
    c = (C.c_double * 2)(clock[0], clock[1]); i = (C.c_int * 2)(1, clock[2])
    v = (C.c_double * (2 * n))(*[x for q in max_v for x in q]); d = (C.c_double * (2 * n))(*[x for q in dx for x in q])
    probe.probe_advance_levels(c, i, t_stop, tlim, cour_no, nstep_stop, n, 2, v, d)
    got = (c[0], c[1], i[1], i[0])
    assert same(got[0], want[0]) and got[1:] == want[1:], (got, want)
    py = restated(clock, t_stop, tlim, cour_no, nstep_stop, max_v, dx)
    assert same(got[0], py[0]) and got[1:] == py[1:], (got, py)


def test_the_kernel_calls_that_function():
    """k2d_mesh_advance does its arithmetic through run_advance_levels, and the 3-D kernel sources bench.py fingerprints stay clear of
    the device clocks"""
    k = open(os.path.join(CSRC, "hydro2d_kernels.hip")).read()
    body = k[k.index("k2d_mesh_advance(Run2D *rc"):]
    assert "run_advance_levels(&c" in body[:body.index("// ---- launch wrappers")]
    hdr = open(os.path.join(twodfix.ROOT, "include", "athena_amd.h")).read()
    assert "int  aa_mesh_run_2d(aa_mesh *m, double t_stop, double tlim, int nstep_stop, int *nsteps_done);" in hdr
    assert "int  aa_mesh_run_2d_batch(const aa_mesh *m);" in hdr
    smr = open(os.path.join(CSRC, "smr.hip")).read()
    assert 'getenv("AA_2D_BATCH")' in smr


# ---- lib.Mesh.can_run_2d, MeshRun.may_batch / advance, outputs.run ----------------------------------------------------------------
class _G:
    def __init__(self, ndim=2, npin=0): self.ndim, self.npin = ndim, npin
    def history(self): raise AssertionError("no output block asks for a history row here")


def test_mesh_can_run_2d_follows_the_refusals_of_aa_mesh_run_2d():
    lib = pkg("lib")

    class M:
        def __init__(self, lev, cuts=None, links=None, batch=4):
            self.lev, self.cuts, self.links, self.batch = lev, cuts, links, batch
        def run_2d_batch(self): return self.batch
    can = lib.Mesh.can_run_2d
    assert can(M([_G(), _G()]))
    assert not can(M([_G(3), _G(3)]))                      # a Mesh of 3-D Grids
    assert not can(M([_G(), _G()], cuts=(0, 4, 8)))        # cut into slabs
    assert not can(M([_G(), _G()], links=[object()]))      # a rank's stack (aa_mesh_create_local)
    assert not can(M([_G(), _G(npin=1)]))                  # a level with pinned zones
    assert not can(M([_G(), _G()], batch=0))               # AA_2D_BATCH=0


class _FakeMesh:
    """what MeshRun asks of lib.Mesh: the state advances by dt = 0.003 per step"""

    def __init__(self, can=True, stuck=False):
        self.can, self.stuck, self.calls, self.lev = can, stuck, [], []
        self.time, self.dt, self.nstep = 0.0, 0.003, 0

    def start(self): self.calls.append("start"); return self
    def can_run_2d(self): return self.can
    def domain_numbers(self): return []

    def _one(self):
        self.nstep += 1; self.time += self.dt

    def step(self):
        self.calls.append("step"); self._one(); return []

    def run_2d(self, t_stop, tlim, nstep_stop):
        n = 0
        while not self.stuck and self.time < t_stop and self.nstep != nstep_stop:
            self._one(); n += 1
        self.calls.append(("run", t_stop, tlim, nstep_stop, n))
        return n


def _meshrun(mesh, ov=()):
    cfg, D, A = pkg("config"), pkg("driver"), pkg("athinput")
    ov = ["time/tlim=0.02", "job/maxout=0"] + list(ov)
    par = A.ParTable.from_file(DECK).cmdline(ov)
    run = cfg.load(DECK, ov, "blast", "ctu")
    return D.MeshRun(mesh, run), par


def test_meshrun_advance_takes_every_stretch_in_one_call(tmp_path):
    O = pkg("outputs")
    m, par = _meshrun(_FakeMesh(), ["time/nlim=-1"])
    assert m.may_batch()
    m.main(O.OutputSet.from_par(par, 0.0, str(tmp_path / "a")))
    assert m.mesh.calls == ["start", ("run", 0.02, 0.02, 1 << 20, 7)] and m.nstep == 7      # one stretch: t_stop = tlim
    # nlim ends the call
    m, par = _meshrun(_FakeMesh(), ["time/nlim=3"])
    m.main(O.OutputSet.from_par(par, 0.0, str(tmp_path / "b")))
    assert m.mesh.calls == ["start", ("run", 0.02, 0.02, 3, 3)] and m.nstep == 3
    # an output block every 0.007: a call per stretch, to the block's next time (a history block of a Mesh without levels writes nothing)
    m, par = _meshrun(_FakeMesh(), ["time/nlim=-1", "job/maxout=1", "output1/out_fmt=hst", "output1/dt=0.007"])
    m.main(O.OutputSet.from_par(par, 0.0, str(tmp_path / "c")))
    runs = [c for c in m.mesh.calls if c != "start"]
    assert [c[0] for c in runs] == ["run"] * 3 and [c[1] for c in runs] == [0.007, 0.014, 0.02] and [c[4] for c in runs] == [3, 2, 2]
    D = pkg("driver")
    assert "aa_mesh_run_2d" in D.MeshRun.advance.__doc__ and "aa_mesh_run_2d" in D.MeshRun.may_batch.__doc__


def test_meshrun_falls_back_to_single_steps(tmp_path):
    O = pkg("outputs")
    m, par = _meshrun(_FakeMesh(can=False), ["time/nlim=-1"])      # the Mesh says no (AA_2D_BATCH=0, pinned zones, 3-D, cut)
    assert not m.may_batch()
    m.main(O.OutputSet.from_par(par, 0.0, str(tmp_path / "a")))
    assert m.mesh.calls == ["start"] + ["step"] * 7
    # advance() returns 0 (a dt that is not positive ends aa_mesh_run_2d with no step taken): the single step goes on
    m, par = _meshrun(_FakeMesh(stuck=True), ["time/nlim=2"])
    m.main(O.OutputSet.from_par(par, 0.0, str(tmp_path / "b")))
    assert m.mesh.calls == ["start", ("run", 0.02, 0.02, 2, 0), "step", ("run", 0.02, 0.02, 2, 0), "step"]
    # a stand-in without can_run_2d (another engine's mesh) never batches
    m, par = _meshrun(_FakeMesh())
    del type(m.mesh).can_run_2d
    try:
        assert not m.may_batch()
    finally:
        type(m.mesh).can_run_2d = lambda self: self.can
