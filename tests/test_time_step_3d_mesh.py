"""How a refined 3-D run reaches aa_mesh_run_3d, without a GPU (tests/test_gpu_3d_smr_run.py runs the real thing):
  * the host mirror of k3d_mesh_advance, one wavefront behind every queued step of a 3-D Mesh: csrc/time_step.h run_advance_levels
    with three directions over Grids of different dx, then run_step_ratios of the new dt over every Grid's OWN dx -- through
    fixtures/mesh_advance_probe_3d.c, built with the host compilers as C99 and as C++.  The rows are the tables of
    test_time_step.py (outcomes as literals derived from the reference's text there), the way test_run_2d_mesh_host.py runs its own
    rows for two directions; a row of PICK / LIVE reaches the pick through the advance as in test_time_step_3d.py, here with the
    deciding maximum on the ROOT and carried to a finer Grid (new_dt.c:33), so every row also checks the carry.
    The per-level ratios are compared with Python's own IEEE quotient and product: the bits step_ratios() forms on the host.
  * the text of the C-ABI and of the kernel: the two symbols, the knob, the function the kernel calls.
  * lib.Mesh.can_run_3d, driver.MeshRun.may_batch / advance and outputs.run on a stand-in for the Mesh."""
import ctypes as C
import math
import os
import random
import subprocess

import pytest

from test_time_step import FOLD, INF, LIVE, PICK, flat, same
from test_ion_subcycles import HERE, PKG
from test_run_2d_mesh_host import _FakeMesh, _G, _meshrun
from twodfix import pkg

SRC = os.path.join(HERE, "fixtures", "mesh_advance_probe_3d.c")
CSRC = os.path.join(PKG, "csrc")
# root, level 1, level 2 (anisotropic zones: every direction has a dx of its own on every level)
DX3 = [(1.0, 0.5, 0.25), (0.5, 0.25, 0.125), (0.25, 0.125, 0.0625)]


def build(tmp, lang):
    so = os.path.join(str(tmp), f"mesh_advance_3d_{lang}.so")
    cc = ["g++", "-x", "c++"] if lang == "cxx" else ["gcc", "-std=c99"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, SRC, "-o", so])
    L = C.CDLL(so)
    D, I, dp, ip = C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.probe_mesh_advance_3d.restype = None
    L.probe_mesh_advance_3d.argtypes = [dp, ip, D, D, D, I, I, dp, dp, dp]
    return L


@pytest.fixture(scope="module", params=["c99", "cxx"])
def probe(request, tmp_path_factory):
    return build(tmp_path_factory.mktemp("mesh_advance_3d"), request.param)


def advance(L, time, dt, nstep, t_stop, tlim, cour_no, nstep_stop, max_v, dx):
    """-> (time, dt, nstep, live, [six ratios per Grid]) behind one pass of the advance over the Grids (max_v, dx: a triple per Grid)"""
    n = len(dx)
    c = (C.c_double * 2)(dt, time); i = (C.c_int * 2)(1, nstep)
    v = (C.c_double * (3 * n))(*[x for q in max_v for x in q]); d = (C.c_double * (3 * n))(*[x for q in dx for x in q])
    r = (C.c_double * (6 * n))()
    L.probe_mesh_advance_3d(c, i, t_stop, tlim, cour_no, nstep_stop, n, v, d, r)
    return c[1], c[0], i[1], i[0], [list(r[6 * l:6 * l + 6]) for l in range(n)]


def ratios_are_the_hosts(dt, dx, ratios):
    """dt/dx_d and 0.5*(dt/dx_d) of every Grid's own dx, as Python's IEEE division and product give them"""
    for q, r in zip(dx, ratios):
        for a in range(3):
            assert same(r[a], dt / q[a]) and same(r[3 + a], 0.5 * (dt / q[a])), (dt, q, r)


@pytest.mark.parametrize("case", PICK, ids=[c[0] for c in PICK])
def test_advance_picks_the_rows_dt_on_three_levels(probe, case):
    """the row's CFL step from the root's maximum over the FINEST Grid's smallest dx: max_v3 = 0.0625 on the root alone, carried
    to level 2 where dx3 = 0.0625 gives max_dti = 1 (the root itself: 0.0625/0.25, level 1: 0.0625/0.125) -- so cour_no is the CFL
    step, as in test_time_step_3d.py"""
    name, nstep, dt, dt_cfl, time, tlim, want = case
    if dt_cfl == INF:
        cour_no, max_v = 0.5, [(0.0, 0.0, 0.0)] * 3
    else:
        cour_no, max_v = dt_cfl, [(0.0, 0.0, 0.0625), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)]
    assert (time - dt) + dt == time
    t, d, n, live, ratios = advance(probe, time - dt, dt, nstep - 1, 1.0e300, tlim, cour_no, -7, max_v, DX3)
    assert t == time and n == nstep
    assert same(d, want)
    assert live == (1 if want > 0.0 else 0)
    ratios_are_the_hosts(d, DX3, ratios)


@pytest.mark.parametrize("case", [c for c in FOLD if c[1] == 3], ids=[c[0] for c in FOLD if c[1] == 3])
def test_advance_folds_the_rows_levels(probe, case):
    """the FOLD rows with three directions, one to three levels: step 0 far from tlim with CourNo = 1 gives dt = 1/max_dti"""
    name, ndir, levels, want = case
    max_v, dx = [lv[0] for lv in levels], [lv[1] for lv in levels]
    t, d, n, live, ratios = advance(probe, 0.0, 0.0, -1, 1.0e300, INF, 1.0, -7, max_v, dx)
    assert (t, n) == (0.0, 0)
    assert d == (1.0 / want if want > 0.0 else INF) and live == 1
    D = pkg("driver")
    assert D.fold_levels(flat(levels)[0], dx, 3) == want            # the Python statement of the same fold
    ratios_are_the_hosts(d, dx, ratios)


@pytest.mark.parametrize("case", LIVE, ids=[c[0] for c in LIVE])
def test_advance_applies_the_loop_condition(probe, case):
    name, time, t_stop, nstep, nstep_stop, dt, want = case
    max_v = [(0.0, 0.0, 0.0625), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)]
    t, d, n, live, ratios = advance(probe, time - 1.0, 1.0, nstep - 1, t_stop, INF, dt, nstep_stop, max_v, DX3)
    assert t == time and n == nstep and same(d, dt)
    assert live == want
    ratios_are_the_hosts(d, DX3, ratios)


def test_two_domains_on_a_level_and_random_ratios(probe):
    """the carry runs through the Grids in the Mesh's order, so the second Domain of a level also sees the first one's maximum:
    MAX(2/1, 6/0.5, 6/0.5) = 12, 0.6/12 = 0.05 (the 2-D row of test_run_2d_mesh_host.py with a third direction at rest); and
    random dt / dx: every Grid's six ratios are the host's bits"""
    t, d, n, live, ratios = advance(probe, 1.0, 0.05, 3, 10.0, 100.0, 0.6, 99, [(2.0, 1.0, 0.0), (1.0, 6.0, 0.0), (1.0, 1.0, 0.0)],
                                    [(1.0, 1.0, 1.0), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)])
    assert (t, d, n, live) == (1.0 + 0.05, 0.6 / 12.0, 4, 1)
    rng = random.Random(7)
    for _ in range(500):
        ng = rng.randint(1, 16)
        dx = [tuple(rng.uniform(1.0, 10.0) * 10.0 ** rng.randint(-6, 6) for _ in range(3)) for _ in range(ng)]
        mv = [tuple(rng.uniform(0.0, 10.0) for _ in range(3)) for _ in range(ng)]
        t, d, n, live, ratios = advance(probe, 0.0, 0.0, -1, 1.0e300, INF, 0.4, -7, mv, dx)
        cum, max_dti = [0.0] * 3, 0.0
        for v, q in zip(mv, dx):
            cum = [max(a, b) for a, b in zip(cum, v)]
            max_dti = max([max_dti] + [a / b for a, b in zip(cum, q)])
        assert d == 0.4 / max_dti and live == 1
        ratios_are_the_hosts(d, dx, ratios)
    # a stopped clock's dt: NaN passes through as the host's division passes it
    t, d, n, live, ratios = advance(probe, 0.0, 1.0, 3, 1.0e300, INF, 0.4, -7, [(float("nan"),) * 3], [(0.5, 0.25, 0.125)])
    assert math.isnan(d) and live == 0 and all(math.isnan(x) for x in ratios[0])


def test_the_kernel_calls_those_functions():
    """k3d_mesh_advance does its arithmetic through run_advance_levels with three directions and run_step_ratios; the C-ABI has the
    two symbols; the knob is read where the Mesh is made; the chain predicate is asked of a level, not copied"""
    k = open(os.path.join(CSRC, "hydro3d_clock.hip")).read()
    body = k[k.index("k3d_mesh_advance(Run3D *rc"):k.index("void launch_3d_seed(")]
    assert "run_advance_levels(&c" in body and ", tab.n, 3, mv, dx)" in body and "run_step_ratios(c.dt, dx + 3*l" in body
    seed = k[k.index("k3d_mesh_seed(Run3D *rc"):k.index("k3d_mesh_advance(Run3D *rc")]
    assert "run_step_ratios(v.c.dt, tab.dx + 3*l" in seed
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "athena_amd.h")).read()
    assert "int  aa_mesh_run_3d(aa_mesh *m, double t_stop, double tlim, int nstep_stop, int *nsteps_done);" in hdr
    assert "int  aa_mesh_run_3d_batch(const aa_mesh *m);" in hdr
    smr = open(os.path.join(CSRC, "smr.hip")).read()
    assert 'getenv("AA_3D_BATCH")' in smr and "on_queued_chain_3d(g)" in smr
    run = open(os.path.join(CSRC, "run.hip")).read()
    assert run.count("c.correct_all && x3_fused && c.fused_update") == 1       # ONE statement of the chain's conditions


# ---- lib.Mesh.can_run_3d, MeshRun.may_batch / advance, outputs.run ----------------------------------------------------------------
def test_mesh_can_run_3d_follows_the_refusals_of_aa_mesh_run_3d():
    lib = pkg("lib")

    class M:
        def __init__(self, lev, cuts=None, links=None, batch=4):
            self.lev, self.cuts, self.links, self.batch = lev, cuts, links, batch
        def run_3d_batch(self): return self.batch
    can = lib.Mesh.can_run_3d
    assert can(M([_G(3), _G(3)]))
    assert not can(M([_G(2), _G(2)]))                        # a Mesh of 2-D Grids
    assert not can(M([_G(3), _G(3)], cuts=(0, 4, 8)))        # cut into slabs
    assert not can(M([_G(3), _G(3)], links=[object()]))      # a rank's stack (aa_mesh_create_local)
    assert not can(M([_G(3), _G(3, npin=1)]))                # a level with pinned zones
    assert not can(M([_G(3), _G(3)], batch=0))               # AA_3D_BATCH=0, or a level off the queued chain


class _FakeMesh3(_FakeMesh):
    """a stand-in for a Mesh of 3-D Grids: run_2d refuses, run_3d takes the stretch"""

    def can_run_2d(self): return False
    def can_run_3d(self): return self.can
    def run_2d(self, *a): raise AssertionError("a 3-D Mesh goes through run_3d")

    def run_3d(self, t_stop, tlim, nstep_stop):
        return _FakeMesh.run_2d(self, t_stop, tlim, nstep_stop)


def test_meshrun_takes_every_stretch_of_a_3d_mesh_in_one_call(tmp_path):
    O, D = pkg("outputs"), pkg("driver")
    m, par = _meshrun(_FakeMesh3(), ["time/nlim=-1", "job/maxout=1", "output1/out_fmt=hst", "output1/dt=0.007"])
    assert m.may_batch()
    m.main(O.OutputSet.from_par(par, 0.0, str(tmp_path / "a")))
    runs = [c for c in m.mesh.calls if c != "start"]
    assert [c[0] for c in runs] == ["run"] * 3 and [c[1] for c in runs] == [0.007, 0.014, 0.02] and [c[4] for c in runs] == [3, 2, 2]
    m, par = _meshrun(_FakeMesh3(can=False), ["time/nlim=-1"])      # the Mesh says no (AA_3D_BATCH=0, a level off the chain, pinned zones, cut)
    assert not m.may_batch()
    m.main(O.OutputSet.from_par(par, 0.0, str(tmp_path / "b")))
    assert m.mesh.calls == ["start"] + ["step"] * 7
    assert "aa_mesh_run_3d" in D.MeshRun.advance.__doc__ and "aa_mesh_run_3d" in D.MeshRun.may_batch.__doc__
