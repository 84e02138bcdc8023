"""The time-step rule new_dt.c:156-185 and the loop condition main.c:519 as tables of scripted cases with the outcomes as literals,
each derived by hand from the reference's text beside its row:
  :33, :53   max_v1..3 are zeroed ONCE, in front of the loop over Grids: a level's maxima include the coarser levels'
  :156-161   max_dti = MAX(max_dti, max_v_d/dx_d) for the directions with more than one zone, MAX(a,b) = (a > b) ? a : b
  :167-171   dt = CourNo/max_dti on step 0, else MIN(2.0*dt, CourNo/max_dti), MIN(a,b) = (a < b) ? a : b (defs.h.in:146)
  :183-185   if (time < tlim && (tlim - time) < dt) dt = tlim - time

The same rows drive
  * csrc/time_step.h -- what the C library, the two device clocks (k1d_run, k2d_advance) and the drop-in shim call -- through
    fixtures/time_step_probe.c, built with the host compilers (as C++ and as C99; no device),
  * driver.pick_dt and driver.fold_levels, and
  * Driver.new_dt and MeshDriver.new_dt on the scripted engines of test_ion_subcycles.py, one rank.
Results are compared with == on doubles, NaN with math.isnan.

Not scripted for MeshDriver: max_dti = 0.  Its quotient cour_no/max_dti is Python's division, which raises where C gives +inf; the row
reaches MeshDriver's pick through cour_no = +inf over max_dti = 1 instead."""
import copy
import ctypes as C
import math
import os
import subprocess

import pytest

from test_ion_subcycles import HERE, PKG, Phased, decks, mesh_engine, one_rank      # noqa: F401  (decks, one_rank: fixtures)

INF, NAN = float("inf"), float("nan")

# id, nstep, dt, dt_cfl, time, tlim -> dt
PICK = [
    # :167-168 step 0 takes the CFL step as it is: 2*dt = 2 < 5 would bind, and is not looked at
    ("nstep_0_no_factor_two", 0, 1.0, 5.0, 0.0, 100.0, 5.0),
    # :170 MIN(2*1, 5) = 2
    ("factor_two_binds", 3, 1.0, 5.0, 0.0, 100.0, 2.0),
    # :170 MIN(2*1, 1.5) = 1.5
    ("cfl_binds", 3, 1.0, 1.5, 0.0, 100.0, 1.5),
    # :170 2*0.75 < 1.5 is false: the second operand, the same number
    ("two_dt_equals_cfl", 3, 0.75, 1.5, 0.0, 100.0, 1.5),
    # :184 99.25 < 100 and 100 - 99.25 = 0.75 < 1.5: dt = 0.75
    ("clip_at_tlim", 3, 1.0, 1.5, 99.25, 100.0, 0.75),
    # :184 the clip acts on the step the factor two left: MIN(2, 5) = 2, 0.75 < 2
    ("clip_behind_factor_two", 3, 1.0, 5.0, 99.25, 100.0, 0.75),
    # :184 time < tlim is false at time == tlim and beyond: no clip (tlim - time would be 0 and -1)
    ("time_equals_tlim", 3, 1.0, 1.5, 100.0, 100.0, 1.5),
    ("time_beyond_tlim", 3, 1.0, 1.5, 101.0, 100.0, 1.5),
    # :184 (tlim - time) < dt is false at 1.5 < 1.5: no clip
    ("rest_equals_dt", 3, 1.0, 1.5, 98.5, 100.0, 1.5),
    # :168-170 max_dti = 0: CourNo/0 = +inf; MIN(2*1, inf) = 2 -- and on step 0 inf itself, which the clip cuts to 100 - 0
    ("max_dti_0_factor_two_decides", 3, 1.0, INF, 0.0, 100.0, 2.0),
    ("max_dti_0_step_0_clip_decides", 0, 1.0, INF, 0.0, 100.0, 100.0),
    # :170 2 < NaN is false: MIN gives its second operand, NaN; :184 100 < NaN is false: it stays
    ("nan_cfl_gives_nan", 3, 1.0, NAN, 0.0, 100.0, NAN),
    ("nan_cfl_step_0", 0, 1.0, NAN, 0.0, 100.0, NAN),
    # :170 MIN(2*0, 1.5) = 0: a run whose dt is 0 stays there
    ("dt_0", 3, 0.0, 1.5, 0.0, 100.0, 0.0),
]

# id, ndir, [(max_v1..3, dx1..3) per level] -> max_dti
FOLD = [
    # :156 a 1-D Grid: x1 alone, 3/0.5 = 6 (the other two would give 1e5)
    ("one_direction", 1, [((3.0, 100.0, 100.0), (0.5, 0.001, 0.001))], 6.0),
    # :156-159 a 2-D Grid: MAX(3/0.5, 1/0.125) = 8 (x3 would give 1e5)
    ("two_directions", 2, [((3.0, 1.0, 100.0), (0.5, 0.125, 0.001))], 8.0),
    # :156-161 MAX(6, 8, 2/0.0625) = 32
    ("three_directions", 3, [((3.0, 1.0, 2.0), (0.5, 0.125, 0.0625))], 32.0),
    # nothing moves: MAX(0, 0/dx) = 0
    ("at_rest", 3, [((0.0, 0.0, 0.0), (0.5, 0.5, 0.5))], 0.0),
    # :33 two levels: the root's max_v1 = 4 is still there when level 1 divides by ITS dx: 4/0.5 = 8 (level 1 alone: 1/0.5 = 2;
    # without the carry MAX(4/1, 2) = 4)
    ("two_levels_root_decides", 3, [((4.0, 1.0, 1.0), (1.0, 1.0, 1.0)), ((1.0, 1.0, 1.0), (0.5, 0.5, 0.5))], 8.0),
    # :33 three levels: carried maxima (1,6,1) -> (2,6,1) -> (2,6,3); the root's max_v2 = 6 over level 2's dx: 6/0.25 = 24
    # (level 2 alone: 3/0.25 = 12; level 1 with the carry: 6/0.5 = 12)
    ("three_levels_root_decides", 3, [((1.0, 6.0, 1.0), (1.0, 1.0, 1.0)), ((2.0, 1.0, 1.0), (0.5, 0.5, 0.5)),
                                      ((1.0, 1.0, 3.0), (0.25, 0.25, 0.25))], 24.0),
    # ... and a finer level's own maximum where it is the larger one: 5/0.5 = 10 against the carried 4/0.5 = 8
    ("two_levels_fine_decides", 3, [((4.0, 1.0, 1.0), (1.0, 1.0, 1.0)), ((1.0, 5.0, 1.0), (0.5, 0.5, 0.5))], 10.0),
]

# id, time, t_stop, nstep, nstep_stop, dt -> whether the loop goes on (main.c:519 as the run calls use it)
LIVE = [
    ("goes_on", 0.5, 1.0, 3, 9, 0.125, 1),
    ("nan_dt_stops", 0.5, 1.0, 3, 9, NAN, 0),                 # NaN > 0 is false
    ("dt_0_stops", 0.5, 1.0, 3, 9, 0.0, 0),
    ("negative_dt_stops", 0.5, 1.0, 3, 9, -0.125, 0),
    ("nstep_at_its_stop", 0.5, 1.0, 9, 9, 0.125, 0),
    ("time_at_t_stop", 1.0, 1.0, 3, 9, 0.125, 0),               # time < t_stop is false
    ("time_beyond_t_stop", 1.5, 1.0, 3, 9, 0.125, 0),
    ("nstep_stop_is_no_ceiling", 0.5, 1.0, 10, 9, 0.125, 1),    # != , not < : the callers bound the span (0 .. 2^20)
]


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def flat(levels):
    return [x for lv in levels for x in lv[0]], [x for lv in levels for x in lv[1]]


# ---- csrc/time_step.h ---------------------------------------------------------------------------------------------------------
SRC = os.path.join(HERE, "fixtures", "time_step_probe.c")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("time_step") / "time_step_probe.so")
    subprocess.check_call(["g++", "-x", "c++", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(PKG, "csrc"), SRC, "-o", so])
    L = C.CDLL(so)
    D, I, dp = C.c_double, C.c_int, C.POINTER(C.c_double)
    for name, res, args in (("probe_fold", D, [D, dp, dp, I]), ("probe_fold_levels", D, [I, dp, dp, I]), ("probe_courant", D, [D, D]),
                            ("probe_grow", D, [I, D, D]), ("probe_clip", D, [D, D, D]), ("probe_pick", D, [I, D, D, D, D]),
                            ("probe_two_halves", D, [I, D, D, D, D, D]), ("probe_live", I, [D, D, I, I, D]), ("probe_clock_layout", I, [])):
        f = getattr(L, name); f.restype = res; f.argtypes = args
    return L


def test_header_is_c99(tmp_path):
    """the shim includes the header from C"""
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), "-c", SRC,
                           "-o", str(tmp_path / "time_step_probe.o")])


@pytest.mark.parametrize("case", PICK, ids=[c[0] for c in PICK])
def test_header_pick(probe, case):
    name, nstep, dt, dt_cfl, time, tlim, want = case
    assert same(probe.probe_pick(nstep, dt, dt_cfl, time, tlim), want)
    # the two halves, as the MPI shim calls them around its MIN over ranks (:169-177, :183-185): another rank that found nothing
    # smaller changes nothing ...
    grown = probe.probe_grow(nstep, dt, dt_cfl)
    assert same(probe.probe_clip(grown, time, tlim), want)
    assert same(probe.probe_two_halves(nstep, dt, dt_cfl, INF, time, tlim), want)


def test_header_two_halves_with_a_smaller_rank(probe):
    """... and one that found 1.25 where this rank has MIN(2*1, 5) = 2 gives 1.25; the clip acts on that: 100 - 99.25 = 0.75 < 1.25,
    and 100 - 98.5 = 1.5 is not"""
    assert probe.probe_two_halves(3, 1.0, 5.0, 1.25, 0.0, 100.0) == 1.25
    assert probe.probe_two_halves(3, 1.0, 5.0, 1.25, 99.25, 100.0) == 0.75
    assert probe.probe_two_halves(3, 1.0, 5.0, 1.25, 98.5, 100.0) == 1.25


@pytest.mark.parametrize("case", FOLD, ids=[c[0] for c in FOLD])
def test_header_fold(probe, case):
    name, ndir, levels, want = case
    v, dx = flat(levels)
    n = len(v)
    assert probe.probe_fold_levels(len(levels), (C.c_double * n)(*v), (C.c_double * n)(*dx), ndir) == want
    if len(levels) == 1:
        assert probe.probe_fold(0.0, (C.c_double * 3)(*v), (C.c_double * 3)(*dx), ndir) == want


def test_header_courant(probe):
    """:168 CourNo/max_dti: 0.8/32 = 0.025 (both exact in binary up to the one rounding of the division, which Python shares);
    max_dti = 0 gives +inf, a NaN maximum NaN"""
    assert probe.probe_courant(0.5, 32.0) == 0.015625
    assert probe.probe_courant(0.8, 32.0) == 0.8 / 32.0
    assert probe.probe_courant(0.8, 0.0) == INF
    assert math.isnan(probe.probe_courant(0.8, NAN))


@pytest.mark.parametrize("case", LIVE, ids=[c[0] for c in LIVE])
def test_header_loop_condition(probe, case):
    name, time, t_stop, nstep, nstep_stop, dt, want = case
    assert probe.probe_live(time, t_stop, nstep, nstep_stop, dt) == want


def test_header_clock_layout(probe):
    assert probe.probe_clock_layout() == 1


# ---- driver.py ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PICK, ids=[c[0] for c in PICK])
def test_pick_dt(decks, case):
    name, nstep, dt, dt_cfl, time, tlim, want = case
    assert same(decks[0].pick_dt(nstep, dt, dt_cfl, time, tlim), want)


@pytest.mark.parametrize("case", FOLD, ids=[c[0] for c in FOLD])
def test_fold_levels(decks, case):
    name, ndir, levels, want = case
    assert decks[0].fold_levels(flat(levels)[0], [lv[1] for lv in levels], ndir) == want


class Cfl(Phased):
    """Driver's engine protocol for new_dt: the Grid's CFL step, and the state it is told afterwards"""

    def __init__(self, dt_cfl):
        super().__init__([])
        self.dt_cfl = dt_cfl

    def new_dt_local(self): return self.dt_cfl


@pytest.mark.parametrize("case", PICK, ids=[c[0] for c in PICK])
def test_driver_new_dt(decks, case):
    name, nstep, dt, dt_cfl, time, tlim, want = case
    driver, run1, _, _ = decks
    run = copy.copy(run1); run.tlim = tlim
    d = driver.Driver(run, lambda grid: Cfl(dt_cfl))
    d.nstep, d.dt, d.time = nstep, dt, time
    d.new_dt()
    assert same(d.dt, want)
    assert d.eng.state[0] == time and same(d.eng.state[1], want) and d.eng.state[2] == nstep


def mesh_driver(decks, levels, cour_no, tlim):
    """a two-level MeshDriver whose levels have the scripted maxima and zone sizes (level 1: half the root's, init_mesh.c)"""
    driver, _, par2, run2 = decks
    run = copy.copy(run2); run.tlim, run.cour_no = tlim, cour_no
    run.xmin, run.xmax = (0.0, 0.0, 0.0), tuple(levels[0][1][d] * run.rootNx[d] for d in range(3))      # (dx = extent/rootNx, exact)
    assert all(run.dx[d] == levels[0][1][d] and levels[1][1][d] == run.dx[d] / 2.0 for d in range(3))
    eng = mesh_engine(Phased, [])
    eng.cfl_max_v = lambda l: list(levels[l][0])
    d = driver.MeshDriver(par2, run, lambda cfg: eng)
    assert (d.NL, d.nl) == (2, 2)
    return d


@pytest.mark.parametrize("case", PICK, ids=[c[0] for c in PICK])
def test_mesh_driver_new_dt_pick(decks, case):
    """max_dti = MAX(0.5/1, 0.5/0.5) = 1, so the CFL step is cour_no itself: the row's dt_cfl goes in as cour_no"""
    name, nstep, dt, dt_cfl, time, tlim, want = case
    d = mesh_driver(decks, [((0.5, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.5, 0.0, 0.0), (0.5, 0.5, 0.5))], dt_cfl, tlim)
    d.nstep, d.dt, d.time = nstep, dt, time
    d.new_dt()
    assert same(d.dt, want) and all(same(x, want) for x in d.dtl)
    assert d.eng.state[0] == time and same(d.eng.state[1], want) and d.eng.state[2] == nstep


@pytest.mark.parametrize("case", [c for c in FOLD if len(c[2]) == 2], ids=[c[0] for c in FOLD if len(c[2]) == 2])
def test_mesh_driver_new_dt_carry(decks, case):
    """the two-level rows through MeshDriver.new_dt on step 0 far from tlim: dt = cour_no/max_dti = 0.5/8 and 0.5/10"""
    name, ndir, levels, want = case
    d = mesh_driver(decks, levels, 0.5, 100.0)
    d.nstep, d.dt, d.time = 0, 1.0, 0.0
    d.new_dt()
    assert d.dt == {8.0: 0.0625, 10.0: 0.05}[want] == 0.5 / want
