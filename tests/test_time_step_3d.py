"""The host mirror of aa_run_3d's device clock: csrc/time_step.h run_advance_grid (what k3d_advance does behind every queued step:
nstep++, time += dt, new_dt.c:156-185, main.c:519) and run_step_ratios (the six dt/dx_d and 0.5*(dt/dx_d) k3d_seed / k3d_advance
leave beside dt for the *_dc kernels), through fixtures/time_step_probe_3d.c built with the host compilers -- no device.

The rows are the tables of test_time_step.py, outcomes as literals derived from the reference's text there.  A row's state reaches
the pick through the advance: the clock starts one step and one dt earlier (every number in the tables is a binary fraction, so
(time - dt) + dt is time again), max_dti = 1/1 makes the CFL step cour_no itself, and a row with max_dti = 0 gets maxima of 0.
The ratios are compared with Python's own IEEE quotient and product, bit for bit: the bits step_ratios() forms on the host."""
import ctypes as C
import math
import os
import random
import subprocess

import pytest

from test_time_step import FOLD, INF, LIVE, PICK, same
from test_ion_subcycles import HERE, PKG

SRC = os.path.join(HERE, "fixtures", "time_step_probe_3d.c")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("time_step_3d") / "time_step_probe_3d.so")
    subprocess.check_call(["g++", "-x", "c++", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(PKG, "csrc"), SRC, "-o", so])
    L = C.CDLL(so)
    D, I, dp = C.c_double, C.c_int, C.POINTER(C.c_double)
    for name, res, args in (("probe_advance_grid", I, [D, D, I, D, D, D, I, I, dp, dp, dp]), ("probe_step_ratios", None, [D, dp, dp]),
                            ("probe_dt_over_dx", D, [D, D]), ("probe_half_dt_over_dx", D, [D, D])):
        f = getattr(L, name); f.restype = res; f.argtypes = args
    return L


def advance(L, time, dt, nstep, t_stop, tlim, cour_no, nstep_stop, ndir, max_v, dx):
    """-> (time, dt, nstep, live) behind one pass of the advance"""
    out = (C.c_double * 2)()
    r = L.probe_advance_grid(time, dt, nstep, t_stop, tlim, cour_no, nstep_stop, ndir, (C.c_double * 3)(*max_v), (C.c_double * 3)(*dx), out)
    return out[0], out[1], r >> 1, r & 1


def test_header_is_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), "-c", SRC,
                           "-o", str(tmp_path / "time_step_probe_3d.o")])


@pytest.mark.parametrize("case", PICK, ids=[c[0] for c in PICK])
def test_advance_picks_the_rows_dt(probe, case):
    name, nstep, dt, dt_cfl, time, tlim, want = case
    if dt_cfl == INF:
        cour_no, max_v = 0.5, (0.0, 0.0, 0.0)               # CourNo/0 = +inf
    else:
        cour_no, max_v = dt_cfl, (1.0, 0.0, 0.0)            # max_dti = MAX(0, 1/1, 0/1, 0/1) = 1
    assert (time - dt) + dt == time
    t, d, n, live = advance(probe, time - dt, dt, nstep - 1, 1.0e300, tlim, cour_no, -7, 3, max_v, (1.0, 1.0, 1.0))
    assert t == time and n == nstep
    assert same(d, want)
    assert live == (1 if want > 0.0 else 0)                 # main.c:519 with t_stop far away: dt > 0 (NaN > 0 is false)


@pytest.mark.parametrize("case", [c for c in FOLD if len(c[2]) == 1], ids=[c[0] for c in FOLD if len(c[2]) == 1])
def test_advance_folds_the_rows_directions(probe, case):
    """step 0 far from tlim with CourNo = 1: dt = 1/max_dti, the quotient Python forms too (+inf where nothing moves)"""
    name, ndir, levels, want = case
    max_v, dx = levels[0]
    t, d, n, live = advance(probe, 0.0, 0.0, -1, 1.0e300, INF, 1.0, -7, ndir, max_v, dx)
    assert (t, n) == (0.0, 0)
    assert d == (1.0 / want if want > 0.0 else INF) and live == 1


@pytest.mark.parametrize("case", LIVE, ids=[c[0] for c in LIVE])
def test_advance_applies_the_loop_condition(probe, case):
    """the row's (time, nstep, dt) behind the advance: one step and 1.0 earlier, the new dt = MIN(2*1.0, CourNo/1) = the row's dt
    (2 < NaN and 2 < -0.125 are false: the second operand)"""
    name, time, t_stop, nstep, nstep_stop, dt, want = case
    t, d, n, live = advance(probe, time - 1.0, 1.0, nstep - 1, t_stop, INF, dt, nstep_stop, 3, (1.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert t == time and n == nstep and same(d, dt)
    assert live == want


def test_step_ratios_are_the_hosts_bits(probe):
    rng = random.Random(11)
    out = (C.c_double * 6)()
    for _ in range(2000):
        dt = rng.uniform(1.0, 10.0) * 10.0 ** rng.randint(-12, 3)
        dx = [rng.uniform(1.0, 10.0) * 10.0 ** rng.randint(-6, 12) for _ in range(3)]
        probe.probe_step_ratios(dt, (C.c_double * 3)(*dx), out)
        for a in range(3):
            assert out[a] == dt / dx[a] == probe.probe_dt_over_dx(dt, dx[a])
            assert out[3 + a] == 0.5 * (dt / dx[a]) == probe.probe_half_dt_over_dx(dt, dx[a])
    # a stopped clock's dt: 0 and NaN pass through as the host's division passes them
    probe.probe_step_ratios(0.0, (C.c_double * 3)(0.5, 0.25, 0.125), out)
    assert list(out) == [0.0] * 6
    probe.probe_step_ratios(float("nan"), (C.c_double * 3)(0.5, 0.25, 0.125), out)
    assert all(math.isnan(x) for x in out)
