"""ion_stop_rule of csrc/ion_subcycle.h: the stop tests of the radiation sub-cycle loop (ionrad_3d.c:982-1012) as ONE function that
the host's loop (ion_subcycles) and the device's queued pick (k_ion_reduce_pick_q, csrc/ion_pass.hip) both call.  Here it is compiled
with the host compiler into fixtures/ion_stop_rule_probe.cpp, whose loop is written the way the device books a sub-cycle, and every
case of test_ion_subcycles.CASES runs through it: niter, the steps, the level's dt, dt_done and the two errors are the table's
literals.  (tests/test_gpu_ion_batch.py runs the same table through the device.)"""
import ctypes as C
import os
import subprocess

import pytest

from test_ion_subcycles import CASES, FINE_DT, HERE, INF, PKG

GO_ON, STOP, STOP_CUT, STOP_NEG = 0, 1, 2, 3


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ion_stop_rule") / "ion_stop_rule_probe.so")
    subprocess.check_call(["g++", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(HERE, "fixtures", "ion_stop_rule_probe.cpp"), "-o", so])
    L = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.probe_ion_stop_rule.restype = C.c_int
    L.probe_ion_stop_rule.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_double, C.c_double]
    L.probe_ion_stop_loop.restype = C.c_int
    L.probe_ion_stop_loop.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, dp, ip, dp, dp, dp, ip, dp, ip]
    return L


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_table_through_the_shared_rule(probe, case):
    name, fine, limit, maxiter, subs, niter, steps, dt, dt_done, raises = case
    rows = [v for s in subs for v in (s[0], s[1], float(s[2]), s[3], float(len(s) > 4))]
    n = len(subs)
    got_niter, rc_close, stop = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    got_dt, got_tc, got_done, got_steps = C.c_double(), C.c_double(), C.c_double(), (C.c_double * n)()
    dt_in, tc_in = (FINE_DT, limit) if fine else (limit, 123.0)
    rc = probe.probe_ion_stop_loop(int(fine), limit, maxiter, dt_in, tc_in, n, (C.c_double * len(rows))(*rows), C.byref(got_niter),
                                   C.byref(got_dt), C.byref(got_tc), C.byref(got_done), C.byref(stop), got_steps, C.byref(rc_close))
    if name == "negative_dt_chem":
        # the flagged sub-cycle ends the loop before any test: it is not counted, dt_done does not move
        assert (rc, stop.value, got_niter.value, got_done.value) == (-4, STOP_NEG, 1, 1.0)
        return
    assert rc == 0 and stop.value in (STOP, STOP_CUT)
    if name == "negative_dt":
        assert rc_close.value != 0           # ionrad_3d.c:1044
        return
    assert rc_close.value == 0
    assert (got_niter.value, list(got_steps)[:got_niter.value], got_dt.value, got_done.value) == (niter, steps, dt, dt_done)
    assert got_tc.value == (limit if fine else dt_done)
    assert got_niter.value == n, "the script has sub-cycles the loop never reached"
    # a refined level always takes the cut; the root's cut is the step set to dt_done in front of ion_close_root
    if fine:
        assert stop.value == STOP_CUT
    elif niter != maxiter:
        assert (stop.value == STOP_CUT) == (dt != limit)


def test_order_and_comparison_forms(probe):
    """the reference's order and its strict comparisons, operand by operand"""
    r = probe.probe_ion_stop_rule
    # root: check_range (> 20) before hit before dt_hydro (< dt_done)
    assert r(0, 0, 20, INF, 1.0) == GO_ON and r(0, 0, 21, INF, 1.0) == STOP_CUT
    assert r(0, 1, 21, INF, 1.0) == STOP_CUT and r(0, 1, 20, 0.0, 1.0) == STOP
    assert r(0, 0, 0, 1.0, 1.0) == GO_ON and r(0, 0, 0, float.fromhex("0x1.fffffffffffffp-1"), 1.0) == STOP_CUT
    assert r(0, 0, 0, float("nan"), 1.0) == GO_ON          # (a NaN dt_hydro compares false, as in the reference)
    # refined level: hit alone, and always the cut
    assert r(1, 0, 1000, 0.0, 1.0) == GO_ON and r(1, 1, 0, INF, 1.0) == STOP_CUT
