"""The control flow of the radiation sub-cycle loop (ionrad_3d.c:919-1047) as a table of scripted cases: which sub-cycle ends
the loop, what the level's dt is afterwards and what time the loop covered.  A case scripts, per sub-cycle, what the rates and
the update hand back -- (dt_chem, dt_therm, cells out of range, dt_hydro) -- and states the outcome as literals.

The same scripts drive
  * the four loops of driver.py -- Driver.ion_radtransfer, Driver._ion_radtransfer_fused, MeshDriver.ion_radtransfer and
    MeshDriver._ion_radtransfer_fused -- through tiny scripted engines on one rank (the one-kernel forms emulate pick and fetch
    the way test_distributed_gloo.OracleFusedEngine does), and
  * csrc/ion_subcycle.h -- the loop, the step pick and the root closing of the C library -- through
    fixtures/ion_subcycle_probe.cpp, built with the host compiler (no device).
words_script states a case as the reduction words of the one-kernel sub-cycle's passes: tests/test_gpu_ion_subcycles.py writes
them to the device and drives the real kernels with them; here they are checked on their own and through the emulated pick.

Not scripted for MeshDriver: a root step that is negative on entry (the last case).  The reference's sanity check :1044 is the
root's on a refined Mesh too; the case runs on Driver and on the header."""
import copy
import ctypes as C
import importlib
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
PKG = os.path.join(os.path.dirname(HERE), "atmospheric-athena_amd")
DECK = os.path.join(PKG, "decks", "athinput.ifront")

INF = float("inf")
H = float.fromhex
# 0.2 + (0.9 - 0.2) is one bit short of 0.9: a loop that ends by covering the step leaves dt_done != limit, so "dt untouched"
# and "dt = dt_done" differ
LIMIT = 0.9                               # 0x1.ccccccccccccdp-1
REST = H("0x1.6666666666666p-1")          # 0.9 - 0.2
SHORT = H("0x1.cccccccccccccp-1")         # 0.2 + REST
BELOW2 = H("0x1.fffffffffffffp+0")        # the double below 2.0

# id, fine, limit, maxiter, sub-cycles (dt_chem, dt_therm, cellcount, dt_hydro[, negative-dt_chem flag]),
#   -> niter, the steps applied, the level's dt afterwards, dt_done (the root's: tcoarse), the error raised (or None)
# A root level enters with dt = limit; a refined level enters with dt = 3.0 under a root that keeps dt = 3.0, tcoarse = limit.
CASES = [
    # :951-954 the step is cut back to the hydro step; :989 hydro_done ends the loop, pGrid->dt untouched
    ("whole_step", False, 1.0, 100, [(4.0, 2.0, 0, INF)], 1, [1.0], 1.0, 1.0, None),
    # :945 MIN(dt_therm, dt_chem) whichever is smaller, or equal; :951 `>`: covering the step exactly is no hit, the next
    # sub-cycle is cut back to a step of 0
    ("pick_min_and_exact_cover", False, 2.0, 100, [(1.0, 4.0, 0, INF), (4.0, 1.0, 0, INF), (1.0, 1.0, 0, INF)],
     3, [1.0, 1.0, 0.0], 2.0, 2.0, None),
    # :982-986 check_range = cellcount > MAXCELLCOUNT (ionrad.h:38: 20): 20 goes on, 21 stops with pGrid->dt = dt_done
    ("cellcount_20_goes_on_21_stops", False, 8.0, 100, [(1.0, 2.0, 20, INF), (1.0, 2.0, 21, INF)], 2, [1.0, 1.0], 2.0, 2.0, None),
    # :997-1002 dt_hydro < dt_done: equal goes on, one bit below stops with pGrid->dt = dt_done
    ("dt_hydro_equal_goes_on_below_stops", False, 8.0, 100, [(1.0, 2.0, 0, 1.0), (1.0, 2.0, 0, BELOW2)], 2, [1.0, 1.0], 2.0, 2.0, None),
    # :989 stands before :997: a sub-cycle that covers the step AND finds dt_hydro < dt_done leaves pGrid->dt untouched
    ("hit_before_dt_hydro", False, LIMIT, 100, [(0.2, 4.0, 0, INF), (4.0, 4.0, 0, 0.0)], 2, [0.2, REST], LIMIT, SHORT, None),
    # :982 stands before :989: cells out of range AND the step covered takes the cut
    ("cellcount_before_hit", False, LIMIT, 100, [(0.2, 4.0, 0, INF), (4.0, 4.0, 21, INF)], 2, [0.2, REST], SHORT, SHORT, None),
    # :1022-1025 niter == maxiter, tested after the loop: pGrid->dt = dt_done (hit_before_dt_hydro without it: untouched)
    ("maxiter_after_loop", False, LIMIT, 2, [(0.2, 4.0, 0, INF), (4.0, 4.0, 0, INF)], 2, [0.2, REST], SHORT, SHORT, None),
    # :919 the loop has no iteration cap: niter passes maxiter = 1 inside, nothing stops, nothing touches pGrid->dt
    ("maxiter_passed_inside_loop", False, LIMIT, 1, [(0.2, 4.0, 0, INF), (2.0 ** -60, 4.0, 0, INF), (4.0, 4.0, 0, INF)],
     3, [0.2, 2.0 ** -60, REST], LIMIT, SHORT, None),
    # :1004-1012 a refined level ignores check_range, dt_hydro and maxiter; :958-961, :1008-1011 it stops when tcoarse is
    # covered and sets its own pGrid->dt = dt_done; :1017 the root's dt and tcoarse stay
    ("fine_ignores_root_rules", True, LIMIT, 2, [(0.2, 4.0, 1000, 0.0), (4.0, 4.0, 1000, 0.0)], 2, [0.2, REST], SHORT, SHORT, None),
    ("fine_whole_step", True, 1.0, 1, [(4.0, 2.0, 21, 0.0)], 1, [1.0], 1.0, 1.0, None),
    # :389-391 compute_chem_rates' negative dt_chem (the one-kernel forms carry it as a flag of the rates behind the step)
    ("negative_dt_chem", False, 8.0, 100, [(1.0, 2.0, 0, INF), (-1.0, 2.0, 0, INF, 1)], None, None, None, None, "negative dt_chem"),
    # :1044 the sanity check: the step handed in was negative, one sub-cycle "covers" it
    ("negative_dt", False, -1.0, 100, [(1.0, 1.0, 0, INF)], None, None, None, None, r"\[ion_radtransfer_3d\]: dt = "),
]
FINE_DT = 3.0
BIG = 1.7976931348623157e308              # DBL_MAX: the neutral element of the two MIN reductions


# ---- the same cases as the reduction words of the one-kernel sub-cycle (tests/test_gpu_ion_subcycles.py writes them to the device)
def max_dti_for(dt_hydro, cour_no):
    """The device carries max_dti, the host forms dt_hydro = cour_no/max_dti: the max_dti of a scripted dt_hydro.  INF is 0 (no
    zone moves), 0.0 is inf (the division gives 0), else the smallest max_dti whose quotient does not pass dt_hydro: the quotient
    is dt_hydro where a double gives it, and the largest double the division can give below it otherwise."""
    import numpy as np
    if dt_hydro == INF:
        return 0.0
    if dt_hydro == 0.0:
        return INF
    c, m = np.float64(cour_no), np.float64(cour_no) / np.float64(dt_hydro)
    while c / m > dt_hydro:
        m = np.nextafter(m, np.float64(INF))
    while c / np.nextafter(m, np.float64(0.0)) <= dt_hydro:
        m = np.nextafter(m, np.float64(0.0))
    return float(m)


def words_script(case, cour_no):
    """A case as the words of its passes, 8 doubles each: dt_chem, dt_therm, max_dti, cellcount, neg, 0, 0, 0.  Pass n carries the
    rates of sub-cycle n and the update operands of sub-cycle n-1 (the mapping of Fused.ion_pass): pass 0 has no update behind it,
    the pass behind the script's last sub-cycle has no rates (its sweep is the speculative one), and a step that was cut back to
    the limit leaves the rates of its pass untaken -- all of these come as the neutral elements DBL_MAX / 0."""
    limit, subs = case[2], case[4]
    rows, dt_done, cut = [], 0.0, False
    for n in range(len(subs) + 1):
        dt_chem = dt_therm = BIG
        max_dti = cellcount = neg = 0.0
        if n > 0:
            cellcount, max_dti = float(subs[n - 1][2]), max_dti_for(subs[n - 1][3], cour_no)
        if n < len(subs) and not cut:
            dt_chem, dt_therm, neg = subs[n][0], subs[n][1], float(len(subs[n]) > 4)
            dt = dt_therm if dt_therm < dt_chem else dt_chem               # :945, :951: the step this pass's rates lead to
            cut = dt_done + dt > limit
            dt_done += (limit - dt_done) if cut else dt
        rows.append((dt_chem, dt_therm, max_dti, cellcount, neg, 0.0, 0.0, 0.0))
    return rows


def deal_ranks(row):
    """One pass's words dealt over three ranks so that every fold of k_ion_pick2 matters: the minimum dt_chem on the last rank,
    the minimum dt_therm on the first, the maximum max_dti on the middle one, the cell count in thirds (21 = 7+7+7, 20 = 7+7+6),
    the negative flag on one rank only; DBL_MAX / 0 on the others -> 3 x 8 doubles"""
    dt_chem, dt_therm, max_dti, cellcount, neg = row[:5]
    c = int(cellcount)
    third = [c // 3 + (1 if r < c % 3 else 0) for r in range(3)]
    return [(BIG, dt_therm, 0.0, float(third[0]), 0.0, 0.0, 0.0, 0.0),
            (BIG, BIG, max_dti, float(third[1]), neg, 0.0, 0.0, 0.0),
            (dt_chem, BIG, 0.0, float(third[2]), 0.0, 0.0, 0.0, 0.0)]


def pick_quadruples():
    """every (dt_chem, dt_therm, dt_done, limit) a pick meets in the table, with the step and the dt_done of the sub-cycle before
    it (0, 0 in front of the first: dt_done = prev_done + prev_step is the loop's own sum) -> (case, n, quadruple, prev_done, prev_step)"""
    out = []
    for c in CASES:
        limit, subs = c[2], c[4]
        prev_done, prev_step = 0.0, 0.0
        for n, s in enumerate(subs):
            dt_done = prev_done + prev_step
            out.append((c[0], n, (s[0], s[1], dt_done, limit), prev_done, prev_step))
            dt = s[1] if s[1] < s[0] else s[0]
            prev_done, prev_step = dt_done, (limit - dt_done if dt_done + dt > limit else dt)
    return out


def fold_ranks(rows):
    """k_ion_pick2's fold over the ranks' words, in plain Python: MIN, MIN, MAX, SUM, OR"""
    return (min(r[0] for r in rows), min(r[1] for r in rows), max(r[2] for r in rows), float(sum(r[3] for r in rows)),
            float(any(r[4] != 0.0 for r in rows)), 0.0, 0.0, 0.0)


# ---- scripted engines -------------------------------------------------------------------------------------------------
class Phased:
    """rates / update of the two-kernel sub-cycle from the script (Driver's engine protocol)"""

    def __init__(self, subs):
        self.subs, self.n, self.steps, self.state = subs, 0, [], None

    def ion_begin(self): self.n = 0
    def ion_rates(self): return self.subs[self.n][0], self.subs[self.n][1]

    def ion_update(self, dt):
        s = self.subs[self.n]
        self.n += 1
        self.steps.append(dt)
        return s[2], s[3]

    def set_mesh_state(self, time, dt, nstep): self.state = (time, dt, nstep)


class Fused(Phased):
    """pass / pick / fetch of the one-kernel sub-cycle on the same script: pass n applies update(n-1) with the step the last pick
    chose and, unless that step was cut back to the limit, takes rates(n); the pick books the applied update and chooses the
    next step (the arithmetic of k_ion_pick2); the sweep after the script's last sub-cycle is the speculative one"""
    ion_fused = True
    BIG = 1.7976931348623157e308

    def __init__(self, subs):
        super().__init__(subs)
        self.sc = dict(dt_sel=0.0, hit=False, neg=False, dt_done=0.0, dt_applied=0.0, hit_applied=False, neg_applied=False,
                       count=0, dt_hydro=self.BIG)
        self.words, self.finished = None, False

    def ion_pass(self, update, sweep):
        cnt, dth, dtc, dtt, neg = 0, self.BIG, self.BIG, self.BIG, False
        if update:
            cnt, dth = Phased.ion_update(self, self.sc["dt_sel"])
            if self.sc["hit"]:
                sweep = False
        if sweep and self.n < len(self.subs):
            dtc, dtt = Phased.ion_rates(self)
            neg = len(self.subs[self.n]) > 4
        self.words = (dtc, dtt, dth, cnt, neg)

    def ion_pick(self, dist, first, limit):
        assert dist is None
        dt_chem, dt_therm, dt_hydro, count, neg = self.words
        sc = self.sc
        if not first:
            sc["dt_applied"], sc["hit_applied"], sc["neg_applied"] = sc["dt_sel"], sc["hit"], sc["neg"]
            sc["dt_done"] = sc["dt_done"] + sc["dt_sel"]
        else:
            sc["dt_done"] = 0.0
        sc["count"], sc["dt_hydro"] = count, dt_hydro
        dt = dt_therm if dt_therm < dt_chem else dt_chem
        hit = False
        if sc["dt_done"] + dt > limit:
            dt = limit - sc["dt_done"]; hit = True
        sc["dt_sel"], sc["hit"], sc["neg"] = dt, hit, neg

    def ion_fetch(self):
        sc = self.sc
        return sc["dt_applied"], sc["hit_applied"], 0.0, 0.0, sc["count"], sc["dt_hydro"], sc["neg_applied"]

    def ion_finish(self): self.finished = True


def mesh_engine(base, subs):
    """the same engine behind MeshDriver's protocol: every call names its level first"""
    class Mesh(base):
        def ion_begin(self, l): base.ion_begin(self)
        def ion_rates(self, l): return base.ion_rates(self)
        def ion_update(self, l, dt): return base.ion_update(self, dt)
        def set_level_state(self, l, time, dt, nstep): self.state = (time, dt, nstep)
        def ionflux_prolong(self, l): self.prolonged = l
        if issubclass(base, Fused):
            def ion_is_fused(self, l): return True
            def ion_pass(self, l, update, sweep): base.ion_pass(self, update, sweep)
            def ion_gather(self, dist): assert dist is None
            def ion_pick(self, l, nranks, first, limit): assert nranks == 1; base.ion_pick(self, None, first, limit)
            def ion_fetch(self, l): return base.ion_fetch(self)
            def ion_finish(self, l): base.ion_finish(self)
    return Mesh(subs)


@pytest.fixture(scope="module")
def decks():
    aa = importlib.import_module("atmospheric-athena_amd")
    driver = importlib.import_module("atmospheric-athena_amd.driver")
    ov = ["domain1/Nx1=16", "domain1/Nx2=8", "domain1/Nx3=8"]
    run1 = aa.config.load(DECK, ov, "ifront")
    par2 = aa.athinput.ParTable.from_file(DECK).cmdline(
        ["job/num_domains=2"] + ov + ["domain2/Nx1=16", "domain2/Nx2=8", "domain2/Nx3=8",
                                      "domain2/iDisp=8", "domain2/jDisp=4", "domain2/kDisp=4"])
    return driver, run1, par2, aa.config.from_par(par2, "ifront")


@pytest.fixture(autouse=True)
def one_rank(monkeypatch):
    monkeypatch.delenv("AA_FORCE_DISTRIBUTED", raising=False)


def combos(mesh):
    """(case, engine) for a runner: a Driver has a root level only; the two-kernel form has no negative-dt_chem flag (its rates
    call fails inside the library); MeshDriver and a negative root step: see the module's docstring"""
    out = []
    for c in CASES:
        for e in (Phased, Fused):
            if (c[1] and not mesh) or (c[0] == "negative_dt" and mesh) or (c[0] == "negative_dt_chem" and e is Phased):
                continue
            out.append(pytest.param(c, e, id=f"{c[0]}-{'phased' if e is Phased else 'fused'}"))
    return out


def outcome(call, raises):
    if raises is None:
        return call()
    with pytest.raises(RuntimeError, match=raises):
        call()
    return None


@pytest.mark.parametrize("case,engine", combos(mesh=False))
def test_driver(decks, case, engine):
    """Driver.ion_radtransfer (two-kernel form) and Driver._ion_radtransfer_fused (it dispatches on the engine's ion_fused)"""
    check_driver(decks, case, engine)


def check_driver(decks, case, engine):
    name, fine, limit, maxiter, subs, niter, steps, dt, dt_done, raises = case
    driver, run1, _, _ = decks
    run = copy.copy(run1); run.maxiter = maxiter
    d = driver.Driver(run, lambda grid: engine(subs))
    d.dt = limit
    got = outcome(d.ion_radtransfer, raises)
    if raises is None:
        assert (got, d.eng.steps, d.dt) == (niter, steps, dt)
        assert d.eng.state == (d.time, dt, d.nstep)
        assert engine is Phased or d.eng.finished
    return d


@pytest.mark.parametrize("case,engine", combos(mesh=True))
def test_mesh_driver(decks, case, engine):
    """MeshDriver.ion_radtransfer and MeshDriver._ion_radtransfer_fused, on the root level and on a refined one"""
    check_mesh_driver(decks, case, engine)


def check_mesh_driver(decks, case, engine):
    name, fine, limit, maxiter, subs, niter, steps, dt, dt_done, raises = case
    driver, _, par2, run2 = decks
    run = copy.copy(run2); run.maxiter = maxiter
    d = driver.MeshDriver(par2, run, lambda cfg: mesh_engine(engine, subs))
    assert (d.NL, d.nl) == (2, 2)
    l = 1 if fine else 0
    if fine:
        d.dtl, d.tcoarse = [FINE_DT, FINE_DT], limit
    else:
        d.dtl, d.tcoarse = [limit, limit], 123.0          # (the root clears tcoarse itself, :891)
    got = outcome(lambda: d.ion_radtransfer(l), raises)
    if raises is None:
        assert (got, d.eng.steps, d.dtl[l], d.dt) == (niter, steps, dt, dt)     # :1033 pMesh->dt = pGrid->dt
        assert d.eng.state == (d.time, dt, d.nstep)
        if fine:
            assert (d.dtl[0], d.tcoarse, d.eng.prolonged) == (FINE_DT, limit, 1)
        else:
            assert (d.tcoarse, d.dtl[1]) == (dt_done, limit)
        assert engine is Phased or d.eng.finished
    return d


# ---- the C library's header -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ion_subcycle") / "ion_subcycle_probe.so")
    subprocess.check_call(["g++", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(HERE, "fixtures", "ion_subcycle_probe.cpp"), "-o", so])
    L = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.probe_ion_subcycles.restype = C.c_int
    L.probe_ion_subcycles.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, dp, ip, dp, dp, dp, ip]
    L.probe_maxcellcount.restype = C.c_int
    L.probe_ion_pick_step.restype = C.c_double
    L.probe_ion_pick_step.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, ip]
    return L


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_header(probe, case):
    """ion_subcycles, ion_pick_step and ion_close_root of csrc/ion_subcycle.h under a scripted callable: the same literals"""
    name, fine, limit, maxiter, subs, niter, steps, dt, dt_done, raises = case
    rows = [v for s in subs for v in (s[0], s[1], float(s[2]), s[3], float(len(s) > 4))]
    n = len(subs)
    got_niter, rc_close = C.c_int(-1), C.c_int(-1)
    got_dt, got_tc, got_steps = C.c_double(), C.c_double(), (C.c_double * n)()
    dt_in, tc_in = (FINE_DT, limit) if fine else (limit, 123.0)
    rc = probe.probe_ion_subcycles(int(fine), limit, maxiter, dt_in, tc_in, n, (C.c_double * len(rows))(*rows),
                                   C.byref(got_niter), C.byref(got_dt), C.byref(got_tc), got_steps, C.byref(rc_close))
    if name == "negative_dt_chem":
        assert rc == -4              # the callable's own code comes back at once
        return
    assert rc == 0
    if name == "negative_dt":
        assert rc_close.value != 0
        return
    assert rc_close.value == 0
    assert (got_niter.value, list(got_steps)[:got_niter.value], got_dt.value) == (niter, steps, dt)
    assert got_tc.value == (limit if fine else dt_done)


def test_header_maxcellcount(probe, decks):
    assert probe.probe_maxcellcount() == decks[0].MAXCELLCOUNT == 20          # ionrad.h:38


# ---- the cases as reduction words -------------------------------------------------------------------------------------
COURS = [0.5, 0.4]          # what the runs on the device use (1.0 is max_dti = 0.5), and the deck's own


@pytest.mark.parametrize("cour_no", COURS)
def test_words_script_encodings(cour_no):
    """words_script states dt_hydro as max_dti: with numpy's float64 division cour_no/max_dti is INF, 0 or the scripted value --
    or, where no double gives it, the largest quotient below -- and compares with dt_done as the case needs"""
    import numpy as np
    c = np.float64(cour_no)
    seen = set()
    for case in CASES:
        subs, steps = case[4], case[6]
        rows = words_script(case, cour_no)
        assert len(rows) == len(subs) + 1 and all(len(r) == 8 and r[5:] == (0.0, 0.0, 0.0) for r in rows)
        assert rows[0][2:5] == (0.0, 0.0, float(len(subs[0]) > 4)) and rows[-1][:2] == (BIG, BIG)
        dt_done = 0.0
        for n, s in enumerate(subs):
            m = np.float64(rows[n + 1][2])
            with np.errstate(divide="ignore"):
                q = c / m
            if s[3] == INF:
                assert m == 0.0 and q == INF
            elif s[3] == 0.0:
                assert q == 0.0
            else:
                assert q <= s[3] and c / np.nextafter(m, np.float64(0.0)) > s[3]        # the largest quotient that does not pass it
                seen.add((s[3], float(q)))
            assert rows[n + 1][3] == s[2]
            if steps is not None and n < len(steps):
                dt_done += steps[n]
                assert (q < dt_done) == (s[3] < dt_done), (case[0], n)
    if cour_no == 0.5:
        # "equal goes on, one bit below stops": 1.0 is exact; no quotient of 0.5 is the double below 2.0, the next one down is taken
        assert seen == {(1.0, 1.0), (BELOW2, H("0x1.ffffffffffffep+0"))}


def test_deal_ranks_folds_back():
    for case in CASES:
        for row in words_script(case, 0.5):
            dealt = deal_ranks(row)
            assert fold_ranks(dealt) == row
            # every fold matters: no rank alone, and no two ranks, give the row (unless the row is neutral in that word)
            assert dealt[2][0] == row[0] and dealt[0][1] == row[1] and dealt[1][2] == row[2] and dealt[1][4] == row[4]
            assert dealt[0][0] == dealt[1][0] == BIG and dealt[1][1] == dealt[2][1] == BIG and dealt[0][2] == dealt[2][2] == 0.0
    assert [r[3] for r in deal_ranks((1.0, 1.0, 0.0, 21.0, 0.0))] == [7.0, 7.0, 7.0]
    assert [r[3] for r in deal_ranks((1.0, 1.0, 0.0, 20.0, 0.0))] == [7.0, 7.0, 6.0]


def test_pick_quadruples_follow_the_table(probe):
    """the quadruples walk the cases with the steps the table states, and the header's ion_pick_step gives those steps on them"""
    quads = pick_quadruples()
    assert len(quads) == sum(len(c[4]) for c in CASES)
    for c in CASES:
        mine = [q for q in quads if q[0] == c[0]]
        assert [q[2][2] for q in mine][0] == 0.0 and all(q[2][2] == q[3] + q[4] for q in mine)
        if c[6] is not None:
            assert [q[4] for q in mine[1:]] == c[6][:-1]
            for q, step in zip(mine, c[6]):
                hit = C.c_int(-1)
                assert probe.probe_ion_pick_step(*q[2], C.byref(hit)) == step and hit.value in (0, 1)


class Worded(Fused):
    """Fused fed from words_script: its pass takes the pass's row instead of reading the sub-cycles (the update still books the
    step it applied); dt_hydro is the host's quotient cour_no/max_dti"""

    def __init__(self, case, cour_no):
        super().__init__(case[4])
        self.rows, self.cour_no, self.k = words_script(case, cour_no), cour_no, 0

    def ion_begin(self): self.n = self.k = 0

    def ion_pass(self, update, sweep):
        import numpy as np
        if update:
            self.steps.append(self.sc["dt_sel"]); self.n += 1
        r = self.rows[self.k]; self.k += 1
        with np.errstate(divide="ignore"):
            self.words = (r[0], r[1], float(np.float64(self.cour_no) / np.float64(r[2])), int(r[3]), r[4] != 0.0)


def worded(case, cour_no):
    """Worded as an engine class that is built from the sub-cycles, as Phased and Fused are"""
    class W(Worded):
        def __init__(self, subs): Worded.__init__(self, case, cour_no)
    return W


def worded_combos(mesh):
    return [pytest.param(c, cour, id=f"{c[0]}-{cour}") for c in CASES for cour in COURS
            if not ((c[1] and not mesh) or (c[0] == "negative_dt" and mesh))]


@pytest.mark.parametrize("case,cour_no", worded_combos(mesh=False))
def test_words_script_driver(decks, case, cour_no):
    """the words give the table's outcomes through the emulated pick of Fused and Driver's loop: the script is right before it
    reaches a device"""
    d = check_driver(decks, case, worded(case, cour_no))
    assert case[9] is not None or d.eng.k == case[5] + 1              # niter + 1 passes, the script did not run out


@pytest.mark.parametrize("case,cour_no", worded_combos(mesh=True))
def test_words_script_mesh_driver(decks, case, cour_no):
    d = check_mesh_driver(decks, case, worded(case, cour_no))
    assert case[9] is not None or d.eng.k == case[5] + 1
