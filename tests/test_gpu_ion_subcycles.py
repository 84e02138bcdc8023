"""The stop-rule table of tests/test_ion_subcycles.py through the DEVICE's step pick.  In production the step of a radiation
sub-cycle is picked on the device (ion_pick_body behind k_ion_pick2 and k_ion_reduce_pick, csrc/ion_pass.hip; k_ion_pick,
csrc/ion_kernels.hip) and the bookkeeping of the loop -- dt_done, the applied step, whether it was cut back, the negative flag,
spec_state -- lives beside it; physical runs never meet a tie, an exact cover, cellcount == 20 or dt_hydro == dt_done.  Here the
table's cases reach those kernels as scripted reduction words (words_script), on three routes:

  a. the C library's loop (aa_ion_radtransfer_3d_gather): the gather callback writes the scripted words of one rank or of three
     (deal_ranks: every fold over the ranks matters) -> k_ion_reduce, k_ion_pick2, the read-back, ion_subcycles, ion_root_close;
  b. the Python loops (Driver / MeshDriver.ion_radtransfer) on HipEngine / HipMeshEngine whose pass is followed by the scripted
     words: pass, pick, fetch, speculate and finish are the device's; the refined-level cases run on level 1 of a two-Domain
     mesh; two cases back to back on one Grid show that nothing leaks past `first`;
  c. aa_test_ion_pick, the function-level entry: k_ion_reduce and k_ion_reduce_pick over 1 .. AA_ION_PASS_BLOCKS' default + 1
     records against numpy's fold, and the scalars of k_ion_reduce_pick, k_ion_pick2 and k_ion_pick against ion_pick_step of
     csrc/ion_subcycle.h on every (dt_chem, dt_therm, dt_done, limit) of the table.

The Grids are athinput.ifront at 16 x 8 x 8 (the refined Domain: 16 x 8 x 8 at 8, 4, 4) with cour_no = 0.5, their zones real and
updated with the scripted steps (seconds against the deck's 1e14); nothing asserted depends on the state.  Every comparison is
exact: the expected values are the table's literals.  Both builds (the pick is one add, one compare, one subtract)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import test_ion_subcycles as T
from test_ion_subcycles import CASES, FINE_DT, BIG, DECK, probe      # noqa: F401  (probe: the header's fixture)

pytestmark = pytest.mark.gpu
COUR = 0.5
OV = ["domain1/Nx1=16", "domain1/Nx2=8", "domain1/Nx3=8", "time/cour_no=0.5"]
OV2 = ["job/num_domains=2"] + OV + ["domain2/Nx1=16", "domain2/Nx2=8", "domain2/Nx3=8", "domain2/iDisp=8", "domain2/jDisp=4", "domain2/kDisp=4"]
ROOT_CASES = [c for c in CASES if not c[1]]
driver = importlib.import_module("atmospheric-athena_amd.driver")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("atmospheric-athena_amd.lib")


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(autouse=True)
def one_rank_short_rays(monkeypatch):
    monkeypatch.delenv("AA_FORCE_DISTRIBUTED", raising=False)
    monkeypatch.setenv("AA_ION_FUSED", "1")          # rays of 16 zones on the one-kernel sub-cycle (the engines create their Grids)


def dt_hydro_of(max_dti):
    """the host's quotient (aa_ion_fetch: cour_no/max_dti)"""
    with np.errstate(divide="ignore"):
        return float(np.float64(COUR) / np.float64(max_dti))


def fetches_of(case):
    """what aa_ion_fetch returns per sub-cycle, from the script: (dt, limit_hit, cellcount, dt_hydro); a step was cut back iff it is
    not the MIN of its rates"""
    subs, steps = case[4], case[6]
    rows = T.words_script(case, COUR)
    return [(steps[n], steps[n] != min(s[0], s[1]), s[2], dt_hydro_of(rows[n + 1][2])) for n, s in enumerate(subs[:len(steps)])]


# ---- a. the C library's loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ROOT_CASES, ids=[c[0] for c in ROOT_CASES])
@pytest.mark.parametrize("nranks", [1, 3])
@pytest.mark.parametrize("spec", ["1", "0"])
@pytest.mark.parametrize("strict", [False, True])
def test_library_loop(aa, lib, torch, monkeypatch, strict, spec, nranks, case):
    """aa_ion_radtransfer_3d_gather with the scripted words as the gathered ones: niter, the root's dt afterwards, one gather per
    pass (niter + 1 of them), the two errors"""
    name, fine, limit, maxiter, subs, niter, steps, dt, dt_done, raises = case
    monkeypatch.setenv("AA_ION_SPECULATE", spec)
    run = aa.config.load(DECK, OV, "ifront"); run.maxiter = maxiter
    assert run.cour_no == COUR
    rows = T.words_script(case, COUR)
    script = [[v for r in (T.deal_ranks(row) if nranks == 3 else [row]) for v in r] for row in rows]
    dev = torch.device("cuda", 0)
    words = torch.zeros(lib.ION_WORDS, dtype=torch.float64, device=dev)
    words_all = torch.zeros(lib.ION_WORDS * nranks, dtype=torch.float64, device=dev)
    calls = [0]

    def gather():
        # the pick of the pass before has been queued, not awaited (the first pick of an ion step has no read-back behind it):
        # it must have read its words before the next ones land, and these must have landed before the next pick is queued
        torch.cuda.synchronize()
        assert calls[0] < len(script), "the script ran out"
        words_all.copy_(torch.tensor(script[calls[0]], dtype=torch.float64))
        torch.cuda.synchronize()
        calls[0] += 1

    g = lib.setup_problem(aa.config.slab(run), 0, strict, ion_path=1)
    try:
        assert g.ion_is_fused()
        g.bvals_mhd(); g.bvals_ionrad()
        g.set_mesh_state(0.0, limit, 0)
        call = lambda: g.ion_radtransfer_3d_gather(words.data_ptr(), words_all.data_ptr(), nranks, gather)
        if raises is None:
            assert (call(), g.mesh_state()[1], calls[0]) == (niter, dt, niter + 1)
        else:
            with pytest.raises(lib.AthenaError, match=raises):
                call()
        assert calls[0] == len(script)
    finally:
        g.close()


# ---- b. the Python loops on the real engines ----------------------------------------------------------------------------
class Scripted:
    """what the two engines below share: the scripted words as host rows, the fetches and the state they were handed"""

    def arm(self, case):
        t = self.torch
        self.script = [t.tensor(r, dtype=t.float64) for r in T.words_script(case, COUR)]
        self.k, self.fetched, self.state, self.prolonged = 0, [], None, None
        return self

    def next_row(self, dst):
        assert self.k < len(self.script), "the script ran out"
        dst[:len(self.script[self.k])].copy_(self.script[self.k])      # on the Grid's stream: behind the pass, in front of the pick
        self.k += 1

    steps = property(lambda s: [f[0] for f in s.fetched])


class ScriptedHip(Scripted, driver.HipEngine):
    def ion_pass(self, update, sweep):
        super().ion_pass(update, sweep); self.next_row(self.words)

    def ion_fetch(self):
        self.fetched.append(super().ion_fetch()); return self.fetched[-1]

    def set_mesh_state(self, time, dt, nstep):
        self.state = (time, dt, nstep); super().set_mesh_state(time, dt, nstep)


class ScriptedMesh(Scripted, driver.HipMeshEngine):
    def ion_gather(self, dist):
        super().ion_gather(dist); self.next_row(self.words_all)

    def ion_fetch(self, l):
        self.fetched.append(super().ion_fetch(l)); return self.fetched[-1]

    def set_level_state(self, l, time, dt, nstep):
        self.state = (time, dt, nstep); super().set_level_state(l, time, dt, nstep)

    def ionflux_prolong(self, l):
        self.prolonged = l; super().ionflux_prolong(l)


def check_fetches(eng, case):
    """per sub-cycle, what the device handed the host: the step, whether it was cut back, cells out of range, dt_hydro, the flag"""
    name, raises = case[0], case[9]
    if raises is None:
        assert [(f[0], f[1], f[4], f[5]) for f in eng.fetched] == fetches_of(case)
        assert not any(f[6] for f in eng.fetched) and eng.k == case[5] + 1 == len(eng.script)
    elif name == "negative_dt_chem":
        # the flag belongs to the rates BEHIND a step: it comes back with the update that used them
        assert [(f[0], f[6]) for f in eng.fetched] == [(1.0, False), (-1.0, True)] and eng.k == len(eng.script)
    else:
        assert [(f[0], f[1], f[6]) for f in eng.fetched] == [(case[2], True, False)] and eng.k == len(eng.script)


def run_driver(d, case):
    """test_ion_subcycles.check_driver on a Driver that exists"""
    name, fine, limit, maxiter, subs, niter, steps, dt, dt_done, raises = case
    d.run.maxiter = maxiter
    d.dt = limit
    d.eng.arm(case)
    got = T.outcome(d.ion_radtransfer, raises)
    if raises is None:
        assert (got, d.eng.steps, d.dt) == (niter, steps, dt)
        assert d.eng.state == (d.time, dt, d.nstep) == d.eng.mesh_state()
    check_fetches(d.eng, case)


@pytest.mark.parametrize("case", ROOT_CASES, ids=[c[0] for c in ROOT_CASES])
@pytest.mark.parametrize("spec", ["1", "0"])
@pytest.mark.parametrize("strict", [False, True])
def test_driver_on_the_device(aa, monkeypatch, strict, spec, case):
    """Driver._ion_radtransfer_fused on HipEngine: the assertions of test_ion_subcycles.test_driver, and every fetch"""
    monkeypatch.setenv("AA_ION_SPECULATE", spec)
    run = aa.config.load(DECK, OV, "ifront")
    d = driver.Driver(run, lambda grid: ScriptedHip(grid, 0, strict))
    try:
        assert d.eng.ion_fused
        d.start()
        run_driver(d, case)
    finally:
        d.eng.close()


MESH_CASES = [c for c in CASES if c[0] != "negative_dt"]          # (a negative root step: see test_ion_subcycles' docstring)


@pytest.mark.parametrize("case", MESH_CASES, ids=[c[0] for c in MESH_CASES])
@pytest.mark.parametrize("spec", ["1", "0"])
@pytest.mark.parametrize("strict", [False, True])
def test_mesh_driver_on_the_device(aa, monkeypatch, strict, spec, case):
    """MeshDriver._ion_radtransfer_fused on HipMeshEngine, the root level and level 1 of the two-Domain mesh: the assertions of
    test_ion_subcycles.test_mesh_driver, and every fetch"""
    name, fine, limit, maxiter, subs, niter, steps, dt, dt_done, raises = case
    monkeypatch.setenv("AA_ION_SPECULATE", spec)
    par2 = aa.athinput.ParTable.from_file(DECK).cmdline(OV2)
    run = aa.config.from_par(par2, "ifront"); run.maxiter = maxiter
    d = driver.MeshDriver(par2, run, lambda cfg: ScriptedMesh(cfg, 0, strict))
    try:
        assert (d.NL, d.nl) == (2, 2) and d.eng.ion_is_fused(0) and d.eng.ion_is_fused(1)
        d.start()
        l = 1 if fine else 0
        if fine:
            d.dtl, d.tcoarse = [FINE_DT, FINE_DT], limit
        else:
            d.dtl, d.tcoarse = [limit, limit], 123.0
        d.eng.arm(case)
        got = T.outcome(lambda: d.ion_radtransfer(l), raises)
        if raises is None:
            assert (got, d.eng.steps, d.dtl[l], d.dt) == (niter, steps, dt, dt)
            assert d.eng.state == (d.time, dt, d.nstep) == d.eng.lev[l].mesh_state()
            if fine:
                assert (d.dtl[0], d.tcoarse, d.eng.prolonged) == (FINE_DT, limit, 1)
            else:
                assert (d.tcoarse, d.dtl[1], d.eng.prolonged) == (dt_done, limit, None)
        check_fetches(d.eng, case)
    finally:
        d.eng.close()


@pytest.mark.parametrize("spec", ["1", "0"])
@pytest.mark.parametrize("strict", [False, True])
def test_nothing_leaks_into_the_next_ion_step(aa, monkeypatch, strict, spec):
    """two ion steps on one Grid: the first ends cut back at dt_done = 0.9 - 1 ulp, the second must start from dt_done = 0 (with what
    the first left it would cover its limit of 2.0 one sub-cycle early, by a step of 0.1) and from its own applied fields"""
    by_name = {c[0]: c for c in CASES}
    monkeypatch.setenv("AA_ION_SPECULATE", spec)
    run = aa.config.load(DECK, OV, "ifront")
    d = driver.Driver(run, lambda grid: ScriptedHip(grid, 0, strict))
    try:
        d.start()
        run_driver(d, by_name["hit_before_dt_hydro"])
        run_driver(d, by_name["pick_min_and_exact_cover"])
    finally:
        d.eng.close()


# ---- c. the folds and the picks, function by function -------------------------------------------------------------------
(DT_SEL, HIT, DT_DONE, DT_APPLIED, HIT_APPLIED, NEG_APPLIED, SPEC, DT_CHEM_OUT, DT_THERM_OUT, NEG_OUT,
 MAX_DTI, CELLCOUNT, DT_CHEM, DT_THERM, NEG_DT_CHEM) = range(15)          # a row of aa_test_ion_pick (include/athena_amd.h)
REDUCE_PICK, PICK2, PICK = 0, 1, 2                                         # the rows of `out`


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def ion_pick(lib, strict, rec, first, limit, armed=0, prev=None):
    """aa_test_ion_pick -> (words[2][8], out[3][16])"""
    L = lib.load(strict)
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, 5)
    words, out = np.full((2, lib.ION_WORDS), np.nan), np.full((3, lib.TEST_PICK_SCALARS), np.nan)
    if prev is not None:
        prev = np.ascontiguousarray(prev, dtype=np.float64)
        assert prev.shape == (lib.TEST_PICK_SCALARS,)
    rc = L.aa_test_ion_pick(len(rec), _dp(rec), int(first), float(limit), int(armed), None if prev is None else _dp(prev), _dp(words), _dp(out))
    assert rc == 0, L.aa_last_error().decode()
    return words, out


def row(**kw):
    v = np.zeros(16)
    for k, x in kw.items():
        v[globals()[k.upper()]] = x
    return v


NRECS = [1, 2, 255, 256, 257, 4096 + 1]          # one block's stride of 256 and both sides of it; AA_ION_PASS_BLOCKS' default + 1


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("n", NRECS)
@pytest.mark.parametrize("strict", [False, True])
def test_folds_over_the_records(lib, strict, n, where):
    """k_ion_reduce and k_ion_reduce_pick: MIN, MIN, MAX, an exact integer SUM and OR over n records, bit for bit numpy's; the
    extremum of all three in record 0 or in record n-1, the flag in record n-1 only, every cellcount 3"""
    i = np.arange(n)
    rec = np.stack([10.0 + i % 7, 20.0 + i % 5, 1.0 + i % 3, np.full(n, 3.0), np.zeros(n)], axis=1)
    e = 0 if where == "first" else n - 1
    rec[e, :3] = (1.5, 2.5, 99.0)
    rec[n - 1, 4] = 1.0
    want = np.array([rec[:, 0].min(), rec[:, 1].min(), rec[:, 2].max(), rec[:, 3].sum(), rec[:, 4].max(), 0.0, 0.0, 0.0])
    assert tuple(want[:5]) == (1.5, 2.5, 99.0, 3.0 * n, 1.0)
    words, out = ion_pick(lib, strict, rec, True, 1e300)
    assert np.array_equal(words[0], want) and np.array_equal(words[1], want)
    # ... and what the picks keep of the fold for the host's read-back
    for k in (REDUCE_PICK, PICK2):
        assert tuple(out[k][[DT_CHEM_OUT, DT_THERM_OUT, NEG_OUT, MAX_DTI, CELLCOUNT]]) == (1.5, 2.5, 1.0, 99.0, 3.0 * n)
        assert (out[k][DT_SEL], out[k][HIT]) == (1.5, 0.0)
    assert np.array_equal(out[REDUCE_PICK], out[PICK2])
    if where == "last":          # no flag anywhere: the OR of zeros
        rec[n - 1, 4] = 0.0
        words, out = ion_pick(lib, strict, rec, True, 1e300)
        assert words[0][4] == words[1][4] == out[REDUCE_PICK][NEG_OUT] == out[PICK2][NEG_OUT] == 0.0


QUADS = T.pick_quadruples()


@pytest.mark.parametrize("q", QUADS, ids=[f"{q[0]}-{q[1]}" for q in QUADS])
@pytest.mark.parametrize("strict", [False, True])
def test_picks_against_the_header(lib, probe, strict, q):
    """k_ion_reduce_pick, k_ion_pick2 and k_ion_pick on every quadruple of the table: the step and the cut of ion_pick_step; the
    one-kernel picks also book the update before them (the first pick of an ion step: none), k_ion_pick re-arms its reductions"""
    name, n, (dt_chem, dt_therm, dt_done, limit), prev_done, prev_step = q
    hit = C.c_int(-1)
    dt = probe.probe_ion_pick_step(dt_chem, dt_therm, dt_done, limit, C.byref(hit))
    first = n == 0
    # what the pick before left: its step, that it was not cut back (the loop went on) and, to tell the picks apart, a raised flag
    prev = row(dt_sel=prev_step, hit=0, neg_out=1, dt_done=prev_done, dt_applied=-7.0, hit_applied=1, neg_applied=0, spec=2)
    if first:
        prev = row(dt_sel=0.3, hit=1, neg_out=1, dt_done=0.7, dt_applied=-7.0, hit_applied=1, neg_applied=1, spec=1)   # an earlier ion step's
    words, out = ion_pick(lib, strict, [[dt_chem, dt_therm, 0.25, 5.0, 0.0]], first, limit, armed=0, prev=prev)
    for k in (REDUCE_PICK, PICK2, PICK):
        assert (out[k][DT_SEL], out[k][HIT]) == (dt, float(hit.value)), k
        assert (out[k][DT_CHEM_OUT], out[k][DT_THERM_OUT], out[k][NEG_OUT]) == (dt_chem, dt_therm, 0.0), k
    for k in (REDUCE_PICK, PICK2):
        assert (out[k][DT_DONE], out[k][SPEC], out[k][MAX_DTI], out[k][CELLCOUNT]) == (dt_done, 0.0, 0.25, 5.0), k
        if not first:
            assert (out[k][DT_APPLIED], out[k][HIT_APPLIED], out[k][NEG_APPLIED]) == (prev_step, 0.0, 1.0), k
    assert np.array_equal(out[REDUCE_PICK], out[PICK2])
    # k_ion_pick leaves the reductions of the next round armed
    assert tuple(out[PICK][[DT_CHEM, DT_THERM, NEG_DT_CHEM, MAX_DTI, CELLCOUNT]]) == (BIG, BIG, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("strict", [False, True])
def test_pick_books_the_update_before_it(lib, strict):
    """hit_applied, neg_applied and dt_applied are those of the pick BEFORE (the update the pass just applied), not of this one;
    k_ion_pick hands on the flag of its own rates"""
    prev = row(dt_sel=0.25, hit=1, neg_out=1, dt_done=0.5, dt_applied=7.0, hit_applied=0, neg_applied=0, spec=1)
    words, out = ion_pick(lib, strict, [[1.0, 2.0, 0.0, 0.0, 0.0]], False, 8.0, armed=1, prev=prev)
    for k in (REDUCE_PICK, PICK2):
        assert tuple(out[k][[DT_APPLIED, HIT_APPLIED, NEG_APPLIED, DT_DONE, DT_SEL, HIT, NEG_OUT, SPEC]]) == (0.25, 1.0, 1.0, 0.75, 1.0, 0.0, 0.0, 0.0)
    prev = row(dt_sel=0.25, hit=0, neg_out=0, dt_done=0.5)
    words, out = ion_pick(lib, strict, [[-1.0, 2.0, 0.0, 0.0, 1.0]], False, 8.0, prev=prev)
    for k in (REDUCE_PICK, PICK2):
        assert tuple(out[k][[DT_APPLIED, HIT_APPLIED, NEG_APPLIED, DT_DONE, DT_SEL, HIT, NEG_OUT]]) == (0.25, 0.0, 0.0, 0.75, -1.0, 0.0, 1.0)
    assert tuple(out[PICK][[DT_SEL, HIT, NEG_OUT, NEG_DT_CHEM]]) == (-1.0, 0.0, 1.0, 0.0)


@pytest.mark.parametrize("covered", [True, False])
@pytest.mark.parametrize("armed", [1, 0])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("strict", [False, True])
def test_spec_state(lib, strict, first, armed, covered):
    """1: the first pick of an ion step found the speculated whole step to be the one; 2: it did not; 0: nothing was speculated"""
    prev = row(dt_sel=0.0, dt_done=0.0, spec=1 + (not covered))           # (the opposite answer, to be overwritten)
    words, out = ion_pick(lib, strict, [[4.0 if covered else 0.5, 2.0 if covered else 0.5, 0.0, 0.0, 0.0]], first, 1.0, armed=armed, prev=prev)
    want = (1.0 if covered else 2.0) if (first and armed) else 0.0
    for k in (REDUCE_PICK, PICK2):
        assert (out[k][HIT], out[k][SPEC]) == (float(covered), want)
