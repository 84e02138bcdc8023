"""K radiation sub-cycles per host visit (Grid.set_ion_batch / AA_ION_BATCH; csrc/api.hip ion_run_queued, the queued entries of
csrc/ion_pass.hip).  With K > 1 the stop tests of the sub-cycle loop (ionrad_3d.c:982-1012) are applied on the device by the pick
itself, the kernels of a queued sub-cycle leave at once behind a stop, and the host reads back once per visit.  Nothing else
changes, so every comparison here is exact:

  a. K in {2, 4, 7, 64} against K = 1 in the same process: sub-cycle counts, dt after every step, state and EdgeFlux, bit for bit,
     on three inputs; the visits and executed sub-cycles the Grid counted against the visit-size rule; fewer read-backs;
  b. a step behind a one-sub-cycle step queues nothing that leaves at once (the stationary regime keeps its launches);
  c. the stop-rule table of tests/test_ion_subcycles.py through the device's loop (aa_test_ion_batch): niter, the applied steps,
     dt_done and the stop code are the table's literals, for K in {1, 2, 3, 8} and a first visit of 1 and of K;
  d. a two-level Mesh: Mesh.set_ion_batch(4) against 1;
  e. what keeps the per-sub-cycle loop: the two-kernel sub-cycle, AA_ION_FUSE_PICK=0, a Grid cut into slabs, the gather entry;
  f. the knob's range, through AA_ION_BATCH and through set_ion_batch;
  g. Driver(..., ion_batch=4) against the default Driver.
A K = 1 run is made once per (input, build, environment) and shared; nobody writes to it."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest

import test_ion_subcycles as T
from test_ion_subcycles import CASES

pytestmark = pytest.mark.gpu
DECKS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "atmospheric-athena_amd", "decks")
INPUTS = {
    # gravity, scalar, the pinned core.  With the deck's cour_no the default build takes 80, 13, 12, 11, 1, ... sub-cycles (the strict
    # one 80, 13, 12, 11, 10, 1, ...): no count of residue 2 modulo 4.  At cour_no = 0.5 the strict build takes 81, 14, 13, 15, 11,
    # 10, 8, 2, 1, ... and the default build 81, 14, 12, 14, 11, 10, 1, ...: both meet the condition asserted below
    "sphere": ("ioniz_sphere", ["domain1/Nx1=64", "domain1/Nx2=16", "domain1/Nx3=16", "time/cour_no=0.5"], 12),
    "ifront_flux": ("ifront", ["domain1/Nx1=64", "domain1/Nx2=8", "domain1/Nx3=8", "problem/flux=1e3"], 5),
    "ifront_128": ("ifront", ["domain1/Nx1=128", "domain1/Nx2=6", "domain1/Nx3=5"], 4),
}
KS = [2, 4, 7, 64]
COUR = 0.5
OV2 = ["job/num_domains=2", "domain1/Nx1=16", "domain1/Nx2=8", "domain1/Nx3=8", "time/cour_no=0.5",
       "domain2/Nx1=16", "domain2/Nx2=8", "domain2/Nx3=8", "domain2/iDisp=8", "domain2/jDisp=4", "domain2/kDisp=4"]
ION_ENV = ("AA_ION_SPECULATE", "AA_ION_LEAN", "AA_ION_FUSED", "AA_ION_FUSE_PICK", "AA_ION_BATCH")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("atmospheric-athena_amd.lib")


_runs = {}


def run_grid(aa, lib, monkeypatch, key, strict, K, env=(), nslab=1, nstep=None):
    """the input `key` for its steps with ion_batch = K (1: the Grid as it is made) -> a dict; cached"""
    ck = (key, strict, K, tuple(env), nslab, nstep)
    if ck in _runs:
        return _runs[ck]
    for name in ION_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, v in env:
        monkeypatch.setenv(name, v)
    problem, ov, n = INPUTS[key]
    run = aa.config.load(os.path.join(DECKS, "athinput." + problem), ov, problem)
    g = lib.setup_problem(aa.config.slab(run), 0, strict, nslab=nslab)
    try:
        assert g.ion_batch == 1
        if K != 1:
            g.set_ion_batch(K)
            assert g.ion_batch == K
        active = g.ion_batch_active()
        g.start()
        g.host_syncs(True)
        its, dts, counts = [], [], [g.ion_batch_counts()]
        for _ in range(nstep or n):
            its.append(g.step()); dts.append(g.dt); counts.append(g.ion_batch_counts())
        r = dict(its=its, dts=dts, U=g.download(), ef=g.download_edgeflux(), counts=counts, syncs=g.host_syncs(), active=active,
                 fused=g.ion_is_fused(), active_after=g.ion_batch_active())
    finally:
        g.close()
    _runs[ck] = r
    return r


def same(a, b, what):
    assert a["its"] == b["its"], f"{what}: sub-cycle counts {a['its']} / {b['its']}"
    assert a["dts"] == b["dts"], f"{what}: dt after every step"
    assert np.array_equal(a["U"], b["U"], equal_nan=True), f"{what}: state"
    assert np.array_equal(a["ef"], b["ef"], equal_nan=True), f"{what}: EdgeFlux"


def visits_of(its, K):
    """the visit-size rule: the first visit of an ion step queues b0 = min(K, the previous step's count) (1 in front of the first
    step), later ones K -> 1 + ceil(max(n - b0, 0) / K) visits for a step of n sub-cycles"""
    out, prev = [], 1
    for n in its:
        b0 = max(1, min(K, prev))
        out.append(1 + math.ceil(max(n - b0, 0) / K))
        prev = n
    return out


def skipped_of(its, K):
    out, prev = [], 1
    for n, v in zip(its, visits_of(its, K)):
        out.append(max(1, min(K, prev)) + (v - 1) * K - n)
        prev = n
    return out


def check_counts(r, ref, K):
    its = ref["its"]
    d = np.diff(np.array(r["counts"]), axis=0)
    print("K", K, "sub-cycles", its, "visits", list(d[:, 0]), "left at once", list(d[:, 2]), "read-backs", r["syncs"], "against", ref["syncs"])
    assert list(d[:, 0]) == visits_of(its, K)
    assert list(d[:, 1]) == its and r["counts"][-1][1] == sum(its)
    assert list(d[:, 2]) == skipped_of(its, K)


# ---- a. same bits as the per-sub-cycle loop -------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("key", list(INPUTS))
@pytest.mark.parametrize("strict", [True, False])
def test_same_bits_as_one_per_visit(aa, lib, monkeypatch, strict, key, K):
    ref = run_grid(aa, lib, monkeypatch, key, strict, 1)
    assert ref["fused"] and not ref["active"] and ref["counts"][-1] == (0, 0, 0)
    if key == "sphere":
        # asserted on the K = 1 counts: a step longer than the longest visit, every residue modulo 4, and the stationary regime
        its = ref["its"]
        assert max(its) > 64 and {n % 4 for n in its if n > 1} == {0, 1, 2, 3} and 1 in its, its
    r = run_grid(aa, lib, monkeypatch, key, strict, K)
    assert r["active"] and r["active_after"]
    same(r, ref, f"K = {K}")
    check_counts(r, ref, K)
    if K == 4:
        assert r["syncs"] < ref["syncs"]


@pytest.mark.parametrize("env", [(("AA_ION_SPECULATE", "0"),), (("AA_ION_LEAN", "0"),)], ids=["no_speculation", "no_lean"])
@pytest.mark.parametrize("key", list(INPUTS))
@pytest.mark.parametrize("strict", [True, False])
def test_same_bits_without_speculation_and_lean(aa, lib, monkeypatch, strict, key, env):
    ref = run_grid(aa, lib, monkeypatch, key, strict, 1, env)
    r = run_grid(aa, lib, monkeypatch, key, strict, 4, env)
    assert r["active"]
    same(r, ref, f"K = 4, {env}")
    same(ref, run_grid(aa, lib, monkeypatch, key, strict, 1), f"{env} against the default")
    check_counts(r, ref, 4)


# ---- b. the stationary regime keeps its launches --------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 64])
@pytest.mark.parametrize("strict", [True, False])
def test_stationary_steps_queue_nothing_in_vain(aa, lib, monkeypatch, strict, K):
    ref = run_grid(aa, lib, monkeypatch, "sphere", strict, 1)
    r = run_grid(aa, lib, monkeypatch, "sphere", strict, K)
    its, d = ref["its"], np.diff(np.array(r["counts"]), axis=0)
    quiet = [i for i in range(1, len(its)) if its[i] == 1 and its[i - 1] == 1]
    assert len(quiet) >= 3, its
    for i in quiet:
        assert tuple(d[i]) == (1, 1, 0), (i, its, d[i])


# ---- c. the stop-rule table through the device's loop ---------------------------------------------------------------------
def ion_batch_script(lib, strict, case, K, b0):
    """aa_test_ion_batch over the case's words -> (rc, message, niter, dt_done, stop, visits, left at once, steps)"""
    L = lib.load(strict)
    rec = np.ascontiguousarray([r[:5] for r in T.words_script(case, COUR)], dtype=np.float64)
    out, steps = np.full(5, np.nan), np.full(len(rec), np.nan)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.aa_test_ion_batch(len(rec), dp(rec), int(case[1]), float(case[2]), COUR, K, b0, dp(out), dp(steps))
    return rc, L.aa_last_error().decode(), int(out[0]), float(out[1]), int(out[2]), int(out[3]), int(out[4]), list(steps)


FIRST_VISITS = [(K, b0) for K in (1, 2, 3, 8) for b0 in sorted({1, K})]


@pytest.mark.parametrize("K,b0", FIRST_VISITS, ids=[f"K{K}-first{b0}" for K, b0 in FIRST_VISITS])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("strict", [False, True])
def test_table_through_the_device_loop(lib, strict, case, K, b0):
    name, fine, limit, maxiter, subs, niter, steps, dt, dt_done, raises = case
    rc, msg, got_niter, got_done, stop, visits, left, got_steps = ion_batch_script(lib, strict, case, K, b0)
    assert rc == 0, msg
    if name == "negative_dt_chem":
        # the flag comes back with the update that used its rates: sub-cycle 2 of the script; it is not counted
        flagged = [n for n, s in enumerate(subs) if len(s) > 4]
        assert (stop, got_niter, got_steps[:got_niter]) == (3, flagged[0], [1.0])
        ran = got_niter + 1
    elif name == "negative_dt":
        # one sub-cycle "covers" the negative step; the host's ion_close_root raises behind the loop
        assert (stop, got_niter, got_steps[:1], got_done) == (1, 1, [limit], limit)
        ran = 1
    else:
        assert (got_niter, got_steps[:got_niter], got_done) == (niter, steps, dt_done)
        assert stop in (1, 2)
        if fine:
            assert stop == 2
        elif niter != maxiter:
            assert (stop == 2) == (dt != limit)          # the cut is the level's dt set to dt_done
        ran = niter
    assert visits == 1 + math.ceil(max(ran - b0, 0) / K)
    assert left == b0 + (visits - 1) * K - ran


# ---- d. a Mesh ------------------------------------------------------------------------------------------------------------
def sphere_2lev():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smr_ioniz_sphere_2lev_s4.npz"))
    return [str(o) for o in g["overrides"]]


# The two-Domain ifront of test_gpu_ion_subcycles.py (OV2), 3 steps: its refined level takes ONE sub-cycle in every step ([26, 1],
# [26, 1], [11, 1] per level in both builds), so the root alone shows the queued loop there.  The refined level that sub-cycles is
# the two-level sphere of tests/test_gpu_smr.py (a 32^3 root; its level 1 takes about ten sub-cycles per step), 4 steps.
@pytest.mark.parametrize("problem,ov,nstep,fine_subcycles", [("ifront", OV2, 3, False), ("ioniz_sphere", None, 4, True)],
                         ids=["ifront_two_domains", "sphere_two_levels"])
@pytest.mark.parametrize("strict", [True, False])
def test_mesh_levels(aa, lib, monkeypatch, strict, problem, ov, nstep, fine_subcycles):
    ov = sphere_2lev() if ov is None else ov
    for name in ION_ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("AA_ION_FUSED", "1")          # rays of 16 zones on the one-kernel sub-cycle
    out = {}
    for K in (1, 4):
        par = aa.athinput.ParTable.from_file(os.path.join(DECKS, "athinput." + problem)).cmdline(ov)
        run = aa.config.from_par(par, problem)
        m = lib.Mesh(aa.config.levels(par, run), 0, strict)
        try:
            assert all(lev.ion_is_fused() for lev in m.lev)
            if K != 1:
                m.set_ion_batch(K)
            assert [lev.ion_batch for lev in m.lev] == [K, K] and [lev.ion_batch_active() for lev in m.lev] == [K > 1] * 2
            m.start()
            its, dts = [], []
            for _ in range(nstep):
                its.append(m.step()); dts.append(m.dt)
            out[K] = (its, dts, [lev.download() for lev in m.lev], [lev.download_edgeflux() for lev in m.lev],
                      [lev.dt for lev in m.lev], [lev.ion_batch_counts() for lev in m.lev])
        finally:
            m.close()
    a, b = out[1], out[4]
    print("sub-cycles per step and level:", a[0], "counts at K = 4:", b[5])
    assert max(n[0] for n in a[0]) > 1, a[0]
    if fine_subcycles:
        assert max(n[1] for n in a[0]) > 1, a[0]          # level 1 took more than one sub-cycle in at least one step, at K = 1
    assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4]
    for l in range(2):
        assert np.array_equal(a[2][l], b[2][l], equal_nan=True), l
        assert np.array_equal(a[3][l], b[3][l], equal_nan=True), l
        assert a[5][l] == (0, 0, 0) and b[5][l][1] == sum(n[l] for n in a[0])


# ---- e. what keeps the per-sub-cycle loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("env,nslab", [((("AA_ION_FUSED", "0"),), 1), ((("AA_ION_FUSE_PICK", "0"),), 1), ((), 2)],
                         ids=["two_kernel", "unfused_pick", "two_slabs"])
@pytest.mark.parametrize("strict", [True, False])
def test_old_loop_is_kept(aa, lib, monkeypatch, strict, env, nslab):
    key, nstep = ("sphere", 6) if nslab > 1 else ("ifront_flux", None)
    ref = run_grid(aa, lib, monkeypatch, key, strict, 1, env, nslab, nstep)
    r = run_grid(aa, lib, monkeypatch, key, strict, 4, env, nslab, nstep)
    assert not r["active"] and not r["active_after"] and r["counts"][-1] == (0, 0, 0)
    assert max(ref["its"]) > 1
    same(r, ref, f"{env} nslab {nslab}")
    assert r["syncs"] == ref["syncs"]


@pytest.mark.parametrize("strict", [True, False])
def test_gather_entry_keeps_the_old_loop(aa, lib, monkeypatch, strict):
    torch = importlib.import_module("torch")
    for name in ION_ENV:
        monkeypatch.delenv(name, raising=False)
    problem, ov, _ = INPUTS["ifront_flux"]
    out = {}
    for K in (1, 4):
        run = aa.config.load(os.path.join(DECKS, "athinput." + problem), ov, problem)
        g = lib.setup_problem(aa.config.slab(run), 0, strict)
        try:
            g.set_stream(torch.cuda.current_stream().cuda_stream)
            dev = torch.device("cuda", 0)
            words = torch.zeros(lib.ION_WORDS, dtype=torch.float64, device=dev)
            words_all = torch.zeros(lib.ION_WORDS, dtype=torch.float64, device=dev)
            if K != 1:
                g.set_ion_batch(K)
            g.start()
            g.host_syncs(True)
            its = [g.ion_radtransfer_3d_gather(words.data_ptr(), words_all.data_ptr(), 1, lambda: words_all.copy_(words)) for _ in range(2)]
            out[K] = (its, g.dt, g.download(), g.download_edgeflux(), g.host_syncs(), g.ion_batch_active(), g.ion_batch_counts())
        finally:
            g.close()
    a, b = out[1], out[4]
    assert max(a[0]) > 1, a[0]
    assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4]
    assert np.array_equal(a[2], b[2], equal_nan=True) and np.array_equal(a[3], b[3], equal_nan=True)
    assert not b[5] and b[6] == (0, 0, 0)


# ---- f. the knob ----------------------------------------------------------------------------------------------------------
def test_knob_range(aa, lib, monkeypatch):
    for name in ION_ENV:
        monkeypatch.delenv(name, raising=False)
    problem, ov, _ = INPUTS["ifront_flux"]
    run = aa.config.load(os.path.join(DECKS, "athinput." + problem), ov, problem)
    for bad in (0, -1, 257):
        monkeypatch.setenv("AA_ION_BATCH", str(bad))
        with pytest.raises(lib.AthenaError, match=r"AA_ION_BATCH=%d.*256" % bad):
            lib.setup_problem(aa.config.slab(run), 0, True)
    monkeypatch.setenv("AA_ION_BATCH", "256")
    g = lib.setup_problem(aa.config.slab(run), 0, True)
    try:
        assert g.ion_batch == 256 and g.ion_batch_active()
        for bad in (0, -1, 257):
            with pytest.raises(lib.AthenaError, match=r"ion_batch=%d.*256" % bad):
                g.set_ion_batch(bad)
            assert g.ion_batch == 256
        g.set_ion_batch(1)
        assert g.ion_batch == 1 and not g.ion_batch_active()
        g.set_ion_batch(256)
        assert g.ion_batch == 256 and g.ion_batch_active()
    finally:
        g.close()
    monkeypatch.delenv("AA_ION_BATCH")
    g = lib.setup_problem(aa.config.slab(run), 0, True)
    try:
        assert g.ion_batch == 1 and not g.ion_batch_active()
    finally:
        g.close()


# ---- g. the Driver --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False])
def test_driver_keyword(aa, monkeypatch, strict):
    driver = importlib.import_module("atmospheric-athena_amd.driver")
    for name in ION_ENV + ("AA_FORCE_DISTRIBUTED",):
        monkeypatch.delenv(name, raising=False)
    problem, ov, nstep = INPUTS["ifront_flux"]
    out = {}
    for kw in ({}, {"ion_batch": 4}):
        run = aa.config.load(os.path.join(DECKS, "athinput." + problem), ov, problem)
        d = driver.Driver(run, strict=strict, **kw)
        try:
            assert d.eng.g.ion_batch == kw.get("ion_batch", 1) and d.eng.g.ion_batch_active() == bool(kw)
            d.start()
            times, dts = [], []
            for _ in range(nstep):
                d.step(); times.append(d.time); dts.append(d.dt)
            out[bool(kw)] = (times, dts, list(d.niter_trace), d.eng.g.download(), d.eng.g.download_edgeflux(), d.eng.g.ion_batch_counts())
            if kw:
                # ... and the ion step on its own: the library's loop, the step it may cut read back
                n = d.ion_radtransfer()
                assert n >= 1 and d.dt == d.eng.mesh_state()[1]
        finally:
            d.eng.close()
    a, b = out[False], out[True]
    assert max(a[2]) > 1, a[2]
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[3], b[3], equal_nan=True) and np.array_equal(a[4], b[4], equal_nan=True)
    assert a[5] == (0, 0, 0) and b[5][1] == sum(a[2])
