"""aa_mesh_run_3d / Mesh.run_3d on an MI355X: many steps of a refined 3-D mesh per host visit, the time step picked on the device
for all levels (csrc/smr.hip mesh_queue_step_3d; csrc/flux2_update_kernel.h k_flux2_update_keep_dc; csrc/smr_coupling_kernels.h
k_restrict_dc, k_flux_correct_dc, k_box_copy_dc; csrc/hydro3d_clock.hip k3d_mesh_seed, k3d_mesh_advance; the frame is csrc/run.hip's).

AA_CORRECT_ALL=1 puts the small levels of the fixtures on the kernels a Grid of 4e5 zones or more takes, the chain that has entries
on the device clock (tests/test_gpu_smr.py test_levels_on_the_big_grid_kernels_vs_reference does the same for Mesh.step()).

Two references, as tests/test_gpu_2d_smr_run.py has them for a 2-D Mesh.  The states the reference's own SMR builds left
(tests/golden/smr_*.npz, hydromatrix_*smr_3d_ctu_n3.npz): the strict library bit for bit on every level with time and dt, the
default library within the bars tests/test_gpu_smr.py and tests/test_gpu_hydro_branches.py hold Mesh.step() to on the same
fixtures.  And Mesh.step() of the same library with the same knobs: run_3d gives its bits in BOTH libraries -- the whole block of
every level, ghost zones and corners included, and (time, dt, nstep) -- so a step queued behind the stop that stored anything,
anywhere, shows; two further step() calls behind a call that stopped inside a batch show a stale prolongation snapshot or kept
flux plane."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import hydromatrix as hm                 # noqa: E402
import meshfix                           # noqa: E402
import orc                               # noqa: E402
import twins                             # noqa: E402
import test_gpu_hydro_branches as hb     # noqa: E402  (fixture cache, error measure and the default build's rule for the designed state)
from dumpfix import pkg                  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(HERE, "golden")
NG = 4
FAR = 1.0e300                            # a t_stop no run reaches: the step count ends the call
BLAST = ["smr_blast_3lev_s6", "smr_blast_3lev_edge_s8", "smr_blast_2dom_s6", "smr_blast_tree_s5", "smr_ppm_blast_2lev_s5"]
DESIGNED = [("3d_ctu", 0), ("3d_ctu", 1)]      # hydromatrix_smr_3d_ctu_n3, hydromatrix_s1_smr_3d_ctu_n3
STOP = ["smr_blast_3lev_edge_s8", "smr_blast_tree_s5"]
NTRAJ = 12


@pytest.fixture(autouse=True)
def big_grid_kernels(monkeypatch):
    monkeypatch.setenv("AA_CORRECT_ALL", "1")


_gold = {}


def gold(name):
    if name not in _gold:
        _gold[name] = np.load(os.path.join(GOLD, name + ".npz"))
    return _gold[name]


def blast_mesh(name, strict, extra=()):
    aa, lib = pkg(), pkg("lib")
    g = gold(name)
    par = aa.athinput.ParTable.from_file(orc.deck_for("blast", g)).cmdline([str(o) for o in g["overrides"]] + list(extra))
    run = aa.config.from_par(par, "blast")
    run.integrator = "vl" if name.startswith("smr_vl_") else "ctu"
    run.order = 3 if name.startswith("smr_ppm_") else 2
    return lib.Mesh(aa.config.levels(par, run), 0, strict)


def designed_mesh(tag, strict, nscal):
    """tests/test_gpu_hydro_branches.py run_mesh up to start(): the pattern of tests/hydromatrix.py uploaded on every level"""
    aa, lib = pkg(), pkg("lib")
    _, integrator, case, cour, dvac, pvac = hm.SMR_CFG[tag]
    deck = os.path.join(orc.DECKS, "athinput.blast")
    ov = hm.smr_overrides(case, cour)
    par = aa.athinput.ParTable.from_file(deck).cmdline(ov)
    run = aa.config.load(deck, ov, "blast", integrator)
    run.nscal = nscal
    m = lib.Mesh(aa.config.levels(par, run), 0, strict, initial=not nscal)
    try:
        for g in m.lev:
            c = g.cfg
            blk = g.new_host_block()
            hb.active(blk)[...] = hm.pattern(tuple(c.Nx), run.gamma, c.level, tuple(c.disp) if c.level else (0, 0, 0), dvac, pvac, nscal)[..., :5 + nscal]
            g.upload(blk)
    except Exception:
        m.close()
        raise
    return m


def state(m):
    return (m.time, m.dt, m.nstep), [g.download() for g in m.lev]


def same(a, b):
    return a[0] == b[0] and len(a[1]) == len(b[1]) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[1], b[1]))


def differs(a, b):
    return [int((~((x == y) | (np.isnan(x) & np.isnan(y)))).sum()) for x, y in zip(a[1], b[1])]


def syncs(m, reset=False):
    return sum(g.host_syncs(reset) for g in m.lev)


def relerr(a, b):
    out = []
    for c in range(a.shape[-1]):
        scale = np.nanmax(np.abs(b[..., c]))
        out.append(0.0 if scale == 0 else float(np.nanmax(np.abs(a[..., c] - b[..., c])) / scale))
    return out


_traj = {}


def trajectory(make, key, nsteps):
    """the per-step path: [(time, dt, nstep), whole block of every level] after 0 .. nsteps calls of Mesh.step(); run once per key
    (the knobs in force belong to the key) and shared, never written to"""
    if key not in _traj or len(_traj[key]) <= nsteps:
        m = make()
        try:
            m.start()
            out = [state(m)]
            for _ in range(max(nsteps, 1)):
                m.step()
                out.append(state(m))
        finally:
            m.close()
        for _, Us in out:
            for U in Us:
                U.setflags(write=False)
        _traj[key] = out
    return _traj[key]


# ---- 1. + 2. the fixtures: the reference's state and the per-step path, both builds ------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", BLAST)
def test_run_3d_reproduces_the_reference_and_the_per_step_path(name, strict, monkeypatch):
    """K = 2 and ONE call to the fixture's step count: the 6- and 8-step fixtures are full batches, the 5-step ones (the tree with
    four Grids, third-order reconstruction) leave one queued step behind the stop."""
    monkeypatch.setenv("AA_3D_BATCH", "2")
    g = gold(name)
    n = int(g["nstep"])
    m = blast_mesh(name, strict)
    try:
        assert m.can_run_3d() and m.run_3d_batch() == 2 and not any(lev.can_run_3d() for lev in m.lev)
        m.start()
        dt0 = m.dt
        assert m.run_3d(FAR, nstep_stop=n) == n
        s = state(m)
        assert [(lev.time, lev.dt, lev.nstep) for lev in m.lev] == [s[0]] * len(m.lev)      # every level's copy of MeshS
    finally:
        m.close()
    err = [relerr(U[NG:-NG, NG:-NG, NG:-NG, :5], g[f"U{l}"][..., :5]) for l, U in enumerate(s[1])]
    e_dt0, e_dt, e_t = abs(dt0 / float(g["dt0"]) - 1), abs(s[0][1] / float(g["dt"]) - 1), abs(s[0][0] / float(g["time"]) - 1)
    print(f"{name} {'strict' if strict else 'default'}: max error / field maximum per level {[max(e) for e in err]}, "
          f"dt0 {e_dt0:.2e} dt {e_dt:.2e} time {e_t:.2e}; state {s[0]!r}")
    assert s[0][2] == n and len(s[1]) == int(g["nlevels"])
    if strict:
        assert dt0 == float(g["dt0"]) and s[0][0] == float(g["time"]) and s[0][1] == float(g["dt"])
        for l, U in enumerate(s[1]):
            assert np.array_equal(U[NG:-NG, NG:-NG, NG:-NG, :5], g[f"U{l}"][..., :5]), f"level {l}: {err[l]}"
    else:
        # the bars of tests/test_gpu_smr.py test_blast_three_levels_vs_reference for these fixtures
        assert e_dt0 < 1e-13
        for l in range(len(err)):
            assert max(err[l]) < (1e-10 if "tree" in name else 1e-11), f"level {l}: {err[l]}"
    per_step = trajectory(lambda: blast_mesh(name, strict), (name, strict, "K2"), n)[n]
    assert s[0] == per_step[0], (s[0], per_step[0])
    assert same(s, per_step), f"zones that differ from step() per level: {differs(s, per_step)}"


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("tag,nscal", DESIGNED, ids=["five_variables", "passive_scalar"])
def test_run_3d_on_the_designed_state(tag, nscal, strict, monkeypatch):
    """the two-level case of tests/test_gpu_hydro_branches.py (HLLE, upwind and Roe faces on every kept plane; with a passive scalar
    the NS = 1 instances): three steps at K = 2, one queued step behind the stop"""
    monkeypatch.setenv("AA_3D_BATCH", "2")
    fx = hb.fixture(hm.smr_fixture_name(tag, nscal))
    m = designed_mesh(tag, strict, nscal)
    try:
        assert m.can_run_3d() and m.run_3d_batch() == 2
        m.start()
        dt0 = m.dt
        assert m.run_3d(FAR, nstep_stop=hm.NSTEP) == hm.NSTEP
        s = state(m)
    finally:
        m.close()
    errs = [hb.errors(hb.active(U), fx[f"U_{l}"]) for l, U in enumerate(s[1])]
    label = f"run_3d nested {tag} nscal={nscal}"
    print(f"{label} {'strict' if strict else 'default'}: max error per level {[float(e.max()) for e in errs]}, dt0 {dt0!r} state {s[0]!r}")
    if strict:
        assert dt0 == float(fx["dt0"]) and s[0][0] == float(fx["time"]) and s[0][1] == float(fx["dt"])
        for l, U in enumerate(s[1]):
            assert np.array_equal(hb.active(U), fx[f"U_{l}"]), (label, l)
    else:
        assert abs(dt0 / float(fx["dt0"]) - 1) < 1e-12
        hb.hold_default(label, errs, *twins.hydro_matrix("ctu", None, nscal))
    per_step = trajectory(lambda: designed_mesh(tag, strict, nscal), ("designed", tag, nscal, strict), hm.NSTEP)[hm.NSTEP]
    assert s[0] == per_step[0], (s[0], per_step[0])
    assert same(s, per_step), f"zones that differ from step() per level: {differs(s, per_step)}"


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("fu_kc", ["1", "3"])
def test_kept_x3_faces_at_chunk_boundaries(fu_kc, strict, monkeypatch):
    """k_flux2_update_keep_dc at 1 and 3 planes per block behind k_correct_all at 3 (odd: chunks also start on odd planes): every
    chunk boundary has a kept x3 face with ONE writer.  Against step() with the same chunks, whole blocks, and in the strict
    library against the reference."""
    monkeypatch.setenv("AA_3D_BATCH", "2")
    monkeypatch.setenv("AA_CA_KC", "3")
    monkeypatch.setenv("AA_FU_KC", fu_kc)
    name = "smr_blast_3lev_s6"
    g = gold(name)
    n = int(g["nstep"])
    m = blast_mesh(name, strict)
    try:
        assert m.run_3d_batch() == 2
        m.start()
        assert m.run_3d(FAR, nstep_stop=n) == n
        s = state(m)
    finally:
        m.close()
    per_step = trajectory(lambda: blast_mesh(name, strict), (name, strict, "kc3", fu_kc), n)[n]
    assert s[0] == per_step[0], (s[0], per_step[0])
    assert same(s, per_step), f"zones that differ from step() per level: {differs(s, per_step)}"
    if strict:
        assert s[0][0] == float(g["time"]) and s[0][1] == float(g["dt"])
        for l, U in enumerate(s[1]):
            assert np.array_equal(U[NG:-NG, NG:-NG, NG:-NG, :5], g[f"U{l}"][..., :5]), f"level {l}"


# ---- 3. the stop rules against the per-step path, four steps queued per read-back ---------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", STOP)
def test_stop_rules_leave_the_per_step_paths_state(name, strict, monkeypatch):
    """nstep_stop one below, on and one above a batch of 4 and inside the third; a t_stop inside the second batch.  Behind every
    call that stopped inside a batch two step() calls must land on the per-step path: a prolongation snapshot retaken, a kept flux
    plane or a ghost zone rewritten behind the stop would show there."""
    monkeypatch.setenv("AA_3D_BATCH", "4")
    tr = trajectory(lambda: blast_mesh(name, strict), (name, strict, "K4"), NTRAJ)
    for k in (3, 4, 5, 9):
        m = blast_mesh(name, strict)
        try:
            assert m.run_3d_batch() == 4
            m.start()
            assert m.run_3d(FAR, nstep_stop=k) == k
            s = state(m)
            print(f"{name} strict={strict} nstep_stop={k}: {s[0]!r} / {tr[k][0]!r}")
            assert same(s, tr[k]), (k, s[0], tr[k][0], differs(s, tr[k]))
            syncs(m, True)
            assert m.run_3d(FAR, nstep_stop=k) == 0 and syncs(m) == 0      # at the stop: no launch, no read-back
            m.step(); m.step()
            s2 = state(m)
            assert same(s2, tr[k + 2]), (k, "two steps later", s2[0], tr[k + 2][0], differs(s2, tr[k + 2]))
        finally:
            m.close()
    (t5, dt5, _), _ = tr[5]
    m = blast_mesh(name, strict)
    try:
        m.start()
        assert m.run_3d(t5 + 0.5 * dt5) == 6              # time >= t_stop first holds after the sixth step
        assert same(state(m), tr[6])
        assert m.run_3d(m.time) == 0 and m.run_3d(0.0) == 0 and same(state(m), tr[6])
        m.step(); m.step()
        assert same(state(m), tr[8])
        assert m.run_3d(FAR, nstep_stop=11) == 3          # ... and the device clock takes the host's dt over again
        assert same(state(m), tr[11])
    finally:
        m.close()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_the_last_dt_is_clipped_at_tlim(strict, monkeypatch):
    monkeypatch.setenv("AA_3D_BATCH", "4")
    name = STOP[0]
    (t6, dt6, _), _ = trajectory(lambda: blast_mesh(name, strict), (name, strict, "K4"), NTRAJ)[6]
    tlim = t6 + 0.5 * dt6
    extra = [f"time/tlim={tlim!r}"]
    h = blast_mesh(name, strict, extra)
    try:
        h.start()
        dts = []
        while h.time < tlim:
            dts.append(h.dt)
            h.step()
        per_step = state(h)
    finally:
        h.close()
    assert len(dts) == 7 and dts[6] == tlim - t6 < dt6 and per_step[0][0] == tlim
    m = blast_mesh(name, strict, extra)
    try:
        m.start()
        assert m.lev[0].cfg.run.tlim == tlim
        assert m.run_3d(tlim) == 7
        s = state(m)
        print(f"{name} strict={strict}: {s[0]!r} / {per_step[0]!r}")
        assert same(s, per_step), differs(s, per_step)
    finally:
        m.close()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_a_call_reads_back_once_per_batch(strict, monkeypatch):
    name = STOP[0]
    out = {}
    for k in ("4", "0"):
        monkeypatch.setenv("AA_3D_BATCH", k)
        m = blast_mesh(name, strict)
        try:
            assert m.run_3d_batch() == int(k) and m.can_run_3d() == (k != "0")
            m.start()
            syncs(m, True)
            assert m.run_3d(FAR, nstep_stop=12) == 12
            out[k] = (syncs(m), m.lev[0].host_syncs(), state(m))
        finally:
            m.close()
    m = blast_mesh(name, strict)
    try:
        m.start()
        syncs(m, True)
        for _ in range(12):
            m.step()
        stepping = syncs(m)
    finally:
        m.close()
    print(f"strict={strict}: host_syncs of 12 steps: {out['4'][0]} with AA_3D_BATCH=4, {out['0'][0]} with AA_3D_BATCH=0, {stepping} by step()")
    assert out["4"][0] == out["4"][1] == 3                 # one per batch, counted on the root
    assert out["4"][0] < stepping and out["0"][0] == stepping
    assert same(out["4"][2], out["0"][2])
    monkeypatch.setenv("AA_3D_BATCH", "4")
    assert same(out["0"][2], trajectory(lambda: blast_mesh(name, strict), (name, strict, "K4"), NTRAJ)[12])
    monkeypatch.setenv("AA_3D_BATCH", "-1")
    with pytest.raises(pkg("lib").AthenaError, match="AA_3D_BATCH=-1: must be 0 \\(step by step\\) or 1..1024"):
        blast_mesh(name, strict)


# ---- 4. stepwise inside the call, and refused --------------------------------------------------------------------------------------
STEPWISE = [("van_leer", "smr_vl_blast_2lev_s5", {}), ("tile_kernels", "smr_blast_3lev_s6", {"AA_CORRECT_ALL": None}),
            ("batch_0", "smr_blast_3lev_s6", {"AA_3D_BATCH": "0"})]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("why,name,knobs", STEPWISE, ids=[c[0] for c in STEPWISE])
def test_a_level_off_the_queued_chain_steps_inside_the_call(why, name, knobs, strict, monkeypatch):
    """the van Leer integrator, a level on the tile kernels (AA_CORRECT_ALL left to the size switch) and AA_3D_BATCH=0: batch 0,
    can_run_3d False, and run_3d takes the steps one at a time to the per-step bits -- a read-back per level and step"""
    monkeypatch.setenv("AA_3D_BATCH", "4")
    for k, v in knobs.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    g = gold(name)
    n = int(g["nstep"])
    m = blast_mesh(name, strict)
    try:
        assert m.run_3d_batch() == 0 and not m.can_run_3d()
        m.start()
        syncs(m, True)
        assert m.run_3d(FAR, nstep_stop=n) == n
        assert syncs(m) >= n * len(m.lev)
        s = state(m)
    finally:
        m.close()
    h = blast_mesh(name, strict)
    try:
        h.start()
        for _ in range(n):
            h.step()
        per_step = state(h)
    finally:
        h.close()
    assert same(s, per_step), (why, s[0], per_step[0], differs(s, per_step))
    if strict:
        assert s[0][0] == float(g["time"]) and s[0][1] == float(g["dt"])


def test_refusals_set_the_last_error(monkeypatch):
    import ctypes as C
    import twodfix
    monkeypatch.setenv("AA_3D_BATCH", "4")
    aa, cfg, lib = pkg(), pkg("config"), pkg("lib")
    L = lib.load(True)
    n = C.c_int()

    def refused(rc, *words):
        msg = L.aa_last_error().decode()
        assert rc != 0 and msg.startswith("[aa_mesh_run_3d]") and all(w in msg for w in words), (rc, msg)
    refused(L.aa_mesh_run_3d(None, 1.0, 1.0, 1, C.byref(n)), "null")
    assert L.aa_mesh_run_3d_batch(None) == 0
    # a Mesh of 2-D Grids: named to aa_mesh_run_2d
    fx = twodfix.fixture("g2dsmr_A_ctu_s8")
    deck = os.path.join(twodfix.DECKS, "athinput.blast2d_smr")
    ov = [str(o) for o in fx["overrides"]]
    m2 = lib.Mesh(cfg.levels_2d(aa.athinput.ParTable.from_file(deck).cmdline(ov), cfg.load(deck, ov, "blast", "ctu")), 0, True)
    try:
        assert not m2.can_run_3d() and m2.run_3d_batch() == 0
        refused(L.aa_mesh_run_3d(m2._h, 1.0, m2.lev[0].cfg.run.tlim, 1, C.byref(n)), "2-D", "aa_mesh_run_2d")
        with pytest.raises(lib.AthenaError, match="aa_mesh_run_2d"):
            m2.run_3d(1.0)
    finally:
        m2.close()
    name = "smr_blast_3lev_s6"
    m = blast_mesh(name, True)
    try:
        m.start()
        before = state(m)
        tlim = m.lev[0].cfg.run.tlim
        with pytest.raises(lib.AthenaError, match="tlim"):
            m.run_3d(tlim, tlim=2.0 * tlim)
        with pytest.raises(lib.AthenaError, match="2\\^20"):
            m.run_3d(tlim, nstep_stop=(1 << 20) + 1)
        assert same(state(m), before)                      # a refused call touches nothing
        for lev in m.lev:                                  # aa_run_3d on a level keeps refusing, aa_mesh_run_2d a 3-D Mesh
            assert L.aa_run_3d(lev._h, 1.0, tlim, 1, C.byref(n)) != 0 and "Mesh" in L.aa_last_error().decode()
        assert L.aa_mesh_run_2d(m._h, 1.0, tlim, 1, C.byref(n)) != 0 and "3-D" in L.aa_last_error().decode()
        # a pinned zone on level 1: refused with the state untouched, and step() still takes it
        g = m.lev[1]
        idx = ((NG + 2) * g.N[1] + NG + 3) * g.N[0] + NG + 1
        pin = np.array([[1.0, 0.0, 0.0, 0.0, 2.5]])
        g.set_pinned_cells(np.array([idx]), pin)
        assert not m.can_run_3d()
        refused(L.aa_mesh_run_3d(m._h, tlim, tlim, 3, C.byref(n)), "pinned", "grid 1")
        with pytest.raises(lib.AthenaError, match="pinned"):
            m.run_3d(tlim, nstep_stop=3)
        assert m.nstep == 0 and same(state(m), before)
        m.step()
        assert m.nstep == 1 and np.array_equal(g.download()[NG + 2, NG + 3, NG + 1], pin[0])
    finally:
        m.close()


# ---- 5. MeshRun.main with <outputN> blocks --------------------------------------------------------------------------------------------
def _tree(d):
    return sorted(os.path.relpath(os.path.join(dp, f), d) for dp, _, fs in os.walk(d) for f in fs)


def _meshrun(batch, out, strict, monkeypatch):
    D, O, cfg, lib = pkg("driver"), pkg("outputs"), pkg("config"), pkg("lib")
    monkeypatch.setenv("AA_3D_BATCH", batch)
    blocks = {"1": {"out_fmt": "hst", "dt": "0.004"}, "2": {"out_fmt": "vtk", "out": "prim", "dt": "0.008"}, "3": {"out_fmt": "rst", "dt": "0.012"}}
    ov = [str(o) for o in gold("smr_ppm_blast_2lev_s5")["overrides"]] + ["time/nlim=14", "time/cour_no=0.2"]
    par = meshfix.deck_par("blast", ov, blocks)
    run = cfg.from_par(par, "blast")
    m = D.MeshRun(lib.Mesh(cfg.levels(par, run), 0, strict), run)
    try:
        assert m.may_batch() == (batch != "0")
        calls = []
        adv = m.advance
        monkeypatch.setattr(m, "advance", lambda *a: (calls.append(adv(*a)), calls[-1])[1])
        syncs(m.mesh, True)
        m.main(O.OutputSet.from_par(par, 0.0, out))
        return dict(syncs=syncs(m.mesh), nstep=m.nstep, calls=calls, state=state(m.mesh))
    finally:
        m.mesh.close()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_meshrun_main_batches_and_writes_the_same_files(strict, tmp_path, monkeypatch):
    """a two-level blast with hst + vtk + rst blocks at cour_no 0.2 (a stretch between two output times is several steps): every
    file byte for byte the same with AA_3D_BATCH=4 and =0, with fewer read-backs"""
    res = {k: _meshrun(k, str(tmp_path / k), strict, monkeypatch) for k in ("4", "0")}
    paths = _tree(str(tmp_path / "0"))
    for k, r in res.items():
        print(f"AA_3D_BATCH={k}: {r['nstep']} steps, host_syncs {r['syncs']}, advance() -> {r['calls']}")
    assert {p.rsplit(".", 1)[1] for p in paths} == {"hst", "vtk", "rst"} and len(paths) > 6
    assert _tree(str(tmp_path / "4")) == paths
    for rel in paths:
        assert open(os.path.join(tmp_path / "4", rel), "rb").read() == open(os.path.join(tmp_path / "0", rel), "rb").read(), rel
    assert res["0"]["calls"] == [] and res["0"]["nstep"] == res["4"]["nstep"] == 14
    assert same(res["4"]["state"], res["0"]["state"])
    assert sum(res["4"]["calls"]) > len(res["4"]["calls"]) > 0 and all(c > 0 for c in res["4"]["calls"])
    assert res["4"]["syncs"] < res["0"]["syncs"]
