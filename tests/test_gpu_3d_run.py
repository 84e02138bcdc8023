"""aa_run_3d / Grid.run_3d on an MI355X: many steps of a 3-D hydro Grid per host visit, the time step picked on the device
(csrc/hydro_kernels.hip k3d_seed / k3d_advance and the *_dc entry points of the default CTU chain; csrc/run.hip).

Two references.  The states the unmodified reference left (tests/golden/blast_*.npz, hydromatrix_*.npz): the strict library
reproduces them bit for bit, the default library within the bars the per-step tests of those fixtures use (blast: 1e-11 of each
field's maximum and 1e-12 in dt, test_gpu_parity.py; the designed state: the twins rule of test_gpu_hydro_branches.py).  And the
per-step path (Grid.step) of the same library with the same knobs: run_3d gives its bits in BOTH libraries -- the whole block, ghost
zones included, and (time, dt, nstep) -- because the queued kernels run the same code on the same operands; a step queued behind
the stop that stored anything would show there.

The queued chain is the one aa_integrate_3d_ctu launches by default on Grids of 4e5 zones or more (k_correct_all with both other
first passes on board, k_flux2_update); the tests force it on their small Grids with AA_CORRECT_ALL=1, as the per-step tests of
those kernels do.  Without the knob a small Grid takes the tile kernels and run_3d loops over aa_step ("by-size" below)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import hydromatrix as hm
import orc
import twins
from test_gpu_hydro_branches import active, errors, fixture, hold_default

pytestmark = pytest.mark.gpu
NG = 4
FAR = 1.0e300                       # a t_stop no run reaches: the step count ends the call
BIG = {"AA_CORRECT_ALL": "1"}
NTRAJ = 9


def pkg(sub=None):
    return importlib.import_module("atmospheric-athena_amd" + ("." + sub if sub else ""))


def set_knobs(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def nx_ov(nx):
    return [f"domain1/Nx{d + 1}={int(nx[d])}" for d in range(3)]


def blast(nx, strict, integrator="ctu", order=2, extra=()):
    aa, lib = pkg(), pkg("lib")
    run = aa.config.load(os.path.join(orc.DECKS, "athinput.blast"), nx_ov(nx) + list(extra), "blast", integrator)
    run.order = order
    g = lib.setup_problem(aa.config.slab(run), 0, strict)
    g.start()
    return g


def sphere(nx, strict):
    """The hydro side of the ioniz_sphere configuration -- a passive scalar and a static potential, the 6-variable gravity
    kernels -- without its radiation plane and its pinned core (run_3d takes neither).  The deck's own planet falls into its
    softened potential within a few steps once the core is no longer reset, so the state and the potential (tables at zone
    centres and lower faces, aa_set_static_grav_tables) are smooth patterns of the zone indices instead."""
    aa, lib = pkg(), pkg("lib")
    run = aa.config.load(os.path.join(orc.DECKS, "athinput.ioniz_sphere"), nx_ov(nx) + ["time/tlim=1e30"], "ioniz_sphere")
    run.ion = False
    g = lib.Grid(aa.config.slab(run), 0, strict)
    assert g.nvar == 6
    k, j, i = (a.astype(np.float64) for a in np.meshgrid(np.arange(g.N[2]), np.arange(g.N[1]), np.arange(g.N[0]), indexing="ij"))

    def phi(x, y, z):
        return np.ascontiguousarray(0.02 * (x + 0.5 * y - 0.25 * z) + 0.05 * np.sin(0.3 * x) * np.cos(0.2 * y + 0.1 * z))
    tabs = [phi(i, j, k), phi(i - 0.5, j, k), phi(i, j - 0.5, k), phi(i, j, k - 0.5)]
    g._chk(g.L.aa_set_static_grav_tables(g._h, *[lib._dp(t) for t in tabs]))
    d = 1.0 + 0.3 * np.sin(0.37 * i + 0.21 * j) * np.cos(0.29 * k)
    v = [0.2 * np.sin(0.2 * i + 0.3 * j + 0.4 * k), 0.15 * np.cos(0.25 * i - 0.2 * k), 0.1 * np.sin(0.3 * j + 0.15 * k)]
    p = 1.0 + 0.2 * np.cos(0.23 * i + 0.19 * j - 0.27 * k)
    U = g.new_host_block()
    U[..., 0] = d
    for a in range(3):
        U[..., 1 + a] = d * v[a]
    U[..., 4] = p / (run.gamma - 1.0) + 0.5 * d * (v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    U[..., 5] = d * (0.5 + 0.4 * np.cos(0.31 * i - 0.17 * k))
    g.upload(U)
    g.start()
    return g


def matrix(cfg, nx, strict, nscal=0):
    """the designed state of tests/hydromatrix.py, as test_gpu_hydro_branches.run_single sets it up"""
    aa, lib = pkg(), pkg("lib")
    _, integrator, order, cour, dvac, pvac = hm.CFG[cfg]
    run = aa.config.load(os.path.join(orc.DECKS, "athinput.blast"), hm.overrides(nx, cour), "blast", integrator)
    run.order = order
    run.nscal = nscal
    g = lib.Grid(aa.config.slab(run), 0, strict) if nscal else lib.setup_problem(aa.config.slab(run), 0, strict)
    assert g.nvar == 5 + nscal
    blk = g.new_host_block()
    active(blk)[...] = hm.pattern(nx, run.gamma, dvac=dvac, pvac=pvac, nscal=nscal)[..., :5 + nscal]
    g.upload(blk)
    g.start()
    return g


def state(g):
    return (g.time, g.dt, g.nstep), g.download()


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


def relerr(a, b):
    return [float(np.abs(a[..., c] - b[..., c]).max() / np.abs(b[..., c]).max()) if np.abs(b[..., c]).max() > 0
            else float(np.abs(a[..., c]).max()) for c in range(a.shape[-1])]


def per_step(make, n):
    """the per-step path: the state after 0 .. n calls of step()"""
    g = make()
    out = [state(g)]
    for _ in range(n):
        g.step()
        out.append(state(g))
    g.close()
    for _, U in out:
        U.setflags(write=False)
    return out


# ---- 1. the fixtures: the reference's states, and the per-step path's bits -------------------------------------------------------
FIXTURES = ["blast_16x16x16_n5", "blast_12x20x16_n4"] + [f"hydromatrix_{c}_{s}_n3" for c in ("ctu", "noh", "ppm") for s in ("24x20x16", "67x10x9")]
# with a passive scalar (the *_dc entries of the NS = 1 kernels without a potential): CTU on both Grids, no-H and PPM across the tile edge
# (measured on an MI355X: the strict build bit for bit over six columns, queued and by size; the default build 6.1e-16 ... 2.0e-15 of
#  each field's maximum with no zone beyond 1e-9, against twins of 4.7e-4 ... 8.7e-3)
FIXTURES += ["hydromatrix_s1_ctu_24x20x16_n3", "hydromatrix_s1_ctu_67x10x9_n3", "hydromatrix_s1_noh_67x10x9_n3", "hydromatrix_s1_ppm_67x10x9_n3"]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("chain", ["queued", "by-size"])
@pytest.mark.parametrize("name", FIXTURES)
def test_run_3d_reproduces_the_reference_and_the_per_step_path(name, chain, strict, monkeypatch):
    monkeypatch.setenv("AA_3D_BATCH", "2")      # (the fixtures are 3 .. 5 steps: two or three batches, one step behind the stop where n is odd)
    if chain == "queued":
        set_knobs(monkeypatch, BIG)
    fx = fixture(name)
    n = int(fx["nstep"])
    nx = tuple(int(x) for x in fx["nx"])
    cfg = str(fx["cfg"]) if "cfg" in fx else None
    nscal = int(fx["nscal"]) if cfg else 0
    make = (lambda: matrix(cfg, nx, strict, nscal)) if cfg else (lambda: blast(nx, strict))
    g = make()
    assert g.can_run_3d() and g.run_3d_batch() == (2 if chain == "queued" else 0)
    if cfg:
        assert fx["U"].shape[-1] == 5 + nscal
        assert np.array_equal(active(g.download())[..., :5 + nscal], fx["U0"]), "the uploaded pattern is the fixture's U0"
    dt0 = g.dt
    g.host_syncs(True)
    assert g.run_3d(FAR, nstep_stop=n) == n
    syncs = g.host_syncs()
    s = state(g)
    g.close()
    ref = per_step(make, n)[n]
    nv = fx["U"].shape[-1] if cfg else 5
    Ua = active(s[1])[..., :nv]
    err = errors(Ua, fx["U"][..., :nv])
    print(f"{name} {chain} strict={strict}: max error {float(err.max()):.3e} state {s[0]!r} per step {ref[0]!r} "
          f"fixture ({float(fx['time'])!r}, {float(fx['dt'])!r}) host_syncs {syncs}")
    assert s[0][2] == n
    if chain == "queued":
        assert syncs == -(-n // 2)
    if strict:
        assert dt0 == float(fx["dt0"])
        assert np.array_equal(Ua, fx["U"][..., :nv]), float(err.max())
        assert s[0][0] == float(fx["time"]) and s[0][1] == float(fx["dt"])
    elif cfg:
        w, nf, nz = twins.hydro_matrix(cfg, nx, nscal)
        hold_default(f"{name} {chain}", [err], w, nf / nz)
    else:
        assert float(err.max()) < 1e-11, err.max(axis=(0, 1, 2))
        assert abs(s[0][1] / float(fx["dt"]) - 1) < 1e-12
    assert s[0] == ref[0]
    assert np.array_equal(s[1], ref[1]), relerr(s[1], ref[1])


# ---- 2. the kernels' tiles and chunks against the per-step path -------------------------------------------------------------------
# two x1 tiles, rows no multiple of CA_TJ / FU_TJ - 1, several k-chunks of three planes; one long row of two tiles; three tiles with
# the last face k_correct_all needs (ie + 2) on a tile edge; CTU without H-correction (the eta memset); third order (the slope
# kernels in front); a passive scalar with a static potential (the 6-variable gravity instantiations, 256 registers)
KC3 = dict(BIG, AA_CA_KC="3", AA_FU_KC="3")
SHAPES = [("blast-70x23x37-kc3", lambda st: blast((70, 23, 37), st), KC3),
          # (radius 0.3: with the deck's 0.1 no zone centre of this Grid lies inside the blast and nothing moves)
          ("blast-128x8x4", lambda st: blast((128, 8, 4), st, extra=["problem/radius=0.3"]), BIG),
          ("blast-130x9x11", lambda st: blast((130, 9, 11), st), BIG),
          ("noh-70x23x37-kc3", lambda st: blast((70, 23, 37), st, "ctu-noh"), KC3),
          ("ppm-130x9x11", lambda st: blast((130, 9, 11), st, order=3), BIG),
          ("ppm-noh-70x23x37-kc3", lambda st: blast((70, 23, 37), st, "ctu-noh", 3), KC3),
          ("sphere-32x32x32", lambda st: sphere((32, 32, 32), st), BIG)]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("label,make,knobs", SHAPES, ids=[s[0] for s in SHAPES])
def test_queued_kernels_give_the_per_step_paths_bits(label, make, knobs, strict, monkeypatch):
    """five steps as a batch of four and one of one step with three behind the stop"""
    monkeypatch.setenv("AA_3D_BATCH", "4")
    set_knobs(monkeypatch, knobs)
    ref = per_step(lambda: make(strict), 5)
    g = make(strict)
    # (the strict build's k_correct_all with a scalar AND a potential needs scratch, in either entry; it has no entry on the device
    #  clock and run_3d steps that Grid one at a time -- to the same bits, which is what is held here)
    queued = not (strict and label.startswith("sphere"))
    assert g.can_run_3d() and g.run_3d_batch() == (4 if queued else 0)
    g.host_syncs(True)
    assert g.run_3d(FAR, nstep_stop=5) == 5
    assert g.host_syncs() == 2 if queued else g.host_syncs() >= 5
    s = state(g)
    g.close()
    print(f"{label} strict={strict}: {s[0]!r} / {ref[5][0]!r}")
    assert np.isfinite(s[1]).all() and not np.array_equal(ref[5][1], ref[0][1])
    assert s[0] == ref[5][0]
    assert np.array_equal(s[1], ref[5][1]), relerr(s[1], ref[5][1])


# ---- 3. the stop rules, four steps queued per read-back -------------------------------------------------------------------------------
_traj = {}


def trajectory(strict):
    if strict not in _traj:
        _traj[strict] = per_step(lambda: blast((24, 20, 16), strict), NTRAJ)
    return _traj[strict]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_stop_rules_leave_the_per_step_paths_state(strict, monkeypatch):
    """nstep_stop one below, on and one above a batch of 4 and inside the third; a t_stop inside the second batch; t_stop at the
    Grid's own time and at 0.  The whole block is compared, so a step queued behind the stop that stored anything would show."""
    monkeypatch.setenv("AA_3D_BATCH", "4")
    set_knobs(monkeypatch, BIG)
    tr = trajectory(strict)
    for n in (1, 3, 4, 5, 9):
        g = blast((24, 20, 16), strict)
        assert g.run_3d_batch() == 4
        g.host_syncs(True)
        assert g.run_3d(FAR, nstep_stop=n) == n
        assert g.host_syncs() == -(-n // 4)
        s = state(g)
        print(f"strict={strict} nstep_stop={n}: {s[0]!r} / {tr[n][0]!r}")
        assert same(s, tr[n]), (n, s[0], tr[n][0])
        # ... and called again at the stop it takes no step and touches nothing
        g.host_syncs(True)
        assert g.run_3d(FAR, nstep_stop=n) == 0 and g.host_syncs() == 0
        assert same(state(g), tr[n])
        g.close()
    (t5, dt5, _), _ = tr[5]
    g = blast((24, 20, 16), strict)
    assert g.run_3d(t5 + 0.5 * dt5) == 6              # time >= t_stop first holds after the sixth step
    assert same(state(g), tr[6])
    g.host_syncs(True)
    assert g.run_3d(g.time) == 0 and g.run_3d(0.0) == 0 and g.host_syncs() == 0 and same(state(g), tr[6])
    # ... and it mixes with single steps
    g.step()
    assert g.run_3d(FAR, nstep_stop=9) == 2 and same(state(g), tr[9])
    g.close()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_the_last_dt_is_clipped_at_tlim(strict, monkeypatch):
    monkeypatch.setenv("AA_3D_BATCH", "4")
    set_knobs(monkeypatch, BIG)
    (t6, dt6, _), _ = trajectory(strict)[6]
    tlim = t6 + 0.5 * dt6
    extra = [f"time/tlim={tlim!r}"]
    h = blast((24, 20, 16), strict, extra=extra)
    dts = []
    while h.time < tlim:
        dts.append(h.dt)
        h.step()
    ref = state(h)
    h.close()
    assert len(dts) == 7 and dts[6] == tlim - t6 < dt6 and ref[0][0] == tlim
    g = blast((24, 20, 16), strict, extra=extra)
    assert g.cfg.run.tlim == tlim
    assert g.run_3d(tlim) == 7
    s = state(g)
    print(f"strict={strict}: {s[0]!r} / {ref[0]!r}")
    assert same(s, ref)
    g.close()


# ---- 4. what steps one at a time inside the call, and what is refused ----------------------------------------------------------------
FALLBACKS = [("van-leer", lambda st: blast((24, 20, 16), st, "vl"), BIG),
             ("unfused-update", lambda st: blast((24, 20, 16), st), dict(BIG, AA_FUSED_UPDATE="0")),
             ("batch-0", lambda st: blast((24, 20, 16), st), dict(BIG, AA_3D_BATCH="0")),
             ("x3-unfused", lambda st: blast((24, 20, 16), st), dict(BIG, AA_X3_FUSED="0")),
             ("cfl-pass", lambda st: blast((24, 20, 16), st), dict(BIG, AA_CFL_FUSED="0")),
             ("edge-overlap", lambda st: blast((24, 20, 16), st), dict(BIG, AA_EDGE_OVERLAP="1")),
             ("tile-kernels", lambda st: blast((24, 20, 16), st), {"AA_CORRECT_ALL": "0"})]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("label,make,knobs", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_off_the_default_chain_run_3d_loops_over_step(label, make, knobs, strict, monkeypatch):
    set_knobs(monkeypatch, knobs)
    ref = per_step(lambda: make(strict), 3)
    g = make(strict)
    assert g.can_run_3d() and g.run_3d_batch() == 0
    g.host_syncs(True)
    assert g.run_3d(FAR, nstep_stop=3) == 3
    assert g.host_syncs() >= 3
    assert same(state(g), ref[3])
    g.close()


def test_the_knob_is_checked(monkeypatch):
    lib = pkg("lib")
    monkeypatch.setenv("AA_3D_BATCH", "1024")
    g = blast((8, 8, 8), True)
    g.close()
    for bad in ("-1", "1025"):
        monkeypatch.setenv("AA_3D_BATCH", bad)
        with pytest.raises(lib.AthenaError, match="AA_3D_BATCH=.*must be 0 \\(step by step\\) or 1..1024"):
            blast((8, 8, 8), True)


def test_refusals_set_the_last_error(monkeypatch):
    aa, lib, cfg = pkg(), pkg("lib"), pkg("config")
    set_knobs(monkeypatch, BIG)
    L = lib.load(True)
    n = C.c_int()

    def refused(rc, who, *words):
        msg = L.aa_last_error().decode()
        assert rc != 0 and msg.startswith(f"[{who}]") and all(w in msg for w in words), (rc, msg)
    run1 = cfg.load(os.path.join(orc.DECKS, "athinput.blast1d"), ["domain1/Nx1=8"], "blast")
    g1 = lib.Grid(cfg.slab(run1), 0, True)
    refused(L.aa_run_3d(g1._h, 1.0, run1.tlim, 1, C.byref(n)), "aa_run_3d", "1-D", "aa_run_1d")
    assert not g1.can_run_3d() and g1.run_3d_batch() == 0
    g1.close()
    run2 = cfg.load(os.path.join(orc.DECKS, "athinput.blast2d"), ["domain1/Nx1=8", "domain1/Nx2=8"], "blast")
    g2 = lib.Grid(cfg.slab(run2), 0, True)
    refused(L.aa_run_3d(g2._h, 1.0, run2.tlim, 1, C.byref(n)), "aa_run_3d", "2-D", "aa_run_2d")
    assert not g2.can_run_3d() and g2.run_3d_batch() == 0
    g2.close()
    g = blast((24, 20, 16), True)
    tlim = g.cfg.run.tlim
    assert g.can_run_3d() and not g.can_run_2d() and not g.can_run_until()
    refused(L.aa_run_2d(g._h, 1.0, tlim, 1, C.byref(n)), "aa_run_2d", "3-D")      # the 2-D call still refuses a 3-D Grid
    refused(L.aa_run_1d(g._h, 1.0, tlim, 1, C.byref(n)), "aa_run_1d", "3-D")
    with pytest.raises(lib.AthenaError, match="tlim"):
        g.run_3d(tlim, tlim=2.0 * tlim)
    with pytest.raises(lib.AthenaError, match="2\\^20"):
        g.run_3d(tlim, nstep_stop=(1 << 20) + 1)
    with pytest.raises(lib.AthenaError, match="2\\^20"):
        g.run_3d(tlim, nstep_stop=-1)
    before = state(g)
    m = ((NG + 3) * g.N[1] + NG + 2) * g.N[0] + NG + 1
    pin = np.array([[1.0, 0.0, 0.0, 0.0, 2.5]])
    g.set_pinned_cells(np.array([m]), pin)
    assert not g.can_run_3d()
    refused(L.aa_run_3d(g._h, tlim, tlim, 3, C.byref(n)), "aa_run_3d", "pinned")
    assert g.nstep == 0 and same(state(g), before)
    g.step()                                        # ... and the per-step path takes them
    assert g.nstep == 1 and np.array_equal(g.download()[NG + 3, NG + 2, NG + 1, :5], pin[0])
    g.close()
    # a Grid cut into slabs (both on this device)
    monkeypatch.setenv("AA_SLAB_DEVICES", "0,0")
    run3 = cfg.load(os.path.join(orc.DECKS, "athinput.blast"), nx_ov((24, 20, 16)), "blast")
    gs = lib.setup_problem(cfg.slab(run3), 0, True, nslab=2)
    try:
        gs.start()
        assert not gs.can_run_3d() and gs.run_3d_batch() == 0
        refused(L.aa_run_3d(gs._h, 1.0, run3.tlim, 1, C.byref(n)), "aa_run_3d", "slabs")
    finally:
        gs.close()
    # a level of a Mesh
    _, integrator, case, cour, _, _ = hm.SMR_CFG["3d_ctu"]
    ov = hm.smr_overrides(case, cour)
    deck = os.path.join(orc.DECKS, "athinput.blast")
    par = aa.athinput.ParTable.from_file(deck).cmdline(ov)
    runm = cfg.load(deck, ov, "blast", integrator)
    mesh = lib.Mesh(cfg.levels(par, runm), 0, True)
    try:
        for lev in mesh.lev:
            assert not lev.can_run_3d()
            refused(L.aa_run_3d(lev._h, 1.0, runm.tlim, 1, C.byref(n)), "aa_run_3d", "Mesh")
    finally:
        mesh.close()


# ---- 5. Driver.main on a short blast deck with two output times ------------------------------------------------------------------
def _tree(d):
    return sorted(os.path.relpath(os.path.join(dp, f), d) for dp, _, fs in os.walk(d) for f in fs)


OUTPUT_BLOCKS = """
<output1>
out_fmt = hst
dt      = 0.015

<output2>
out_fmt = vtk
out     = prim
dt      = 0.015

<output3>
out_fmt = rst
dt      = 0.03
"""


def _driver_run(batch, out, deck, monkeypatch):
    cfg = pkg("config"); D = pkg("driver"); O = pkg("outputs"); A = pkg("athinput")
    set_knobs(monkeypatch, BIG)
    if batch is None:
        monkeypatch.delenv("AA_3D_BATCH", raising=False)
    else:
        monkeypatch.setenv("AA_3D_BATCH", batch)
    ov = nx_ov((24, 20, 16)) + ["time/cour_no=0.4", "time/tlim=0.03", "problem/radius=0.3", "job/maxout=3"]
    par = A.ParTable.from_file(deck).cmdline(ov)
    d = D.Driver(cfg.from_par(par, "blast"), strict=True)
    assert d.may_batch() == (batch != "0")
    calls = []
    adv = d.advance
    monkeypatch.setattr(d, "advance", lambda *a: (calls.append(adv(*a)), calls[-1])[1])
    d.eng.host_syncs(True)
    d.main(O.OutputSet.from_par(par, 0.0, out))
    res = dict(syncs=d.eng.host_syncs(), nstep=d.nstep, trace=list(d.niter_trace), calls=calls, state=(d.time, d.dt, d.nstep), U=d.eng.download())
    d.eng.close()
    return res


def test_driver_main_batches_a_3d_run_and_writes_the_same_files(tmp_path, monkeypatch):
    """the shipped blast deck at 24 x 20 x 16 with an hst and a vtk block every 0.015 and an rst block, to tlim = 0.03"""
    deck = str(tmp_path / "athinput.blast_out")
    open(deck, "w").write(open(os.path.join(orc.DECKS, "athinput.blast")).read() + OUTPUT_BLOCKS)
    res = {m: _driver_run(b, str(tmp_path / m), deck, monkeypatch) for m, b in (("knob", "0"), ("default", None))}
    paths = _tree(str(tmp_path / "knob"))
    assert {p.rsplit(".", 1)[1] for p in paths} == {"hst", "vtk", "rst"} and sum(p.endswith(".vtk") for p in paths) >= 3
    for m, r in res.items():
        print(f"{m}: {r['nstep']} steps, host_syncs {r['syncs']}, advance() -> {r['calls']}")
        assert _tree(str(tmp_path / m)) == paths
        assert len(r["trace"]) == r["nstep"] and r["state"] == res["knob"]["state"] and np.array_equal(r["U"], res["knob"]["U"])
        for rel in paths:
            assert open(os.path.join(tmp_path / m, rel), "rb").read() == open(os.path.join(tmp_path / "knob", rel), "rb").read(), (m, rel)
    assert res["knob"]["calls"] == [] and res["knob"]["nstep"] >= 4 and res["knob"]["syncs"] >= res["knob"]["nstep"]
    assert 0 < sum(res["default"]["calls"]) <= res["default"]["nstep"] and len(res["default"]["calls"]) <= 3
    assert res["default"]["syncs"] < res["knob"]["syncs"]
