"""The CPU oracle against the golden vectors produced by the REAL reference
(tests/golden/make_golden.py).  Pins the oracle: every comparison is bit-for-bit."""
import glob
import os

import numpy as np
import pytest

import hydromatrix
import ionmatrix
import orc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("nscal", [0, 1])
def test_kernels_bitwise(nscal):
    g = np.load(os.path.join(GOLD, f"kernels_nscal{nscal}.npz"))
    gam = float(g["gamma"])
    assert _same(orc.cons_to_prim(g["Ul"], gam, nscal), g["W"])
    assert _same(orc.cfast(g["Ul"], gam, nscal), g["cfast"])
    assert _same(orc.fluxes(g["Ul"], g["Ur"], g["eta"], gam, nscal), g["F"])
    Wl, Wr = orc.lr_states(g["Wp"], float(g["dt"]), float(g["dx"]), int(g["il"]), int(g["iu"]), gam, nscal)
    assert _same(Wl, g["Wl"]) and _same(Wr, g["Wr"])


@pytest.mark.parametrize("nscal", [0, 1])
def test_ppm_reconstruction_bitwise(nscal):
    """lr_states_ppm.c (--with-order=3) on the 2048-cell pencils, incl. the scalar column whose work
    arrays overlap in the reference (see the oracle's comment)."""
    g = np.load(os.path.join(GOLD, f"kernels_ppm_nscal{nscal}.npz"))
    Wl, Wr = orc.lr_states(g["Wp"], float(g["dt"]), float(g["dx"]), int(g["il"]), int(g["iu"]), float(g["gamma"]), nscal, order=3)
    assert _same(Wl, g["Wl"]) and _same(Wr, g["Wr"])


def test_kernel_vectors_cover_all_roe_branches():
    """The Riemann vectors must exercise the HLLE fallback and the supersonic returns."""
    import ctypes as C
    L = orc.lib()
    h = C.c_long.in_dll(L, "orc_dbg_hlle"); s = C.c_long.in_dll(L, "orc_dbg_supersonic")
    g = np.load(os.path.join(GOLD, "kernels_nscal1.npz"))
    h.value = 0; s.value = 0
    orc.fluxes(g["Ul"], g["Ur"], g["eta"], float(g["gamma"]), 1)
    assert h.value > 100 and s.value > 100


def _rayplane(name, g):
    """Rays along +x1 / +x2 from our own problem file (tests/fixtures/rayplane_dir.c) run by the reference:
    get_ph_rate_plane cases -1 and -2 (ionradplane_3d.c:254-354), bvals_ionrad's lit face."""
    s = orc.make_rayplane_sim(g["nx"], -int(name.split("_dir")[1][0]))
    assert _same(s.active, g["U0"]), "initial condition"
    s.start()
    assert s.dt == float(g["dt0"])
    niter = [s.step() for _ in range(int(g["nstep"]))]
    assert niter == [int(x) for x in g["niter"]], "radiation sub-cycle counts"
    assert s.time == float(g["time"]) and s.dt == float(g["dt"])
    assert _same(s.active, g["U"])
    assert _same(s.edgeflux, g["edgeflux"])


def _coolpat(name, g):
    """Optically thin cooling (integrate_3d_ctu.c Steps 1c-3c, 8b, 11c; CoolingFunc = KoyInut, microphysics/cool.c:48) from our own
    problem file (tests/fixtures/cool_pattern.c) run by the reference, with and without the cooling function enrolled."""
    s = orc.make_coolpat_sim(g)
    assert _same(s.active[..., :5], g["U0"][..., :5]), "initial condition"
    s.start()
    assert s.dt == float(g["dt0"])
    for _ in range(int(g["nstep"])): s.step()
    assert s.time == float(g["time"]) and s.dt == float(g["dt"])
    assert _same(s.active[..., :5], g["U"][..., :5])


def test_cooling_fixtures_differ_from_the_run_without():
    a = np.load(os.path.join(GOLD, "coolpat_c1_16x12x10_n4.npz")); b = np.load(os.path.join(GOLD, "coolpat_c0_16x12x10_n4.npz"))
    assert _same(a["U0"], b["U0"]) and float(a["time"]) != float(b["time"])
    assert np.abs(a["U"][..., 4] / b["U"][..., 4] - 1).max() > 1e-2          # the cooling terms move the energy by per cent


def _ionmatrix(name, g):
    """The designed ion state (tests/ionmatrix.py) from our own problem file (tests/fixtures/ion_matrix.c) run by the reference:
    every branch of the sub-cycle's per-zone chemistry (ionrad_3d.c:70-590), with the temperature ceiling and without."""
    kv = dict(str(o).split("=") for o in g["overrides"])
    s = ionmatrix.make_sim(tuple(int(n) for n in g["nx"]), kv.get("ionradiation/tceil"))
    assert _same(s.active, g["U0"]), "initial condition"
    s.start()
    assert s.dt == float(g["dt0"])
    niter = [s.step() for _ in range(int(g["nstep"]))]
    assert niter == [int(x) for x in g["niter"]], "radiation sub-cycle counts"
    assert s.time == float(g["time"]) and s.dt == float(g["dt"])
    assert _same(s.active, g["U"])
    assert _same(s.edgeflux, g["edgeflux"])


def test_ion_matrix_fixtures_differ_where_the_ceiling_acts():
    a = np.load(os.path.join(GOLD, "ionmatrix_64x7x6_n1.npz")); b = np.load(os.path.join(GOLD, "ionmatrix_tceil0_64x7x6_n1.npz"))
    assert _same(a["U0"], b["U0"])
    hot = ionmatrix.indices()[0] == 8                    # the 3e6 K zones
    assert hot.sum() >= 32 and (a["U"][..., 4] != b["U"][..., 4])[hot].all()


def test_ion_matrix_covers_every_branch():
    """The census of the designed state, from the oracle's own arrays (orc_ion_zone_rates): the first rates pass puts at least 32
    zones into every class of compute_chem_rates / compute_therm_rates, every class stays populated over the 12 sub-cycles the GPU
    tests follow, and the entry takes every branch of the two floors in at least 32 zones.  Conditions, not measurements: a pattern
    that misses one has to change."""
    s = ionmatrix.make_sim()
    run = s.grid.run
    entry = ionmatrix.entry_census(s.active.copy(), run)
    print("entry:", entry)
    assert all(v >= 32 for v in entry.values()), entry
    assert entry["T<tfloor"] == ionmatrix.floored_by_design()
    s.bvals(); s.bvals_ionrad(); s.new_dt()
    s.ion_begin()
    seen = dict.fromkeys(ionmatrix.CLASSES, 0)
    for n in range(ionmatrix.NSUB):
        dt_chem, dt_therm = s.ion_rates()
        c = ionmatrix.census(s)
        if n == 0:
            print("first rates pass:", c)
            assert all(c[k] >= 32 for k in ionmatrix.CLASSES), c
        assert all(c[k] > 0 for k in ionmatrix.CLASSES), (n, c)
        for k in ionmatrix.CLASSES:
            seen[k] += c[k]
        s.ion_update(ionmatrix.subcycle_dt(dt_chem, dt_therm))
    print(f"zone-sub-cycles over {ionmatrix.NSUB} sub-cycles:", seen)


def test_ifront_with_20_rays_leaves_by_dt_hydro():
    """ifront 16x5x4: 20 rays = MAXCELLCOUNT, so check_range never stops the sub-cycles (ionrad_3d.c:985): the one step of the golden
    run takes its 109 sub-cycles and leaves by dt_hydro < dt_done (:1003) -- the data-dependent stop the one-kernel path learns of
    one sweep late -- and the sign-flip damping (:360-363, sign_count > MAXSIGNCOUNT) acts on the way."""
    g = np.load(os.path.join(GOLD, "ifront_16x5x4_n1.npz"))
    s = orc.make_sim("ifront", [f"domain1/Nx{d + 1}={int(g['nx'][d])}" for d in range(3)])
    s.start()
    limit = s.dt
    dt_done, niter, damped, exit_by = 0.0, 0, 0, None
    s.ion_begin()
    while exit_by is None:
        dt_chem, dt_therm = s.ion_rates()
        damped += int((s.ion_zone_rates()[4] > 4).sum())
        dt = min(dt_therm, dt_chem)
        done = dt_done + dt > limit
        if done:
            dt = limit - dt_done
        s.ion_update(dt)
        dt_done += dt; niter += 1
        count = s.ion_check_range_count()
        assert count <= 20
        if done:
            exit_by = "hydro_done"
        elif s.ion_dt_hydro() < dt_done:
            exit_by = "dt_hydro"
    print(f"ifront 16x5x4: {niter} sub-cycles, exit by {exit_by}, {count} zones out of range, {damped} damped zone-sub-cycles")
    assert exit_by == "dt_hydro" and niter == 109 == int(g["niter"][0])
    assert damped > 0


def _hydromatrix(name, g):
    """The designed hydro state (tests/hydromatrix.py) from our own problem file (tests/fixtures/hydro_matrix.c) run by the reference:
    every branch of the Roe solver, the reconstruction and the tracing.  3-D runs, one level or nested: the oracle reaches the
    reference's state bit for bit, and its live counters of the Roe solver's four exits equal, step by step, the execution counts
    gcov read from the reference's own run (cov_roe) -- the same faces are solved, the same branches taken.  2-D runs (the oracle
    has no 2-D path): the fixture starts from the pattern and stays finite with positive density.  A scalar fixture
    (hydromatrix_s1_*, put together with its base by hydromatrix.load) is reproduced over six columns, and its concentration s / d
    stays finite within the range the fixture records."""
    g = hydromatrix.load(name)
    nscal = int(g["nscal"]); nv = 5 + nscal
    if nscal:
        states = [g[k] for k in g if k == "U" or k.startswith("U_")]
        r = [U[..., 5] / U[..., 0] for U in states]
        assert all(np.isfinite(x).all() for x in r)
        assert [min(float(x.min()) for x in r), max(float(x.max()) for x in r)] == g["conc_range"].tolist()
    cnt = hydromatrix.counters()
    if "nlevels" in g:
        _, integrator, case, cour, dvac, pvac = hydromatrix.SMR_CFG[str(g["tag"])]
        assert (float(g["dvac"]), float(g["pvac"])) == (dvac, pvac)
        gam = hydromatrix.gamma(case[0][2])
        for l in range(int(g["nlevels"])):
            U0 = hydromatrix.pattern(tuple(g["nxs"][l]), gam, int(g["levels"][l]), tuple(g["disp"][l]), dvac, pvac, nscal)
            assert _same(U0[..., :nv], g[f"U0_{l}"]), f"initial condition, level {l}"
            assert np.isfinite(g[f"U_{l}"]).all() and (g[f"U_{l}"][..., 0] > 0).all() and (g[f"U0_{l}"][..., 0] > 0).all()
        if case[0][2] == 1:
            return
        m = hydromatrix.make_mesh(str(g["tag"]), nscal)
        m.start()
        assert m.dt == float(g["dt0"])
        for n in range(int(g["nstep"])):
            cnt[...] = 0
            m.step()
            assert cnt[:4].sum(axis=1).tolist() == g["cov_roe"][n].tolist(), f"exits of the Roe solver in step {n + 1}"
        assert m.time == float(g["time"]) and m.dt == float(g["dt"])
        for l, s in enumerate(m.lev):
            assert _same(s.active[..., :nv], g[f"U_{l}"]), f"level {l}"
        return
    cfg, nx = str(g["cfg"]), tuple(int(n) for n in g["nx"])
    dvac, pvac = hydromatrix.CFG[cfg][4:]
    assert (float(g["dvac"]), float(g["pvac"])) == (dvac, pvac)
    assert np.isfinite(g["U"]).all() and (g["U"][..., 0] > 0).all() and (g["U0"][..., 0] > 0).all()
    if nx[2] == 1:
        assert _same(hydromatrix.pattern(nx, hydromatrix.gamma(1), dvac=dvac, pvac=pvac)[..., :5], g["U0"]), "initial condition"
        return
    s = hydromatrix.make_sim(cfg, nx, nscal)
    assert _same(s.active[..., :nv], g["U0"]), "initial condition"
    s.start()
    assert s.dt == float(g["dt0"])
    for n in range(int(g["nstep"])):
        cnt[...] = 0
        s.step()
        assert cnt[:4].sum(axis=1).tolist() == g["cov_roe"][n].tolist(), f"exits of the Roe solver in step {n + 1}"
    assert s.time == float(g["time"]) and s.dt == float(g["dt"])
    assert _same(s.active[..., :nv], g["U"])


SMALL_GRID_MIN = 8
HYDROMATRIX = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "hydromatrix_*.npz")))


@pytest.mark.parametrize("name", HYDROMATRIX)
def test_hydro_matrix_covers_every_branch(name):
    """The census of the designed hydro state.  In every reference run every step reaches each class at least 32 times per sweep
    direction: conditions on the fixtures, not measurements -- a pattern that misses one has to change.
      3-D, one level   the oracle's counters (pinned to the reference bit for bit and, for the Roe solver's exits, count for count):
      and nested       the two supersonic returns, HLLE by u0 <= 0 and by p_inter < 0, the limiter giving zero / 2 lim1 / lim2, the
                       clamps acting, the four tracing branches (CTU), the parabola flattened and steepened (PPM), the pressure floor
                       where the configuration asks for it, and on the second-pass (H-corrected) faces etah winning the MAX for at
                       least one wave and losing it for at least one.  (A face on which etah wins NO wave cannot be had short of a
                       supersonic return: etah >= the face's own eta = |(vr + cr) - (vl - cl)| / 2, about the sound speed, so the
                       entropy wave |v| > etah means ev0 >= 0 or ev4 <= 0, roe.c:215-235.)
      2-D and nested   the reference's own execution counts of the Roe solver's exits, step by step (cov_roe; line counts tell neither
                       the sweep directions nor the limiter and tracing outcomes apart), and, per direction and class, the first-order
                       Riemann problems of the stored first state classified by the oracle's solver.  24x20 has a fifth of the faces
                       of 67x35 (960 against 4690) and two receding block edges of either strength per direction: there each HLLE class
                       is asked for SMALL_GRID_MIN = 8 times per direction (32 scaled by the faces is 6.6), the returns 32 times.
                       The 2-D van Leer fixtures hold >= 32 zones whose pressure is floored in the first state.
    At least 5 % of the zones of the first state lie in supersonic blocks.  Every side of every child Domain holds an HLLE face, and
    at least two sides of every child an upwind face (first-order Riemann problems of the root's last stored state across the outline).
      with a scalar    (hydromatrix_s1_*) also the Roe path's scalar flux taken from the left state (F[0] >= 0) and from the right,
                       per direction and step; and on the first state, per direction, at least 32 faces of each outcome of the Roe
                       solver (Roe flux, F = Fl, F = Fr, HLLE) ACROSS WHICH THE CONCENTRATION DIFFERS
                       -- a scalar flux taken from the wrong side shows only there."""
    g = hydromatrix.load(name)
    nscal = int(g["nscal"])
    nested = "nlevels" in g
    nx = tuple(int(n) for n in (g["nxs"][0] if nested else g["nx"]))
    gam = hydromatrix.gamma(nx[2])
    ndir = 2 if nx[2] == 1 else 3
    assert hydromatrix.supersonic_fraction(nx) >= 0.05
    cov = g["cov_roe"]
    print(name, "reference's exits of the Roe solver per step (Fl, Fr, HLLE u0, HLLE p):", cov.tolist())
    assert cov.shape == (hydromatrix.NSTEP, 4) and (cov >= hydromatrix.MIN_COUNT).all(), cov
    U0 = g["U0_0"] if nested else g["U0"]
    first = [np.bincount(hydromatrix.face_classes(U0, ax, gam).ravel(), minlength=5)[1:] for ax in range(ndir)]
    print(name, "first-order faces of the first state per direction (Fl, Fr, HLLE u0, HLLE p):", [f.tolist() for f in first])
    if nested or ndir == 2:
        hlle_min = SMALL_GRID_MIN if U0[..., 0].size < 1000 else hydromatrix.MIN_COUNT
        assert all((f[:2] >= hydromatrix.MIN_COUNT).all() and (f[2:] >= hlle_min).all() for f in first), first
    if nscal:
        across = [hydromatrix.scalar_faces(U0, ax, gam) for ax in range(ndir)]
        print(name, "first-order faces across which the concentration differs, per direction (Roe, Fl, Fr, HLLE):", [f.tolist() for f in across])
        assert all((f >= hydromatrix.MIN_COUNT).all() for f in across), across
    pvac = float(g["pvac"])
    floored = hydromatrix.floored_zones(U0, gam)
    print(name, "zones of the first state with a floored pressure:", floored)
    assert (floored >= hydromatrix.MIN_COUNT) == (pvac < 0), (floored, pvac)
    if nested:
        # the reference's own 1-ulp twins of the run (recorded by the golden script): the van Leer run is held on the GPU to the 3-D
        # van Leer twins, which flip no decision -- a bound that can only be borrowed for a run whose own twins flip none either
        print(name, f"the reference's 1-ulp twins part by {float(g['ref_twin_spread']):.3e}, {int(g['ref_twin_nflip'])} zones beyond 1e-9")
        if str(g["integrator"]) == "vl" and str(g["tag"]) not in hydromatrix.STRICT_ONLY:
            assert float(g["ref_twin_spread"]) < 1e-12 and int(g["ref_twin_nflip"]) == 0
        Ue = g["U_0"]
        for l in range(1, int(g["nlevels"])):
            sides_with_upwind = 0
            f = 2 ** int(g["levels"][l])
            lo = [int(g["disp"][l][d]) // f for d in range(3)]; hi = [lo[d] + int(g["nxs"][l][d]) // f for d in range(3)]
            for ax in range(ndir):
                cls = hydromatrix.face_classes(Ue, ax, gam)            # [k][j][i]: the face above zone i along ax
                box = [slice(lo[d], hi[d]) for d in range(3)]
                for side, at in (("lower", lo[ax] - 1), ("upper", hi[ax] - 1)):
                    sl = list(box); sl[ax] = slice(at, at + 1)
                    if ndir == 2:
                        sl[2] = slice(0, 1)
                    n = int((cls[sl[2], sl[1], sl[0]] >= 3).sum()); up = int(np.isin(cls[sl[2], sl[1], sl[0]], (1, 2)).sum())
                    print(name, f"Grid {l}, {side} x{ax + 1} side: {n} HLLE faces, {up} upwind faces")
                    assert n >= 1, (name, l, ax, side)
                    sides_with_upwind += up >= 1
            assert sides_with_upwind >= 2, (name, l, sides_with_upwind)
        if ndir == 3:           # the oracle runs the nested 3-D case: its full census, all levels together
            _, integrator, case, cour, dvac, pvac = hydromatrix.SMR_CFG[str(g["tag"])]
            cnt = hydromatrix.census_mesh(str(g["tag"]), nscal=nscal)
            table = {c: cnt[:, i, :].min(axis=0).tolist() for i, c in enumerate(hydromatrix.CLASSES)}
            print(name, "fewest per step, by direction:", table)
            for c in hydromatrix.required_for(integrator, 2, pvac, nscal):
                assert min(table[c]) >= hydromatrix.MIN_COUNT, (name, c, table[c])
        return
    if ndir == 2:
        return
    cfg = str(g["cfg"])
    cnt, _ = hydromatrix.census(cfg, nx, nscal=nscal)
    table = {c: cnt[:, i, :].min(axis=0).tolist() for i, c in enumerate(hydromatrix.CLASSES)}
    print(name, "fewest per step, by direction:", table)
    for c in hydromatrix.required(cfg, nscal):
        assert min(table[c]) >= hydromatrix.MIN_COUNT, (name, c, table[c])


RUNS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "*_n[0-9]*.npz")))


@pytest.mark.parametrize("name", RUNS)
def test_whole_run_bitwise(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    if name.startswith("rayplane"):
        return _rayplane(name, g)
    if name.startswith("coolpat"):
        return _coolpat(name, g)
    if name.startswith("ionmatrix"):
        return _ionmatrix(name, g)
    if name.startswith("hydromatrix"):
        return _hydromatrix(name, g)
    prob = name.rsplit("_", 2)[0]
    integrator = "ctu"
    order = 2
    if prob.startswith("vl_"):
        prob, integrator = prob[3:], "vl"
    if prob.startswith("noh_"):
        prob, integrator = prob[4:], "ctu-noh"             # CTU without --enable-h-correction
    if prob.startswith("ppm_"):
        prob, order = prob[4:], 3
    if prob.startswith("shkset1d"):
        prob = "shkset1d"                       # shkset1d_d<dir>_...
    nx = g["nx"]
    s = orc.make_sim(prob, [f"domain1/Nx{d + 1}={int(nx[d])}" for d in range(3)] + [str(o) for o in g["overrides"]],
                     integrator=integrator, order=order)
    nv = 5 + s.grid.run.nscal
    assert _same(s.active[..., :nv], g["U0"][..., :nv]), "initial condition"
    s.start()
    assert s.dt == float(g["dt0"])
    niter = [s.step() for _ in range(int(g["nstep"]))]
    if s.grid.run.ion:
        assert niter == [int(x) for x in g["niter"]], "radiation sub-cycle counts"
    assert s.time == float(g["time"]) and s.dt == float(g["dt"])
    assert _same(s.active[..., :nv], g["U"][..., :nv])
    if "edgeflux" in g.files:
        assert _same(s.edgeflux, g["edgeflux"])


DEV = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "dev_*.npz")))


@pytest.mark.parametrize("name", DEV)
def test_developed_state_pairs_bitwise(name):
    """Start from a reference state deep into the run (what a restart carries) and reach the
    reference's later state exactly."""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    prob = name[4:].rsplit("_", 3)[0]
    nx = g["nx"]
    over = [str(o) for o in g["overrides"]] if "overrides" in g.files else []      # e.g. the zoomed box of the one-sub-cycle pair
    s = orc.make_sim(prob, [f"domain1/Nx{d + 1}={int(nx[d])}" for d in range(3)] + over)
    nv = 5 + s.grid.run.nscal
    s.active[..., :nv] = g["UA"][..., :nv]
    s.time = float(g["timeA"]); s.dt = float(g["dtA"]); s.nstep = int(g["nstepA"])
    s.bvals(); s.bvals_ionrad()
    niter = [s.step() for _ in range(int(g["nstepB"]) - int(g["nstepA"]))]
    if s.grid.run.ion:
        assert niter == [int(x) for x in g["niter"]]
    assert s.time == float(g["timeB"]) and s.dt == float(g["dtB"])
    assert _same(s.active[..., :nv], g["UB"][..., :nv])
    if "edgefluxB" in g.files:
        assert _same(s.edgeflux, g["edgefluxB"])


def test_the_headline_regime_is_pinned():
    """The benchmark's timed region takes ONE radiation sub-cycle per step (ionrad_3d.c:919-1012 with the loop body
    executed once): one of the developed reference pairs must be in exactly that regime, NaN-free, over several steps."""
    g = np.load(os.path.join(GOLD, "dev_ioniz_sphere_36x36x36_s27_s33.npz"))
    assert [int(x) for x in g["niter"]] == [1] * 6
    assert np.isfinite(g["UA"]).all() and np.isfinite(g["UB"]).all()
    assert float(g["dtB"]) < 1.5 * float(g["dtA"])            # dt is no longer doubling: it sits at the CFL limit


SMR = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "smr_*.npz")))


@pytest.mark.parametrize("name", SMR)
def test_smr_runs_bitwise(name):
    """Static mesh refinement (smr.c RestrictCorrect / Prolongate, ionrad_smr.c, the SMR branches of
    main.c, new_dt.c and ionrad_3d.c): nested levels against runs of the reference built with
    STATIC_MESH_REFINEMENT, bit for bit on every level."""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    prob = "ioniz_sphere" if "ioniz_sphere" in name else "blast"
    m = orc.make_mesh(prob, orc.deck_for(prob, g), [str(o) for o in g["overrides"]], integrator="vl" if name.startswith("smr_vl_") else "ctu",
                      order=3 if name.startswith("smr_ppm_") else 2)
    assert len(m.lev) == int(g["nlevels"])
    nv = 5 + m.lev[0].grid.run.nscal
    m.start()
    assert m.dt == float(g["dt0"])
    niter = []
    for _ in range(int(g["nstep"])):
        niter += m.step()
    if m.lev[0].grid.run.ion:
        assert niter == [int(x) for x in g["niter"]], "radiation sub-cycle counts, level by level"
    assert m.time == float(g["time"]) and m.dt == float(g["dt"]) and m.nstep == int(g["nstep"])
    for l, s in enumerate(m.lev):
        assert _same(s.active[..., :nv], g[f"U{l}"][..., :nv]), f"level {l}"
        if f"edgeflux{l}" in g.files:
            assert _same(s.edgeflux, g[f"edgeflux{l}"]), f"EdgeFlux level {l}"
