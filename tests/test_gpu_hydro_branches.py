"""Every branch of the hydro step inside the fused kernels, on an MI355X, against the reference.

The other whole-step tests run on gentle states: no bitwise fixture holds a supersonic return of the Roe solver, and only one
holds an HLLE fallback.  Here the state is the designed one of tests/hydromatrix.py (our own problem file
tests/fixtures/hydro_matrix.c run by the unmodified reference, tests/golden/hydromatrix_*.npz): thousands of upwind returns, HLLE
fallbacks by either test, every limiter and tracing branch in every sweep direction and step (the census is asserted on the CPU,
tests/test_oracle_golden.py::test_hydro_matrix_covers_every_branch), through every form of the kernel chain the other suites select
by environment knobs, on one level and on nested levels, in 3-D and in 2-D.

  strict build    bit for bit: U of every level, time, dt (and dt0 after start()).  For the 3-D nested case also every level's whole
                  block, ghost zones as Prolongate left them, against the oracle.
  default build   fused multiply-adds move Roe -> HLLE and upwind decisions, on this state by design.  The rule of
                  test_gpu_parity.py::test_from_developed_reference_state: the error (|a - b| over each field's maximum) is at most
                  twice the spread of the ORACLE's own 1-ulp twins of the same run (tests/twins.py: hydro_matrix, computed on the CPU
                  in this session), the zones beyond 1e-9 at most three times the twins'.  The CTU and PPM twins part by 1e-4 ...
                  1e-2 on this state (one flipped decision moves dt) while the contracted build flips almost nothing, so that
                  rule alone would hold those builds to very little: north_star's 1e-6 is asserted as a ceiling in EVERY case
                  (the largest measured is 9.6e-9).
                  The oracle has no 2-D path and its Mesh is not twinned: the 2-D and the nested runs are held to the 3-D twins'
                  figures of the same integrator (the larger spread of the two 3-D Grids, the zones as a share of the Grid).

Measured on an MI355X (default build; the strict build is bit for bit in all 90 cases): CTU, CTU without H-correction and PPM twins
spread by 2.7e-4 ... 1.0e-2 with nearly every zone beyond 1e-9 (one flipped decision moves dt), the GPU differs by 5e-16 ... 2e-15
with no zone beyond 1e-9, but for the 3-D nested case on the big-grid kernels (9.6e-9, 6 zones).  The van Leer twins spread by
1.9e-15 ... 2.7e-15 and flip nothing; the GPU differs by 0.9e-15 ... 1.8e-15 on one level in 3-D and 2-D.
The nested van Leer case has a positive pressure in its near-vacuum blocks (1.3e-15, no zone).  With E below the kinetic
energy there, as in the single-level van Leer runs, the REFERENCE's own 1-ulp twins of the nested run part by 3.8e-9 in two zones at
the first child's side (a decision on the rounding noise of a floored pressure; tests/hydromatrix.py SMR_CFG): that run
("2d_vl_floor") is held in the strict build only, which has to follow the reference decision for decision.

With a passive scalar (the NS = 1 instantiations of every hydro kernel, without a potential; the scalar fixtures hydromatrix_s1_*,
sections 4 and 5 below): the same chains on six variables, the concentration another one across every face.  The rules are the
same ones over six columns: the strict build bit for bit, the default build against the oracle's twins of the six-variable run.
Measured on an MI355X (the strict build is bit for bit in all 29 cases, six columns, time, dt and dt0): the twins of the six-variable
CTU, no-H and PPM runs spread by 4.7e-4 ... 1.0e-2 with nearly every zone beyond 1e-9, those of the van Leer runs by 1.9e-15 ...
2.7e-15 with none.  The default build differs by 6.5e-16 ... 2.0e-15 under CTU (with and without H-correction, every chain),
6.1e-16 ... 6.7e-16 under PPM, 1.1e-15 ... 1.8e-15 under van Leer and 9.2e-16 ... 9.3e-16 under van Leer + PPM, no zone beyond 1e-9
in any single-level case; the nested case by 8.0e-16 on either schedule and by 9.6e-9 in 6 zones of the child on the big-grid
kernels, as without the scalar.

A failure is read with hydromatrix.face_classes on the state before the step: the first differing zone's faces name the branch
(supersonic return, HLLE, Roe) of the kernel to look at; the scalar tests print that line themselves (hydromatrix.describe_zone)."""
import importlib
import os

import numpy as np
import pytest

import hydromatrix as hm
import orc
import twins

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NG = 4
CEILING = 1e-6           # north_star


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("atmospheric-athena_amd.lib")


@pytest.fixture(scope="module")
def aa():
    return importlib.import_module("atmospheric-athena_amd")


_fx = {}


def fixture(name):
    """the npz as a dict (a scalar fixture put together with its base: six columns), read once and shared (nobody writes into it)"""
    if name not in _fx:
        _fx[name] = hm.load(name)
        for a in _fx[name].values():
            a.setflags(write=False)
    return _fx[name]


def active(U):
    return U[NG:-NG, NG:-NG, NG:-NG] if U.shape[0] > 1 else U[:, NG:-NG, NG:-NG]


def errors(a, b):
    """|a - b| over each field's maximum [..., field]"""
    return np.abs(a - b) / np.abs(b).max(axis=tuple(range(b.ndim - 1)))


def set_knobs(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def hold_default(label, errs, twin_worst, twin_share):
    """the default build's rule (module docstring); errs: one error array per level"""
    worst = max(float(e.max()) for e in errs)
    nflip = sum(int((e > 1e-9).any(axis=-1).sum()) for e in errs)
    nzone = sum(e[..., 0].size for e in errs)
    bound = 2.0 * twin_worst
    print(f"{label}: max error {worst:.3e} (twins {twin_worst:.3e}, bound {bound:.3e}), zones beyond 1e-9: {nflip} of {nzone} "
          f"(twins {twin_share * nzone:.0f})")
    for l, e in enumerate(errs):            # the zones that moved: where to point hydromatrix.face_classes
        for z in np.argwhere((e > 1e-9).any(axis=-1))[:8]:
            print(f"    level {l} zone [k, j, i] = {z.tolist()}: errors per field {e[tuple(z)].tolist()}")
    assert worst <= bound, (label, worst, twin_worst)
    assert nflip <= 3 * twin_share * nzone, (label, nflip, twin_share * nzone)
    assert worst < CEILING, (label, worst)


def run_single(aa, lib, cfg, nx, strict, nscal=0):
    """upload the pattern, start(), NSTEP steps -> (U of the active zones, time, dt, dt0)"""
    _, integrator, order, cour, dvac, pvac = hm.CFG[cfg]
    deck = os.path.join(orc.DECKS, "athinput.blast2d" if nx[2] == 1 else "athinput.blast")
    run = aa.config.load(deck, hm.overrides(nx, cour), "blast", integrator)
    run.order = order
    run.nscal = nscal           # (the blast deck on a hydro-only NSCALARS = 1 configuration: no problem generator, the pattern is the state)
    g = lib.Grid(aa.config.slab(run), 0, strict) if nscal else lib.setup_problem(aa.config.slab(run), 0, strict)
    try:
        assert g.nvar == 5 + nscal
        blk = g.new_host_block()
        active(blk)[...] = hm.pattern(nx, run.gamma, dvac=dvac, pvac=pvac, nscal=nscal)[..., :5 + nscal]
        g.upload(blk)
        g.start()
        dt0 = g.dt
        for _ in range(hm.NSTEP):
            g.step()
        return active(g.download()).copy(), g.time, g.dt, dt0
    finally:
        g.close()


def name_the_branch(label, U0s, errs, gam, beyond=0.0):
    """print the first zone of each level whose error lies beyond `beyond`, and the outcome of the Roe solver on its faces in the
    state before the first step: which branch of the kernel to look at"""
    for l, (U0, e) in enumerate(zip(U0s, errs)):
        bad = np.argwhere((e > beyond).any(axis=-1))
        if len(bad):
            print(f"{label}: level {l}, {len(bad)} zones differ, errors per field of the first {e[tuple(bad[0])].tolist()}; "
                  + hm.describe_zone(U0, bad[0], gam))


def check_single(aa, lib, cfg, nx, strict, label, nscal=0):
    nv = 5 + nscal
    fx = fixture(hm.fixture_name(cfg, nx, nscal))
    assert fx["U"].shape[-1] == nv
    assert np.array_equal(hm.pattern(nx, hm.gamma(nx[2]), dvac=hm.CFG[cfg][4], pvac=hm.CFG[cfg][5], nscal=nscal)[..., :nv], fx["U0"]), "the uploaded pattern is the fixture's U0"
    U, time, dt, dt0 = run_single(aa, lib, cfg, nx, strict, nscal)
    err = errors(U, fx["U"])
    if nscal:
        name_the_branch(label, [fx["U0"]], [err], hm.gamma(nx[2]), 0.0 if strict else 1e-9)
    if strict:
        print(f"{label} strict: max error {err.max():.3e}, dt0 {dt0!r} dt {dt!r} time {time!r}")
        assert dt0 == float(fx["dt0"])
        assert np.array_equal(U, fx["U"]), (label, np.argwhere((U != fx["U"]).any(axis=-1))[:4].tolist(), float(err.max()))
        assert time == float(fx["time"]) and dt == float(fx["dt"])
    else:
        assert abs(dt0 / float(fx["dt0"]) - 1) < 1e-12
        if nx[2] > 1:
            w, n, nz = twins.hydro_matrix(cfg, nx, nscal)
            hold_default(label, [err], w, n / nz)
        else:
            hold_default(label, [err], *twins.hydro_matrix(cfg))


def ids(cases):
    return [c[0] + "".join("-" + k[3:] + v for k, v in c[1].items()) for c in cases]


# ---- 1. one level, 3-D ----------------------------------------------------------------------------------------------------------
BIG = {"AA_CORRECT_ALL": "1"}
CASES_3D = [("ctu", {}), ("ctu", BIG), ("ctu", dict(BIG, AA_CA_KC="3", AA_FU_KC="3")), ("ctu", {"AA_FUSED_UPDATE": "0"}),
            ("ctu", dict(BIG, AA_X3_FUSED="0")), ("ctu", dict(BIG, AA_X3_FUSED="1")),
            ("noh", {}), ("noh", BIG), ("noh", {"AA_FUSED_UPDATE": "0"}),
            ("vl", {"AA_VL_PREDICT": "0"}), ("vl", {"AA_VL_PREDICT": "1"}),
            ("ppm", {}), ("vlppm", {})]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("nx", hm.SHAPES_3D, ids=["x".join(map(str, s)) for s in hm.SHAPES_3D])
@pytest.mark.parametrize("cfg,knobs", CASES_3D, ids=ids(CASES_3D))
def test_3d_kernel_chains_on_the_designed_state(aa, lib, cfg, knobs, nx, strict, monkeypatch):
    """CTU + H-correction through the tile kernels, the big-grid kernels (k_correct_all, k_flux2_update; also at short odd chunks, with
    the x3 first pass on board and without), the unfused update; CTU without H-correction through its three chains; van Leer with the
    predictor as four kernels and as one; PPM under CTU and under van Leer.  24x20x16, and 67x10x9: across the 64-lane tile edge,
    every extent off the tile sizes."""
    set_knobs(monkeypatch, knobs)
    check_single(aa, lib, cfg, nx, strict, f"{cfg} {knobs} {nx}")


# ---- 2. one level, 2-D ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("cfl_fused", ["0", "1"])
@pytest.mark.parametrize("nx", hm.SHAPES_2D, ids=["x".join(map(str, s)) for s in hm.SHAPES_2D])
@pytest.mark.parametrize("cfg", hm.CFG_2D)
def test_2d_integrators_on_the_designed_state(aa, lib, cfg, nx, cfl_fused, strict, monkeypatch):
    """The 2-D CTU (with and without H-correction) and van Leer kernels (csrc/hydro2d_kernels.hip), new_dt's maxima taken in the
    step kernel and in a pass of their own; the third momentum is supersonic here."""
    monkeypatch.setenv("AA_CFL_FUSED", cfl_fused)
    check_single(aa, lib, cfg, (nx[0], nx[1], 1), strict, f"2-D {cfg} AA_CFL_FUSED={cfl_fused} {nx}")


# ---- 3. nested levels -----------------------------------------------------------------------------------------------------------
def run_mesh(aa, lib, tag, strict, nscal=0):
    """upload the pattern on every level, aa_mesh_start, NSTEP steps -> (whole blocks of every level, time, dt, dt0, the Grids' configs)"""
    _, integrator, case, cour, dvac, pvac = hm.SMR_CFG[tag]
    two_d = case[0][2] == 1
    deck = os.path.join(orc.DECKS, "athinput.blast2d_smr" if two_d else "athinput.blast")
    ov = hm.smr_overrides(case, cour)
    par = aa.athinput.ParTable.from_file(deck).cmdline(ov)
    run = aa.config.load(deck, ov, "blast", integrator)
    run.nscal = nscal
    # (the blast generator has no scalar and refuses NSCALARS = 1: with one the levels are created without it, the pattern is the state)
    m = lib.Mesh((aa.config.levels_2d if two_d else aa.config.levels)(par, run), 0, strict, initial=not nscal)
    try:
        for g in m.lev:
            c = g.cfg
            blk = g.new_host_block()
            assert g.nvar == 5 + nscal
            active(blk)[...] = hm.pattern(tuple(c.Nx), run.gamma, c.level, tuple(c.disp) if c.level else (0, 0, 0), dvac, pvac, nscal)[..., :5 + nscal]
            g.upload(blk)
        m.start()
        dt0 = m.dt
        for _ in range(hm.NSTEP):
            m.step()
        assert m.nstep == hm.NSTEP
        return [g.download() for g in m.lev], m.time, m.dt, dt0
    finally:
        m.close()


SMR_CASES = [("3d_ctu", {}), ("3d_ctu", {"AA_SMR_ONE_LAUNCH": "0", "AA_MESH_OVERLAP": "0"}), ("3d_ctu", BIG),
             ("2d_ctu", {}), ("2d_ctu", {"AA_SMR_ONE_LAUNCH": "0", "AA_MESH_OVERLAP": "0"}),
             ("2d_vl", {}), ("2d_vl", {"AA_SMR_ONE_LAUNCH": "0", "AA_MESH_OVERLAP": "0"}),
             ("2d_vl_floor", {}), ("2d_vl_floor", {"AA_SMR_ONE_LAUNCH": "0", "AA_MESH_OVERLAP": "0"})]
SMR_RUNS = [(t, k, st) for t, k in SMR_CASES for st in (True, False) if st or t not in hm.STRICT_ONLY]
SMR_IDS = [i + ("-strict" if st else "-default") for i, (t, k) in zip(ids(SMR_CASES), SMR_CASES) for st in (True, False)
           if st or t not in hm.STRICT_ONLY]


@pytest.mark.parametrize("tag,knobs,strict", SMR_RUNS, ids=SMR_IDS)
def test_nested_levels_on_the_designed_state(aa, lib, tag, knobs, strict, monkeypatch):
    """Two levels in 3-D (default schedule, one launch per side with the levels one after the other, the big-grid kernels forced on
    the levels) and three levels in 2-D (CTU and van Leer, both schedules; van Leer also with the floored pressure at the level
    boundaries, strict build only).  Every side of every child lies on a block edge across
    which the flow recedes: the fluxes kept for the flux correction come from HLLE, upwind and Roe faces."""
    set_knobs(monkeypatch, knobs)
    check_mesh(aa, lib, tag, strict, f"nested {tag} {knobs}")


def check_mesh(aa, lib, tag, strict, label, nscal=0):
    nv = 5 + nscal
    fx = fixture(hm.smr_fixture_name(tag, nscal))
    _, integrator, case, cour, dvac, pvac = hm.SMR_CFG[tag]
    for l in range(int(fx["nlevels"])):
        U0 = hm.pattern(tuple(fx["nxs"][l]), hm.gamma(case[0][2]), int(fx["levels"][l]), tuple(fx["disp"][l]), dvac, pvac, nscal)
        assert fx[f"U_{l}"].shape[-1] == nv
        assert np.array_equal(U0[..., :nv], fx[f"U0_{l}"]), f"the uploaded pattern is the fixture's U0, level {l}"
    blocks, time, dt, dt0 = run_mesh(aa, lib, tag, strict, nscal)
    errs = [errors(active(U), fx[f"U_{l}"]) for l, U in enumerate(blocks)]
    if nscal:
        name_the_branch(label, [fx[f"U0_{l}"] for l in range(len(blocks))], errs, hm.gamma(case[0][2]), 0.0 if strict else 1e-9)
    if strict:
        print(f"{label} strict: max error per level {[float(e.max()) for e in errs]}, dt0 {dt0!r} dt {dt!r}")
        assert dt0 == float(fx["dt0"])
        for l, U in enumerate(blocks):
            assert np.array_equal(active(U), fx[f"U_{l}"]), (label, l, np.argwhere((active(U) != fx[f"U_{l}"]).any(axis=-1))[:4].tolist())
        assert time == float(fx["time"]) and dt == float(fx["dt"])
        if case[0][2] > 1:          # the whole blocks, ghost zones as Prolongate left them, against the oracle
            o = oracle_mesh_blocks(tag, nscal)
            for l, U in enumerate(blocks):
                assert np.array_equal(U, o[l]), (label, "whole block", l, np.argwhere((U != o[l]).any(axis=-1))[:4].tolist())
    else:
        assert abs(dt0 / float(fx["dt0"]) - 1) < 1e-12
        cfg = {"ctu": "ctu", "vl": "vl"}[integrator]
        hold_default(label, errs, *twins.hydro_matrix(cfg, None, nscal))


_oracle_blocks = {}


def oracle_mesh_blocks(tag, nscal=0):
    if (tag, nscal) not in _oracle_blocks:
        m = hm.make_mesh(tag, nscal).start()
        for _ in range(hm.NSTEP):
            m.step()
        _oracle_blocks[tag, nscal] = [s.U[..., :5 + nscal].copy() for s in m.lev]
    return _oracle_blocks[tag, nscal]


# ---- 4. one level, 3-D, with a passive scalar ------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("nx", hm.SHAPES_3D, ids=["x".join(map(str, s)) for s in hm.SHAPES_3D])
@pytest.mark.parametrize("cfg,knobs", CASES_3D, ids=ids(CASES_3D))
def test_3d_kernel_chains_with_a_passive_scalar(aa, lib, cfg, knobs, nx, strict, monkeypatch):
    """Every chain of section 1 on six variables: the NS = 1 instantiations without a potential (the ones every scalar run without
    gravity takes).  The concentration differs across every face, so the scalar flux's rule behind each exit of the Roe solver
    (upwind returns, HLLE, the Roe path's choice by the sign of the mass flux), the sixth column of the reconstruction and the
    tracing, and the sixth variable's way through tiles, halos and parked fluxes all carry data, differently along x1, x2 and x3.
    67x10x9 crosses the 64-lane tile edge along x1 with every extent off the tile sizes: the smallest Grid on which k_correct_all's
    x1 halo of the sixth variable and its tile-edge fluxes are read; 24x20x16 has several rows of tiles along x2."""
    set_knobs(monkeypatch, knobs)
    check_single(aa, lib, cfg, nx, strict, f"scalar {cfg} {knobs} {nx}", nscal=1)


# ---- 5. nested levels with a passive scalar ----------------------------------------------------------------------------------------
SMR_SCALAR = [(t, k) for t, k in SMR_CASES if t in hm.SCAL_SMR]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("tag,knobs", SMR_SCALAR, ids=ids(SMR_SCALAR))
def test_nested_levels_with_a_passive_scalar(aa, lib, tag, knobs, strict, monkeypatch):
    """The 3-D nested case on six variables under its three knob sets: restriction, prolongation (the scalar's slopes) and flux
    correction of the sixth column.  Strict build: every level's active zones against the fixture and the whole blocks, ghost zones
    as the prolongation left them, against the oracle; default build: the single-level twins of the six-variable CTU run."""
    set_knobs(monkeypatch, knobs)
    check_mesh(aa, lib, tag, strict, f"scalar nested {tag} {knobs}", nscal=1)
