"""2-D Grids (Nx3 = 1) on an MI355X: the 2-D CTU and van Leer integrators (csrc/hydro2d_kernels.hip), bvals_mhd and new_dt of a
2-D Grid, the problem generators, the outputs and the refusals.

The reference is the set of restart states and output files the unmodified reference executables left on decks with Nx3 = 1
(tests/golden/g2d_*.npz, tests/golden/make_golden_2d.py): the strict library reproduces them bit for bit, the default library
within the bars of the 3-D hydro fixtures (test_gpu_parity.py: 1e-11 of each field's maximum, 1e-12 in dt)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import twodfix                      # noqa: E402
from twodfix import pkg, fixture    # noqa: E402

pytestmark = pytest.mark.gpu
NG = twodfix.NG


def relerr(a, b):
    """max |a-b| / max|b| per variable; a variable that vanishes identically in the reference must vanish here too"""
    out = []
    for c in range(a.shape[-1]):
        scale = np.abs(b[..., c]).max()
        diff = float(np.abs(a[..., c] - b[..., c]).max())
        out.append(diff / scale if scale > 0 else (0.0 if diff == 0.0 else np.inf))
    return out


def run_fixture(fx, strict, env=None):
    lib = pkg("lib")
    gc = twodfix.grid_config(fx)
    g = lib.Grid(gc, 0, strict)
    g.upload(twodfix.host_block(gc, fx["U0"]))
    g.start()
    dt0 = g.dt
    for _ in range(int(fx["nstep"])):
        g.step()
    return g, gc, dt0


# ---- 1. every fixture: CTU + H-correction, CTU without, van Leer; every grid size around the kernels' tiles -------------------
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("name", twodfix.STEP_FIXTURES)
def test_steps_reproduce_the_reference(name, strict):
    fx = fixture(name)
    g, gc, dt0 = run_fixture(fx, strict)
    U = g.download()
    assert U.shape == (1, gc.Nx[1] + 2 * NG, gc.Nx[0] + 2 * NG, 5)
    Ua = U[:, NG:-NG, NG:-NG, :]
    err = relerr(Ua, fx["U"])
    print(f"{name} strict={strict}: relerr {err} dt {g.dt!r} / {float(fx['dt'])!r}")
    assert g.nstep == int(fx["nstep"])
    if strict:
        assert dt0 == float(fx["dt0"])
        assert np.array_equal(Ua, fx["U"]), err
        assert g.time == float(fx["time"]) and g.dt == float(fx["dt"])
    else:
        assert max(err) < 1e-11, err
        assert abs(g.dt / float(fx["dt"]) - 1) < 1e-12
    g.close()


def test_every_integrator_and_tile_case_has_a_fixture():
    names = twodfix.STEP_FIXTURES
    for integ in ("ctu", "ctu-noh", "vl"):
        for size in ("4x4", "5x7", "64x8", "63x6", "64x7", "65x8", "130x9", "67x35"):
            assert any(n.startswith(f"g2d_blast_{integ}_c4_{size}_") for n in names), (integ, size)
    assert sum(n.startswith("g2d_shk_") for n in names) == 8 and sum("_c8_" in n for n in names) == 8


# ---- 2. bvals_mhd of a 2-D Grid: four sides, corners by the x1-then-x2 order -------------------------------------------------
@pytest.mark.parametrize("bc", [(1, 2, 4, 4), (4, 4, 2, 1), (2, 1, 1, 2), (1, 1, 4, 4)])
@pytest.mark.parametrize("nx", [(5, 7), (67, 9)])
def test_bvals_mhd_fills_the_four_sides_and_corners(bc, nx):
    aa = pkg(); lib = pkg("lib")
    ov = [f"domain1/Nx1={nx[0]}", f"domain1/Nx2={nx[1]}", "domain1/Nx3=1"] + \
         [f"domain1/bc_{s}={f}" for s, f in zip(("ix1", "ox1", "ix2", "ox2"), bc)]
    run = aa.config.load(os.path.join(twodfix.DECKS, "athinput.shkset2d"), ov, "shkset1d")
    gc = aa.config.slab(run)
    rng = np.random.default_rng(7)
    blk = rng.uniform(-1.0, 1.0, size=(1, nx[1] + 2 * NG, nx[0] + 2 * NG, 5))
    want = twodfix.bvals_2d(blk, gc.bc)
    for strict in (True, False):
        g = lib.Grid(gc, 0, strict)
        g.upload(blk)
        g.bvals_mhd()
        assert np.array_equal(g.download(), want)
        # the ghost-zone download moves the same shell into a block whose active zones are current
        mine = blk.copy(); mine[0, :NG] = 0; mine[0, -NG:] = 0; mine[0, :, :NG] = 0; mine[0, :, -NG:] = 0
        g.download_ghost_zones(mine)
        assert np.array_equal(mine, want)
        g.close()


# ---- 3. the problem generators on 2-D Grids give the reference's step-0 state -------------------------------------------------
@pytest.mark.parametrize("name", ["g2d_blast_ctu_c4_5x7_s5", "g2d_blast_ctu_c4_67x35_s5", "g2d_shk_ctu_d1_refl_48x8_s12",
                                  "g2d_shk_ctu_d2_per_8x48_s12"])
def test_problem_generators_give_the_reference_state(name):
    lib = pkg("lib")
    fx = fixture(name)
    g = lib.setup_problem(twodfix.grid_config(fx), 0, True)
    assert g.host_initial.shape[0] == 1
    assert np.array_equal(g.host_initial[:, NG:-NG, NG:-NG, :], fx["U0"])
    assert np.array_equal(g.download()[:, NG:-NG, NG:-NG, :], fx["U0"])
    g.close()


# ---- 4. the third momentum under van Leer: a uniform v3 changes nothing else and stays uniform -------------------------------
@pytest.mark.parametrize("strict", [True, False])
def test_van_leer_carries_a_uniform_third_velocity(strict):
    """No van Leer target of the reference can carry v3 != 0 (blast.c sets no velocity).  In real arithmetic a uniform v3 added
    to a state with v3 = 0 leaves d, M1, M2 alone and M3/d = v3; what rounding makes of that was measured on the reference's own
    2-D CTU path (g2d_v3cal.npz: D_ref = 3.2e-16 in d, M1, M2 and 5.6e-17 in M3/d), and one decade covers the different
    operation count."""
    aa = pkg(); lib = pkg("lib")
    cal = fixture("g2d_v3cal")
    v3 = float(cal["v3"])
    ov = ["domain1/Nx1=67", "domain1/Nx2=35", "problem/prat=10.0", "problem/radius=0.3", "time/cour_no=0.4"]
    run = aa.config.load(os.path.join(twodfix.DECKS, "athinput.blast2d"), ov, "blast", "vl")
    out = []
    for add in (0.0, v3):
        g = lib.setup_problem(aa.config.slab(run), 0, strict)
        U = g.host_initial.copy()
        U[..., 3] = U[..., 0] * add
        U[..., 4] = U[..., 4] + 0.5 * U[..., 0] * add * add
        g.upload(U)
        g.start()
        for _ in range(int(cal["nstep"])):
            g.step()
        out.append(g.download()[:, NG:-NG, NG:-NG, :])
        g.close()
    a, b = out
    assert np.abs(a[..., 1]).max() > 0 and np.abs(a[..., 2]).max() > 0 and np.all(a[..., 3] == 0.0)
    d_state = max(float(np.abs(a[..., c] - b[..., c]).max() / np.abs(a[..., c]).max()) for c in (0, 1, 2))
    d_v3 = float(np.abs(b[..., 3] / b[..., 0] - v3).max())
    print(f"strict={strict}: D(d, M1, M2) = {d_state:.3e} (D_ref {float(cal['D_ref_state']):.3e})  "
          f"D(M3/d - v3) = {d_v3:.3e} (D_ref {float(cal['D_ref_v3']):.3e})")
    assert d_state <= 10.0 * float(cal["D_ref_state"])
    assert d_v3 <= 10.0 * float(cal["D_ref_v3"])


# ---- 5. Driver.main on the 2-D deck with hst + bin + vtk + rst blocks; resumed from the middle dump ----------------------------
def _out_par(fx):
    blocks = json.loads(str(fx["blocks"]))
    ov = [str(o) for o in fx["overrides"]] + [f"job/maxout={max(int(n) for n in blocks)}"]
    for n, kv in blocks.items():
        ov += [f"output{n}/{k}={v}" for k, v in kv.items()]
    return pkg("athinput").ParTable.from_file(os.path.join(twodfix.DECKS, "athinput.blast2d")).cmdline(ov), blocks


def _payload(b):
    return b[b.index(b"<par_end>\n") + len(b"<par_end>\n"):]


def test_driver_main_writes_the_references_files_and_resumes(tmp_path):
    """vtk and bin byte for byte (headers included), rst: everything behind the parameter dump byte for byte and every block's
    num / time in it, hst: the header and every column as printed -- except the net momenta, which in this symmetric run are the
    rounding noise of the order in which the reference adds the zones up (1e-18; held to 1e-9 of the mass, the rule of
    test_history.py).  Then Driver.from_restart from the middle dump arrives at the same final state bit for bit."""
    fx = fixture("g2d_out_blast_24x20")
    paths = [str(p) for p in fx["paths"]]
    files = {p: fx[f"file_{i}"].tobytes() for i, p in enumerate(paths)}
    cfg = pkg("config"); D = pkg("driver"); O = pkg("outputs"); A = pkg("athinput")
    par, blocks = _out_par(fx)
    run = cfg.from_par(par, "blast")
    full = str(tmp_path / "full")
    d = D.Driver(run, strict=True)
    d.main(O.OutputSet.from_par(par, 0.0, full))
    got = sorted(os.path.relpath(os.path.join(dp, f), full) for dp, _, fs in os.walk(full) for f in fs)
    assert got == paths, (got, paths)
    nx = (int(fx["nx"][0]), int(fx["nx"][1]), 1)
    for rel in paths:
        ours = open(os.path.join(full, rel), "rb").read(); ref = files[rel]
        ext = rel.rsplit(".", 1)[1]
        if ext in ("vtk", "bin"):
            n = {"bin": "2", "vtk": "3"}[ext]
            import dumpfix
            assert dumpfix.compare_dump(ours, ref, nx, 0, ext, blocks[n].get("out", "cons") == "prim", rel) == 0
        elif ext == "rst":
            assert _payload(ours) == _payload(ref), rel
            po = A.ParTable.from_text(ours[:ours.index(b"<par_end>")].decode()); pr = A.ParTable.from_text(ref[:ref.index(b"<par_end>")].decode(errors="replace"))
            for n in blocks:
                assert po.geti(f"output{n}", "num") == pr.geti(f"output{n}", "num"), (rel, n)
                assert po.getd(f"output{n}", "time") == pr.getd(f"output{n}", "time"), (rel, n)
            assert po.getd("time", "time") == pr.getd("time", "time") and po.geti("time", "nstep") == pr.geti("time", "nstep")
        else:
            lo, lr = ours.decode().splitlines(), ref.decode().splitlines()
            assert lo[:3] == lr[:3] and len(lo) == len(lr) == 7
            for a, b in zip(lo[3:], lr[3:]):
                ca, cb = a.split(), b.split()
                assert ca[:4] == cb[:4] and ca[7:] == cb[7:], (a, b)
                assert all(abs(float(x) - float(y)) <= 1e-9 * float(cb[2]) for x, y in zip(ca[4:7], cb[4:7])), (a, b)
    Ufull = d.eng.download(); state = (d.time, d.dt, d.nstep)
    d.eng.close()
    res = str(tmp_path / "resumed")
    r = D.Driver.from_restart(os.path.join(full, "Blast.0001.rst"), strict=True)
    assert r.restarted and 0 < r.nstep < state[2] and r.grid.Nx == nx
    r.main(O.OutputSet.from_par(r.par, r.time, res))
    assert (r.time, r.dt, r.nstep) == state
    assert np.array_equal(r.eng.download(), Ufull)
    # the seed's table says dump 0003 is due at 0.015, which has passed: like the reference, the resumed run writes it at once
    # (the seed's own state again) and the final one as 0004
    for rel, of_full in (("Blast.0002.rst", "Blast.0002.rst"), ("Blast.0003.bin", "Blast.0002.bin"), ("Blast.0003.vtk", "Blast.0002.vtk"),
                         ("Blast.0004.bin", "Blast.0003.bin"), ("Blast.0004.vtk", "Blast.0003.vtk")):
        a, b = open(os.path.join(res, rel), "rb").read(), open(os.path.join(full, of_full), "rb").read()
        assert (_payload(a) == _payload(b)) if rel.endswith(".rst") else (a == b), rel
    r.eng.close()


# ---- 6. new_dt's maxima from the update kernel against the CFL kernel ---------------------------------------------------------
@pytest.mark.parametrize("name", ["g2d_blast_ctu_c8_67x35_s4", "g2d_blast_vl_c4_65x8_s6", "g2d_shk_ctu-noh_d2_refl_8x48_s12"])
def test_fused_cfl_maxima_give_the_same_dt(name, monkeypatch):
    fx = fixture(name)
    monkeypatch.setenv("AA_CFL_FUSED", "0")
    g0, _, _ = run_fixture(fx, True)
    monkeypatch.delenv("AA_CFL_FUSED")
    g1, _, _ = run_fixture(fx, True)
    assert g0.dt == g1.dt == float(fx["dt"]) and g0.time == g1.time
    assert np.array_equal(g0.download(), g1.download())
    # and by hand: the integrator with the maxima on board, then new_dt's own kernel on the same state
    g1.cfl_in_update(True); g1.integrate(); fused = g1.new_dt_local()
    assert fused == g1.new_dt_local()
    v = g1.cfl_max_v()
    assert v[0] > 0 and v[1] > 0 and v[2] == 0.0
    g0.close(); g1.close()


# ---- 7. what is refused on a 2-D Grid, and the entry points of the other dimension ------------------------------------------------
def test_refusals_set_the_last_error():
    aa = pkg(); lib = pkg("lib")
    run = aa.config.load(os.path.join(twodfix.DECKS, "athinput.blast2d"), ["domain1/Nx1=8", "domain1/Nx2=8", "time/cour_no=0.4"], "blast", "vl")
    g = lib.Grid(aa.config.slab(run), 0, True)
    L = g.L

    def refused(rc, *words):
        msg = L.aa_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)
    refused(L.aa_add_radplane_3d(g._h, -1, 1.0), "2-D")
    refused(L.aa_set_static_grav_pot(g._h, lib.GRAVPOT(lambda x, y, z: 0.0)), "gravity", "2-D")
    t = np.zeros((1, 16, 16))
    refused(L.aa_set_static_grav_tables(g._h, lib._dp(t), lib._dp(t), lib._dp(t), lib._dp(t)), "gravity", "2-D")
    refused(L.aa_set_fofc(g._h, 1), "2-D")
    refused(L.aa_integrate_3d_ctu(g._h), "2-D", "aa_integrate_2d_ctu")
    refused(L.aa_integrate_3d_vl(g._h), "2-D", "aa_integrate_2d_vl")
    refused(L.aa_integrate_2d_ctu(g._h), "van Leer")
    import ctypes as C
    hs = (C.c_void_p * 1)(g._h); disp = (C.c_int * 3)(0, 0, 0); m = C.c_void_p()
    refused(L.aa_mesh_create(1, hs, disp, C.byref(m)), "2-D")
    g.close()
    run = aa.config.load(os.path.join(twodfix.DECKS, "athinput.blast2d"), ["domain1/Nx1=8", "domain1/Nx2=8"], "blast")
    g = lib.Grid(aa.config.slab(run), 0, True)
    refused(L.aa_set_cooling(g._h, 1), "cooling", "2-D")
    g.close()
    # the 2-D entry points on a 3-D Grid
    run3 = aa.config.load(os.path.join(twodfix.DECKS, "athinput.blast"), ["domain1/Nx1=8", "domain1/Nx2=8", "domain1/Nx3=8"], "blast")
    g3 = lib.Grid(aa.config.slab(run3), 0, True)
    refused(L.aa_integrate_2d_ctu(g3._h), "3-D")
    refused(L.aa_integrate_2d_vl(g3._h), "3-D")
    g3.close()
    # aa_create: the other degenerate shapes with the reference's messages (integrate.c:81-84), van Leer above 0.5
    p = lib.params_from_grid(aa.config.slab(run))
    h = C.c_void_p()
    p.Nx[1] = 1; p.Nx[2] = 8
    refused(L.aa_create(C.byref(p), C.byref(h)), "2D problem must have Nx1 and Nx2 > 1")
    p.Nx[0] = 1; p.Nx[1] = 8; p.Nx[2] = 1
    refused(L.aa_create(C.byref(p), C.byref(h)), "1D problem must have Nx1 > 1")
    p.Nx[0] = 8; p.Nx[1] = 1; p.Nx[2] = 1
    refused(L.aa_create(C.byref(p), C.byref(h)), "1-D")
    p.Nx[1] = 8; p.integrator = 1; p.cour_no = 0.8
    refused(L.aa_create(C.byref(p), C.byref(h)), "must be <= 0.5 with 2D VL integrator")
    p.integrator = 0; p.nscal = 1
    refused(L.aa_create(C.byref(p), C.byref(h)), "scalars")
    p.nscal = 0; p.order = 3
    refused(L.aa_create(C.byref(p), C.byref(h)), "third-order")
    p.order = 2; p.nslab = 2
    refused(L.aa_create(C.byref(p), C.byref(h)), "slabs")
    p.nslab = 1                                   # ... and cour_no 0.8 is fine with the CTU integrator
    assert L.aa_create(C.byref(p), C.byref(h)) == 0, L.aa_last_error()
    L.aa_destroy(h)
