"""1-D Grids (Nx2 = Nx3 = 1) on an MI355X: the 1-D CTU and van Leer integrators at second and third order
(csrc/hydro1d_kernels.hip: k1d_step, one launch per step, and k1d_run, many steps in one launch), bvals_mhd and new_dt of a 1-D
Grid, the problem generators, the outputs and the refusals.

The reference is the set of restart states and output files the unmodified reference executables left on decks with
Nx2 = Nx3 = 1 (tests/golden/g1d_*.npz, tests/golden/make_golden_1d.py): the strict library reproduces them bit for bit, the
default library within the bars test_gpu_2d.py holds for the same run lengths (1e-11 of each field's maximum, 1e-12 in dt)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import onedfix                      # noqa: E402
from onedfix import pkg, fixture    # noqa: E402

pytestmark = pytest.mark.gpu
NG = onedfix.NG


def relerr(a, b):
    """max |a-b| / max|b| per variable; a variable that vanishes identically in the reference must vanish here too"""
    out = []
    for c in range(a.shape[-1]):
        scale = np.abs(b[..., c]).max()
        diff = float(np.abs(a[..., c] - b[..., c]).max())
        out.append(diff / scale if scale > 0 else (0.0 if diff == 0.0 else np.inf))
    return out


def started(fx, strict, integrator=None, extra=()):
    lib = pkg("lib")
    gc = onedfix.grid_config(fx, extra, integrator)
    g = lib.Grid(gc, 0, strict)
    g.upload(onedfix.host_block(gc, fx["U0"]))
    g.start()
    return g, gc


def check_against(fx, g, gc, dt0, strict, what):
    U = g.download()
    assert U.shape == (1, 1, gc.Nx[0] + 2 * NG, 5)
    Ua = U[:, :, NG:-NG, :]
    err = relerr(Ua, fx["U"])
    print(f"{what} strict={strict}: relerr {err} dt {g.dt!r} / {float(fx['dt'])!r}")
    assert g.nstep == int(fx["nstep"])
    if strict:
        assert dt0 == float(fx["dt0"])
        assert np.array_equal(Ua, fx["U"]), err
        assert g.time == float(fx["time"]) and g.dt == float(fx["dt"])
    else:
        assert max(err) < 1e-11, err
        assert abs(g.dt / float(fx["dt"]) - 1) < 1e-12
    # the ghost zones are what bvals_mhd makes of the active ones
    assert np.array_equal(U, onedfix.bvals_1d(U, gc.bc))


# ---- 1. every fixture through Grid.step() (k1d_step) and, where it fits, through Grid.run_until() (k1d_run) ---------------------
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("name", onedfix.STEP_FIXTURES)
def test_steps_reproduce_the_reference(name, strict):
    fx = fixture(name)
    g, gc, = started(fx, strict)
    assert g.ndim == 1 and g.N == (gc.Nx[0] + 2 * NG, 1, 1)
    dt0 = g.dt
    for _ in range(int(fx["nstep"])):
        g.step()
    check_against(fx, g, gc, dt0, strict, name + " step")
    g.close()
    g, gc = started(fx, strict)
    dt0 = g.dt
    if gc.Nx[0] <= g.run_cap():
        assert g.run_until(1e300, nstep_stop=int(fx["nstep"])) == int(fx["nstep"])
        check_against(fx, g, gc, dt0, strict, name + " run_until")
    else:                                       # above the resident cap: an error, and the Grid steps one launch at a time
        assert gc.Nx[0] == onedfix.R + 1
        with pytest.raises(pkg("lib").AthenaError, match="resident"):
            g.run_until(1e300, nstep_stop=int(fx["nstep"]))
        assert g.nstep == 0
    g.close()


def test_kernel_shapes_are_the_ones_the_fixtures_were_sized_for():
    L = pkg("lib").load(True)
    assert L.aa_step_1d_block() == onedfix.B and L.aa_run_1d_cap() == onedfix.R >= 1200


# ---- 2. the reference's own deck to tlim: one launch, arbitrary cuts, single steps, AA_1D_RESIDENT=0 ----------------------------
def _sod_grid(strict=True):
    lib = pkg("lib")
    run = pkg("config").load(os.path.join(onedfix.DECKS, "athinput.sod1d"), None, "shkset1d", "ctu-noh")
    g = lib.setup_problem(pkg("config").slab(run), 0, strict)
    g.start()
    return g, run


def test_full_sod_run_in_one_launch_and_cut_anywhere(monkeypatch):
    fx = fixture("g1d_sod_full")
    times, dts = [float(t) for t in fx["times"]], [float(t) for t in fx["dts"]]
    tlim = float(fx["tlim"])
    # the problem generator gives the reference's step-0 state
    g, run = _sod_grid()
    assert run.tlim == tlim
    assert np.array_equal(g.host_initial[:, :, NG:-NG, :], fx["U0"]) and g.dt == float(fx["dt0"])
    # (a) one launch to tlim
    n = g.run_until(tlim)
    assert n == 87 == g.nstep and g.time == tlim == times[-1] and g.dt == dts[-1]
    Ufull = g.download()
    assert np.array_equal(Ufull[:, :, NG:-NG, :], fx["U"])
    assert g.run_until(tlim) == 0 and g.nstep == 87               # time >= t_stop: nothing to do
    g.close()
    # (b) 87 launches of one step each: the reference's (time, dt) after every step, the last dt clipped at tlim
    g, _ = _sod_grid()
    for k in range(87):
        assert g.run_until(tlim, nstep_stop=k + 1) == 1
        assert (g.time, g.dt) == (times[k], dts[k]), k
    assert times[-2] + dts[-2] == tlim and np.array_equal(g.download(), Ufull)
    g.close()
    # (c) cut at arbitrary times and step counts, mixed with single steps of k1d_step
    g, _ = _sod_grid()
    g.run_until(0.013); k = g.nstep
    assert 0 < k < 87 and times[k - 1] >= 0.013 > times[k - 2] and (g.time, g.dt) == (times[k - 1], dts[k - 1])
    g.step(); g.step(); k += 2
    assert (g.time, g.dt) == (times[k - 1], dts[k - 1])
    assert g.run_until(tlim, nstep_stop=k + 17) == 17
    g.run_until(0.2); k = g.nstep
    assert times[k - 1] >= 0.2 > times[k - 2]
    g.run_until(tlim)
    assert g.nstep == 87 and (g.time, g.dt) == (times[-1], dts[-1]) and np.array_equal(g.download(), Ufull)
    g.close()
    # (d) 87 single steps
    g, _ = _sod_grid()
    for k in range(87):
        g.step()
        assert (g.time, g.dt) == (times[k], dts[k]), k
    assert np.array_equal(g.download(), Ufull)
    g.close()
    # (e) the knob: the same call steps one launch at a time
    monkeypatch.setenv("AA_1D_RESIDENT", "0")
    g, _ = _sod_grid()
    g.host_syncs(True)
    assert g.run_until(tlim) == 87 and (g.time, g.dt, g.nstep) == (times[-1], dts[-1], 87)
    assert g.host_syncs() >= 87                                      # a read-back per step; the resident run has one per call
    assert np.array_equal(g.download(), Ufull)
    g.close()
    monkeypatch.delenv("AA_1D_RESIDENT")
    g, _ = _sod_grid()
    g.host_syncs(True); g.run_until(tlim)
    assert g.host_syncs() == 1
    g.close()


def test_run_until_refuses_what_it_cannot_do():
    g, run = _sod_grid()
    lib = pkg("lib")
    with pytest.raises(lib.AthenaError, match="2\\^20"):
        g.run_until(run.tlim, nstep_stop=(1 << 20) + 1)
    with pytest.raises(lib.AthenaError, match="2\\^20"):
        g.run_until(run.tlim, nstep_stop=-1)
    with pytest.raises(lib.AthenaError, match="tlim"):
        g.run_until(run.tlim, tlim=1.0)
    g.set_pinned_cells(np.array([NG + 3]), np.array([[1.0, 0.0, 0.0, 0.0, 2.5]]))
    with pytest.raises(lib.AthenaError, match="pinned"):
        g.run_until(run.tlim)
    g.step()                                    # ... and the per-step path takes them
    assert np.array_equal(g.download()[0, 0, NG + 3], [1.0, 0.0, 0.0, 0.0, 2.5])
    g.close()
    aa = pkg()
    run2 = aa.config.load(os.path.join(onedfix.DECKS, "athinput.blast2d"), ["domain1/Nx1=8", "domain1/Nx2=8"], "blast")
    g2 = lib.Grid(aa.config.slab(run2), 0, True)
    with pytest.raises(lib.AthenaError, match="2-D"):
        g2.run_until(1.0)
    g2.close()


# ---- 3. integrators 0 and 2 are one thing in 1-D ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1d_shk_ctu-noh_bc1_c4_249_s8", "g1d_blast_ctu_o3_c8_65_s6"])
def test_integrators_0_and_2_give_the_same_bits(name):
    fx = fixture(name)
    out = []
    for integ in ("ctu", "ctu-noh"):
        g, gc = started(fx, True, integ)
        assert g.params.integrator == {"ctu": 0, "ctu-noh": 2}[integ]
        for _ in range(int(fx["nstep"])):
            g.step()
        out.append((g.download(), g.time, g.dt))
        g.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1:] == out[1][1:] == (float(fx["time"]), float(fx["dt"]))


# ---- 4. bvals_mhd of a 1-D Grid: the x1 pass only -------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(1, 2), (2, 4), (4, 1), (1, 1), (4, 4)])
@pytest.mark.parametrize("n", [4, 5, 249])
def test_bvals_mhd_fills_the_eight_ghost_zones(bc, n):
    aa = pkg(); lib = pkg("lib")
    ov = [f"domain1/Nx1={n}", f"domain1/bc_ix1={bc[0]}", f"domain1/bc_ox1={bc[1]}"]
    run = aa.config.load(os.path.join(onedfix.DECKS, "athinput.sod1d"), ov, "shkset1d")
    gc = aa.config.slab(run)
    rng = np.random.default_rng(11)
    blk = rng.uniform(-1.0, 1.0, size=(1, 1, n + 2 * NG, 5))
    want = onedfix.bvals_1d(blk, gc.bc)
    if bc[0] == 1:                              # reflecting: M1 alone changes sign
        assert np.array_equal(want[0, 0, :NG, 1], -blk[0, 0, 2 * NG - 1:NG - 1:-1, 1])
        assert np.array_equal(want[0, 0, :NG, [0, 2, 3, 4]], blk[0, 0, 2 * NG - 1:NG - 1:-1, [0, 2, 3, 4]])
    for strict in (True, False):
        g = lib.Grid(gc, 0, strict)
        g.upload(blk)
        g.bvals_mhd()
        assert np.array_equal(g.download(), want)
        mine = blk.copy(); mine[0, 0, :NG] = 0; mine[0, 0, -NG:] = 0
        g.download_ghost_zones(mine)
        assert np.array_equal(mine, want)
        for d in (1, 2):                        # no boundary functions along x2, x3
            g.bvals_mhd_side(d, 0); g.bvals_mhd_side(d, 1)
        assert np.array_equal(g.download(), want)
        g.close()


# ---- 5. new_dt's maximum from the step kernel against the CFL kernel --------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1d_shk_ctu-noh_bc4_c8_746_s7", "g1d_blast_vl_o3_c4_249_s6", "g1d_blast_ctu_o3_c8_4_s6"])
def test_fused_cfl_maximum_gives_the_same_dt(name, monkeypatch):
    fx = fixture(name)
    monkeypatch.setenv("AA_CFL_FUSED", "0")
    g0, _ = started(fx, True)
    monkeypatch.delenv("AA_CFL_FUSED")
    g1, _ = started(fx, True)
    for g in (g0, g1):
        for _ in range(int(fx["nstep"])):
            g.step()
    assert g0.dt == g1.dt == float(fx["dt"]) and g0.time == g1.time
    assert np.array_equal(g0.download(), g1.download())
    # and by hand: the integrator with the maximum on board, then new_dt's own kernel on the same state
    g1.cfl_in_update(True); g1.integrate(); fused = g1.new_dt_local()
    assert fused == g1.new_dt_local()
    v = g1.cfl_max_v()
    assert v[0] > 0 and v[1] == 0.0 and v[2] == 0.0
    assert fused == g1.cfg.run.cour_no / (v[0] / g1.cfg.run.dx[0])
    g0.close(); g1.close()


# ---- 6. Driver.main on the 1-D deck with hst + vtk + bin + rst blocks, batched and not; resumed from a dump -------------------------
def _out_par(fx):
    blocks = json.loads(str(fx["blocks"]))
    ov = [str(o) for o in fx["overrides"]] + [f"job/maxout={max(int(n) for n in blocks)}"]
    for n, kv in blocks.items():
        ov += [f"output{n}/{k}={v}" for k, v in kv.items()]
    return pkg("athinput").ParTable.from_file(os.path.join(onedfix.DECKS, "athinput.sod1d")).cmdline(ov), blocks


def _payload(b):
    return b[b.index(b"<par_end>\n") + len(b"<par_end>\n"):]


def _tree(d):
    return sorted(os.path.relpath(os.path.join(dp, f), d) for dp, _, fs in os.walk(d) for f in fs)


def _same_hst(ours, ref, volume):
    """the header and every column as printed, as test_gpu_2d.py holds them: the sums are taken over states that are the
    reference's bit for bit, so only the order of the additions differs (1e-16 of a sum, against the 1e-7 of a printed digit),
    and M1 does not cancel in a shock tube.  Every row that differs is printed before the assertion."""
    lo, lr = ours.decode().splitlines(), ref.decode().splitlines()
    assert lo[:3] == lr[:3] and len(lo) == len(lr) == 9
    assert "volume=%e" % volume in lo[0]                        # dump_history.c:316-321: the x1 extent alone
    bad = [(a, b) for a, b in zip(lo[3:], lr[3:]) if a.split() != b.split()]
    for a, b in bad:
        print("hst row differs:\n  ours %s\n  ref  %s" % (a, b))
    assert not bad, bad


@pytest.mark.parametrize("mode", ["batched", "knob", "single", "extents"])
def test_driver_main_writes_the_references_files(mode, tmp_path, monkeypatch):
    # "extents": the batched run in a root Domain of 1 x 2 x 1.5 (x2max = 2, x3 = -0.5 .. 1): the deck's own 1 x 1 x 1 cannot tell
    # the x1 extent from the volume, nor the root's x2 / x3 extents from 1
    fx = fixture("g1d_out_sod_24_x2" if mode == "extents" else "g1d_out_sod_24")
    ext3 = (2.0, 1.5) if mode == "extents" else (1.0, 1.0)
    paths = [str(p) for p in fx["paths"]]
    files = {p: fx[f"file_{i}"].tobytes() for i, p in enumerate(paths)}
    cfg = pkg("config"); D = pkg("driver"); O = pkg("outputs"); A = pkg("athinput")
    if mode == "knob":
        monkeypatch.setenv("AA_1D_RESIDENT", "0")
    if mode == "single":
        monkeypatch.setattr(D.Driver, "may_batch", lambda self: False)
    par, blocks = _out_par(fx)
    run = cfg.from_par(par, "shkset1d")
    run.integrator = "ctu-noh"
    full = str(tmp_path / "full")
    d = D.Driver(run, strict=True)
    assert d.may_batch() == (mode != "single")
    calls = []
    adv = d.advance
    monkeypatch.setattr(d, "advance", lambda *a: (calls.append(adv(*a)), calls[-1])[1])
    d.main(O.OutputSet.from_par(par, 0.0, full))
    assert _tree(full) == paths
    if mode != "single":                        # a call per stretch between output times, not one per step
        assert sum(calls) == d.nstep and len(calls) <= 6 < d.nstep
    for rel in paths:
        ours = open(os.path.join(full, rel), "rb").read(); ref = files[rel]
        ext = rel.rsplit(".", 1)[1]
        if ext in ("vtk", "bin"):
            assert ours == ref, rel
            if ext == "vtk":
                assert b"DIMENSIONS 25 1 1\n" in ours and b"SPACING %e %e %e \n" % (1.0 / 24, ext3[0], ext3[1]) in ours
        elif ext == "rst":
            assert _payload(ours) == _payload(ref), rel
            po = A.ParTable.from_text(ours[:ours.index(b"<par_end>")].decode()); pr = A.ParTable.from_text(ref[:ref.index(b"<par_end>")].decode(errors="replace"))
            for n in blocks:
                assert po.geti(f"output{n}", "num") == pr.geti(f"output{n}", "num"), (rel, n)
                assert po.getd(f"output{n}", "time") == pr.getd(f"output{n}", "time"), (rel, n)
            assert po.getd("time", "time") == pr.getd("time", "time") and po.geti("time", "nstep") == pr.geti("time", "nstep")
        else:
            _same_hst(ours, ref, 1.0)
            # (dump_history.c:174-177: a zone's dVol has the root's x2 and x3 extents in it, the divisor :316-321 has not)
            assert float(ours.decode().splitlines()[3].split()[2]) == 0.5625 * ext3[0] * ext3[1]
    if mode != "batched":
        d.eng.close()
        return
    # Driver.from_restart on the middle dump continues to the same final files
    Ufull = d.eng.download(); state = (d.time, d.dt, d.nstep)
    d.eng.close()
    res = str(tmp_path / "resumed")
    r = D.Driver.from_restart(os.path.join(full, "Sod.0001.rst"), problem="shkset1d", integrator="ctu-noh", strict=True)
    assert r.restarted and 0 < r.nstep < state[2] and r.grid.Nx == (24, 1, 1)
    r.main(O.OutputSet.from_par(r.par, r.time, res))
    assert (r.time, r.dt, r.nstep) == state
    assert np.array_equal(r.eng.download(), Ufull)
    last = max(int(p.split(".")[1]) for p in paths if p.endswith(".rst"))
    for ext in ("rst", "vtk", "bin"):
        rel = "Sod.%04d.%s" % (last, ext)
        a, b = open(os.path.join(res, rel), "rb").read(), open(os.path.join(full, rel), "rb").read()
        assert (_payload(a) == _payload(b)) if ext == "rst" else (a == b), rel
    assert open(os.path.join(res, "Sod.hst")).read().splitlines()[-1] == open(os.path.join(full, "Sod.hst")).read().splitlines()[-1]
    with pytest.raises(pkg("restart").RestartError, match="1-D"):
        D.Driver.from_restart(os.path.join(full, "Sod.0001.rst"), problem="shkset1d", integrator="ctu-noh", strict=True, regrid=True)
    r.eng.close()


def test_overlapped_dumps_fall_back_with_one_warning(tmp_path):
    fx = fixture("g1d_out_sod_24")
    cfg = pkg("config"); D = pkg("driver"); O = pkg("outputs")
    par, _ = _out_par(fx)
    run = cfg.from_par(par, "shkset1d"); run.integrator = "ctu-noh"
    d = D.Driver(run, strict=True)
    with pytest.warns(UserWarning) as rec:
        d.main(O.OutputSet.from_par(par, 0.0, str(tmp_path), overlap=True, overlap_rst=True))
    said = [str(w.message) for w in rec if "1-D" in str(w.message)]
    assert len(said) == 2 and any("overlap_rst" in s for s in said), said      # once per switch
    assert _tree(str(tmp_path)) == [str(p) for p in fx["paths"]]
    L = d.eng.g.L
    assert L.aa_dump_snapshot_begin(d.eng.g._h, 0, pkg("dumps").FORMATS["vtk"], 0, 1 << 30) != 0 and b"1-D" in L.aa_last_error()
    assert L.aa_rst_snapshot_begin(d.eng.g._h, 0, 1 << 30) != 0 and b"1-D" in L.aa_last_error()
    d.eng.close()


# ---- 7. the problem generators on 1-D Grids give the reference's step-0 state ---------------------------------------------------
@pytest.mark.parametrize("name", ["g1d_blast_vl_o2_c4_65_s6", "g1d_blast_ctu_o3_c4_1272_s6", "g1d_shk_ctu-noh_bc1_c8_5_s5",
                                  "g1d_shk_ctu-noh_einfeldt1125_128_s10"])
def test_problem_generators_give_the_reference_state(name):
    lib = pkg("lib")
    fx = fixture(name)
    g = lib.setup_problem(onedfix.grid_config(fx), 0, True)
    assert g.host_initial.shape == (1, 1, int(fx["nx"][0]) + 2 * NG, 5)
    assert np.array_equal(g.host_initial[:, :, NG:-NG, :], fx["U0"])
    assert np.array_equal(g.download()[:, :, NG:-NG, :], fx["U0"])
    g.close()


# ---- 8. what is refused on a 1-D Grid, and the entry points of the other dimensions -----------------------------------------------
def test_refusals_set_the_last_error():
    aa = pkg(); lib = pkg("lib")
    run = aa.config.load(os.path.join(onedfix.DECKS, "athinput.blast1d"), ["domain1/Nx1=8", "time/cour_no=0.4"], "blast", "vl")
    g = lib.Grid(aa.config.slab(run), 0, True)
    L = g.L

    def refused(rc, *words):
        msg = L.aa_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)
    refused(L.aa_add_radplane_3d(g._h, -1, 1.0), "1-D")
    refused(L.aa_set_static_grav_pot(g._h, lib.GRAVPOT(lambda x, y, z: 0.0)), "gravity", "1-D")
    t = np.zeros((1, 1, 16))
    refused(L.aa_set_static_grav_tables(g._h, lib._dp(t), lib._dp(t), lib._dp(t), lib._dp(t)), "gravity", "1-D")
    refused(L.aa_set_fofc(g._h, 1), "1-D")
    refused(L.aa_integrate_3d_ctu(g._h), "1-D", "aa_integrate_1d_ctu")
    refused(L.aa_integrate_3d_vl(g._h), "1-D", "aa_integrate_1d_vl")
    refused(L.aa_integrate_2d_ctu(g._h), "1-D", "aa_integrate_1d_ctu")
    refused(L.aa_integrate_2d_vl(g._h), "1-D", "aa_integrate_1d_vl")
    refused(L.aa_integrate_1d_ctu(g._h), "van Leer")
    buf = np.zeros(64)
    refused(L.aa_halo_get(g._h, 2, 0, lib._dp(buf)), "1-D")
    hs = (C.c_void_p * 1)(g._h); disp = (C.c_int * 3)(0, 0, 0); m = C.c_void_p()
    refused(L.aa_mesh_create(1, hs, disp, C.byref(m)), "1-D")
    refused(L.aa_mesh_create_2d(1, hs, disp, C.byref(m)), "1-D")
    links = (C.c_int * 21)()
    refused(L.aa_mesh_create_local(1, hs, links, C.byref(m)), "1-D")
    g.close()
    run = aa.config.load(os.path.join(onedfix.DECKS, "athinput.blast1d"), ["domain1/Nx1=8"], "blast")
    g = lib.Grid(aa.config.slab(run), 0, True)
    refused(L.aa_set_cooling(g._h, 1), "cooling", "1-D")
    refused(L.aa_integrate_1d_vl(g._h), "CTU")
    g.close()
    # the 1-D entry points on Grids of the other dimensions
    for deck, ov, dim in (("athinput.blast", ["domain1/Nx1=8", "domain1/Nx2=8", "domain1/Nx3=8"], "3-D"),
                          ("athinput.blast2d", ["domain1/Nx1=8", "domain1/Nx2=8"], "2-D")):
        gg = lib.Grid(aa.config.slab(aa.config.load(os.path.join(onedfix.DECKS, deck), ov, "blast")), 0, True)
        refused(L.aa_integrate_1d_ctu(gg._h), dim)
        refused(L.aa_integrate_1d_vl(gg._h), dim)
        n = C.c_int()
        refused(L.aa_run_1d(gg._h, 1.0, 1.0, 1, C.byref(n)), dim)
        gg.close()
    # aa_create
    p = lib.params_from_grid(aa.config.slab(run))
    h = C.c_void_p()
    p.integrator = 1                            # the deck's cour_no 0.8
    refused(L.aa_create(C.byref(p), C.byref(h)), "must be <= 0.5 with 1D VL integrator")
    p.integrator = 0; p.ion = 1; p.nscal = 1
    refused(L.aa_create(C.byref(p), C.byref(h)), "ion radiation", "1-D")
    p.ion = 0
    refused(L.aa_create(C.byref(p), C.byref(h)), "scalars", "1-D")
    p.nscal = 0; p.nslab = 2
    refused(L.aa_create(C.byref(p), C.byref(h)), "slabs", "1-D")
    p.nslab = 1; p.level = 1
    refused(L.aa_create(C.byref(p), C.byref(h)), "1-D")
    p.level = 0; p.rootNx[1] = 8                # a one-row cut of a 2-D root Domain
    refused(L.aa_create(C.byref(p), C.byref(h)), "1-D", "8 x 8 x 1")
    p.rootNx[1] = 1
    cuts = (C.c_int * 2)(0, 1)
    refused(L.aa_create_cut(C.byref(p), 0, 1, cuts, C.byref(h)), "1-D")
    for order in (2, 3):                        # ... and both orders, any cour_no with the CTU integrator, integrators 0 and 2
        for integ in (0, 2):
            p.order = order; p.integrator = integ; p.cour_no = 0.95
            assert L.aa_create(C.byref(p), C.byref(h)) == 0, L.aa_last_error()
            L.aa_destroy(h)


def test_nslab_from_the_environment_is_refused(monkeypatch):
    aa = pkg(); lib = pkg("lib")
    run = aa.config.load(os.path.join(onedfix.DECKS, "athinput.blast1d"), ["domain1/Nx1=8"], "blast")
    p = lib.params_from_grid(aa.config.slab(run)); p.nslab = 0
    h = C.c_void_p(); L = lib.load(True)
    monkeypatch.setenv("AA_NGPU", "2")
    assert L.aa_create(C.byref(p), C.byref(h)) != 0 and b"1-D" in L.aa_last_error()


def test_driver_steps_singly_once_zones_are_pinned(tmp_path, monkeypatch):
    """aa_run_1d refuses a Grid with pinned zones, so Driver.may_batch says no and outputs.run takes single steps: the same run
    as the single-step Driver, and the pinned zone holds its values"""
    fx = fixture("g1d_out_sod_24")
    cfg = pkg("config"); D = pkg("driver"); O = pkg("outputs")
    par, _ = _out_par(fx)
    pin = (np.array([NG + 3]), np.array([[1.0, 0.0, 0.0, 0.0, 2.5]]))
    out = []
    for k, single in enumerate((False, True)):
        run = cfg.from_par(par, "shkset1d"); run.integrator = "ctu-noh"
        d = D.Driver(run, strict=True)
        assert d.may_batch()
        d.eng.g.set_pinned_cells(*pin)
        assert not d.may_batch() and not d.eng.g.can_run_until()
        if single:
            monkeypatch.setattr(D.Driver, "may_batch", lambda self: False)
        monkeypatch.setattr(d, "advance", lambda *a: pytest.fail("advance() on a Grid with pinned zones"))
        d.main(O.OutputSet.from_par(par, 0.0, str(tmp_path / str(k))))
        U = d.eng.download()
        assert d.time == run.tlim and d.nstep > 6 and np.array_equal(U[0, 0, NG + 3], pin[1][0])
        out.append((U, d.time, d.dt, d.nstep))
        d.eng.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1:] == out[1][1:]


def test_fewer_zones_than_ghost_zones_are_refused():
    aa = pkg(); lib = pkg("lib")
    run = aa.config.load(os.path.join(onedfix.DECKS, "athinput.sod1d"), ["domain1/Nx1=4"], "shkset1d")
    p = lib.params_from_grid(aa.config.slab(run))
    h = C.c_void_p(); L = lib.load(True)
    for n in (2, 3):
        p.Nx[0] = p.rootNx[0] = n
        assert L.aa_create(C.byref(p), C.byref(h)) != 0
        msg = L.aa_last_error().decode()
        assert "1-D" in msg and f"of {n} zones" in msg and "ghost zones" in msg, msg
    p.Nx[0] = p.rootNx[0] = 4
    assert L.aa_create(C.byref(p), C.byref(h)) == 0, L.aa_last_error()
    L.aa_destroy(h)
