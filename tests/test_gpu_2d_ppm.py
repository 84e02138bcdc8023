"""Third-order reconstruction on 2-D Grids (Nx3 = 1) on an MI355X: aa_set_order_2d and the ORD = 3 instantiations of
csrc/hydro2d_kernels.hip (k2d_edge_wl, k2d_first; the VL2 forms of k2d_edge and k2d_step; their *_dc entry points).

The reference is the set of restart states and output files the unmodified third-order reference executables (blast_ppm: CTU +
H-correction; blast_vl_ppm: van Leer) left on decks with Nx3 = 1 (tests/golden/g2dppm_*.npz, tests/golden/make_golden_2d_ppm.py).
The strict library reproduces them bit for bit.  The default library is held to the bars the tree uses for third-order fixtures:
the 3-D third-order cases of test_gpu_parity.py hold the fields to 1e-11 of each field's maximum and set no bar on dt; the 2-D bars
(test_gpu_2d.py) are the same 1e-11 and 1e-12 in dt.  The field bars agree; the 2-D bar on dt is kept (the 3-D cases have none to
compare it with)."""
import ctypes as C
import glob
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
FAR = 1.0e300                       # a t_stop no run reaches: the step count ends the call
TOL_U, TOL_DT = 1e-11, 1e-12
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(twodfix.GOLDEN, "g2dppm_blast_*.npz")) +
                  glob.glob(os.path.join(twodfix.GOLDEN, "g2dppm_vel_*.npz")))


def relerr(a, b):
    """max |a-b| / max|b| per variable; a variable that vanishes identically in the reference must vanish here too"""
    out = []
    for c in range(a.shape[-1]):
        scale = np.abs(b[..., c]).max()
        diff = float(np.abs(a[..., c] - b[..., c]).max())
        out.append(diff / scale if scale > 0 else (0.0 if diff == 0.0 else np.inf))
    return out


def started(fx, strict, order=3):
    """a Grid with the fixture's step-0 state at the given order (None: the setter is never called), started as the reference was:
    aa_start on a fresh run, aa_resume with the seed's dt where the reference was seeded through a restart file"""
    lib = pkg("lib")
    gc = twodfix.grid_config(fx)
    g = lib.Grid(gc, 0, strict)
    if order is not None:
        g.set_order_2d(order)
        assert g.order == order
    g.upload(twodfix.host_block(gc, fx["U0"]))
    if "seeded" in fx:
        g.set_mesh_state(0.0, float(fx["dt0"]), 0)
        g.resume()
    else:
        g.start()
    return g


def state(g):
    return (g.time, g.dt, g.nstep), g.download()


_per_step = {}


def per_step(name, strict):
    """(dt0, (time, dt, nstep), whole block) of the fixture's steps through aa_set_order_2d + aa_step; run once and shared"""
    key = (name, strict)
    if key not in _per_step:
        fx = fixture(name)
        g = started(fx, strict)
        dt0 = g.dt
        for _ in range(int(fx["nstep"])):
            g.step()
        s = state(g)
        g.close()
        s[1].setflags(write=False)
        _per_step[key] = (dt0,) + s
    return _per_step[key]


# ---- 1. every fixture through aa_set_order_2d + aa_step ---------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", FIXTURES)
def test_steps_reproduce_the_third_order_reference(name, strict):
    fx = fixture(name)
    dt0, (time, dt, nstep), U = per_step(name, strict)
    Ua = U[:, NG:-NG, NG:-NG, :]
    err = relerr(Ua, fx["U"])
    print(f"{name} strict={strict}: relerr {err} dt0 {dt0!r} / {float(fx['dt0'])!r} dt {dt!r} / {float(fx['dt'])!r} time {time!r} / {float(fx['time'])!r}")
    assert nstep == int(fx["nstep"])
    if strict:
        assert dt0 == float(fx["dt0"])
        assert np.array_equal(Ua, fx["U"]), err
        assert time == float(fx["time"]) and dt == float(fx["dt"])
    else:
        assert max(err) < TOL_U, err
        assert abs(dt / float(fx["dt"]) - 1) < TOL_DT and abs(dt0 / float(fx["dt0"]) - 1) < TOL_DT


# ---- 2. the same fixtures through aa_run_2d, two queued steps behind the stop -----------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", FIXTURES)
def test_run_2d_gives_the_per_step_bits(name, strict, monkeypatch):
    """one batch of nstep + 2 queued steps: the last two stand behind the stop and must store nothing -- the whole block, ghost
    zones included, and (time, dt, nstep) are the bits of the aa_step loop in both builds"""
    fx = fixture(name)
    n = int(fx["nstep"])
    monkeypatch.setenv("AA_2D_BATCH", str(n + 2))
    g = started(fx, strict)
    assert g.can_run_2d() and g.run_2d_batch() == n + 2 and g.order == 3
    assert g.run_2d(FAR, nstep_stop=n) == n
    s = state(g)
    g.close()
    _, want, U = per_step(name, strict)
    print(f"{name} strict={strict}: run_2d {s[0]!r} per step {want!r}")
    assert s[0] == want
    assert np.array_equal(s[1], U), relerr(s[1], U)


# ---- 3. the fixtures are the cases the kernels' tiles ask for ----------------------------------------------------------------------
def test_every_integrator_and_tile_case_has_a_third_order_fixture():
    sizes = ("4x4", "5x7", "63x6", "64x7", "65x8", "130x9", "67x35")       # R = T2_R - 1 = 7: 64 x R, 65 x (R + 1)
    for tag in ("ctu_c4", "ctu_c8", "vl_c4"):
        for size in sizes:
            hits = [n for n in FIXTURES if n.startswith(f"g2dppm_blast_{tag}_{size}_s")]
            assert len(hits) == 1 and 4 <= int(hits[0].rsplit("_s", 1)[1]) <= 6, (tag, size, hits)
    for integ in ("ctu", "vl"):
        for case in ("d1_48x8", "d2_8x48", "d1_67x9"):
            assert f"g2dppm_vel_{integ}_{case}_s8" in FIXTURES
    assert len(FIXTURES) == 27
    # the seeded states carry all three velocity components, different on the two sides, and the reference kept them all
    for n in FIXTURES:
        fx = fixture(n)
        if n.startswith("g2dppm_vel_"):
            assert int(fx["seeded"]) == 1 and all(np.abs(fx[k][..., c]).min() > 0 for k in ("U0", "U") for c in (1, 2, 3))
            assert sorted(int(b) for b in fx["bc"][:4]) == [2, 2, 4, 4]
        assert np.all(np.isfinite(fx["U"])) and int(fx["nx"][2]) == 1


# ---- 4. the setter: what it refuses, and that order 2 through it is the run without it ---------------------------------------------
def test_the_setter_refuses_by_message():
    aa = pkg(); lib = pkg("lib")
    L = lib.load(True)

    def refused(rc, *words):
        msg = L.aa_last_error().decode()
        assert rc != 0 and msg.startswith("[aa_set_order_2d]") and all(w in msg for w in words), (rc, msg)

    def grid(deck, ov, integ="ctu", prob="blast"):
        return lib.Grid(aa.config.slab(aa.config.load(os.path.join(twodfix.DECKS, deck), ov, prob, integ)), 0, True)
    small = ["domain1/Nx1=8", "domain1/Nx2=8"]
    g = grid("athinput.blast2d", small)
    assert g.order == 2
    refused(L.aa_set_order_2d(g._h, 1), "order 1")
    refused(L.aa_set_order_2d(g._h, 4), "order 4")
    assert L.aa_set_order_2d(g._h, 3) == 0 and g.order == 3 and L.aa_set_order_2d(g._h, 2) == 0 and g.order == 2
    g.set_order_2d(3)
    U = g.new_host_block(); U[..., 0] = 1.0; U[..., 4] = 1.0
    g.upload(U); g.start(); g.step()
    refused(L.aa_set_order_2d(g._h, 2), "already stepped")
    assert g.order == 3
    with pytest.raises(lib.AthenaError, match="already stepped"):
        g.set_order_2d(2)
    g.close()
    # CTU without H-correction: no third-order reference build
    g = grid("athinput.blast2d", small, "ctu-noh")
    refused(L.aa_set_order_2d(g._h, 3), "integrator = 2", "H-correction")
    assert L.aa_set_order_2d(g._h, 2) == 0 and g.order == 2
    g.close()
    # 1-D and 3-D Grids take aa_params.order
    g1 = grid("athinput.blast1d", ["domain1/Nx1=16"])
    refused(L.aa_set_order_2d(g1._h, 3), "1-D", "aa_params.order")
    g1.close()
    g3 = grid("athinput.blast", ["domain1/Nx1=8", "domain1/Nx2=8", "domain1/Nx3=8"])
    refused(L.aa_set_order_2d(g3._h, 3), "3-D", "aa_params.order")
    assert g3.order == 2
    g3.close()
    # (a Grid that belongs to a Mesh: test_gpu_2d_smr_ppm.py)
    # aa_params.order = 3 on a 2-D Grid stays refused with its message, and lib.Grid hands a run's order_2d to the setter
    p = lib.params_from_grid(aa.config.slab(aa.config.load(os.path.join(twodfix.DECKS, "athinput.blast2d"), small, "blast")))
    p.order = 3
    h = C.c_void_p()
    assert L.aa_create(C.byref(p), C.byref(h)) != 0 and "no reference target pins it" in L.aa_last_error().decode()
    run = aa.config.load(os.path.join(twodfix.DECKS, "athinput.blast2d"), small, "blast", order_2d=3)
    g = lib.Grid(aa.config.slab(run), 0, True)
    assert g.order == 3 and g.params.order == 2
    g.close()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", ["g2d_blast_ctu_c8_67x35_s4", "g2d_blast_vl_c4_65x8_s6"])
def test_order_2_through_the_setter_is_the_run_without_it(name, strict):
    """... and the second-order fixtures still hold behind the setter at 2; at 3 the same start leaves other bits (the switch acts)"""
    fx = fixture(name)
    out = []
    for order in (None, 2, 3):
        g = started(fx, strict, order)
        for _ in range(int(fx["nstep"])):
            g.step()
        out.append(state(g))
        g.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
    if strict:
        assert np.array_equal(out[1][1][:, NG:-NG, NG:-NG, :], fx["U"]) and out[1][0][1] == float(fx["dt"])
    assert not np.array_equal(out[0][1], out[2][1])


# ---- 5. Driver.main at third order on the 2-D deck with hst + bin + vtk + rst blocks; resumed from the middle dump ------------------
def _out_par(fx):
    blocks = json.loads(str(fx["blocks"]))
    ov = [str(o) for o in fx["overrides"]] + [f"job/maxout={max(int(n) for n in blocks)}"]
    for n, kv in blocks.items():
        ov += [f"output{n}/{k}={v}" for k, v in kv.items()]
    return pkg("athinput").ParTable.from_file(os.path.join(twodfix.DECKS, "athinput.blast2d")).cmdline(ov), blocks


def _payload(b):
    return b[b.index(b"<par_end>\n") + len(b"<par_end>\n"):]


def test_driver_main_writes_the_third_order_references_files_and_resumes(tmp_path):
    """The comparison of test_gpu_2d.py's output test on the tree blast_ppm left: vtk and bin byte for byte, rst everything behind the
    parameter dump byte for byte and every block's num / time in it, hst the header and every column as printed -- except the net
    momenta, rounding noise of the summation order in this symmetric run (held to 1e-9 of the mass, the rule of test_history.py).
    Then Driver.from_restart(..., order_2d=3) from the middle dump writes the later files again; without the keyword it does not."""
    import dumpfix
    fx = fixture("g2dppm_out_blast_24x20")
    paths = [str(p) for p in fx["paths"]]
    files = {p: fx[f"file_{i}"].tobytes() for i, p in enumerate(paths)}
    cfg = pkg("config"); D = pkg("driver"); O = pkg("outputs"); A = pkg("athinput")
    par, blocks = _out_par(fx)
    run = cfg.from_par(par, "blast")
    run.order_2d = 3
    full = str(tmp_path / "full")
    d = D.Driver(run, strict=True)
    assert d.eng.g.order == 3
    d.main(O.OutputSet.from_par(par, 0.0, full))
    got = sorted(os.path.relpath(os.path.join(dp, f), full) for dp, _, fs in os.walk(full) for f in fs)
    assert got == paths, (got, paths)
    nx = (int(fx["nx"][0]), int(fx["nx"][1]), 1)
    for rel in paths:
        ours = open(os.path.join(full, rel), "rb").read(); ref = files[rel]
        ext = rel.rsplit(".", 1)[1]
        if ext in ("vtk", "bin"):
            n = {"bin": "2", "vtk": "3"}[ext]
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
            assert lo[:3] == lr[:3] and len(lo) == len(lr)
            for a, b in zip(lo[3:], lr[3:]):
                ca, cb = a.split(), b.split()
                assert ca[:4] == cb[:4] and ca[7:] == cb[7:], (a, b)
                assert all(abs(float(x) - float(y)) <= 1e-9 * float(cb[2]) for x, y in zip(ca[4:7], cb[4:7])), (a, b)
    Ufull = d.eng.download(); final = (d.time, d.dt, d.nstep)
    d.eng.close()
    res = str(tmp_path / "resumed")
    r = D.Driver.from_restart(os.path.join(full, "Blast.0001.rst"), strict=True, order_2d=3)
    assert r.restarted and 0 < r.nstep < final[2] and r.grid.Nx == nx and r.eng.g.order == 3
    r.main(O.OutputSet.from_par(r.par, r.time, res))
    assert (r.time, r.dt, r.nstep) == final
    assert np.array_equal(r.eng.download(), Ufull)
    later = [p for p in paths if p.endswith(".rst") and p > "Blast.0001.rst"]
    assert later
    for rel in later:                                   # the later restart dumps, against the REFERENCE's own
        assert _payload(open(os.path.join(res, rel), "rb").read()) == _payload(files[rel]), rel
    last_bin, last_vtk = sorted(p for p in paths if p.endswith(".bin"))[-1], sorted(p for p in paths if p.endswith(".vtk"))[-1]
    res_bin, res_vtk = sorted(f for f in os.listdir(res) if f.endswith(".bin"))[-1], sorted(f for f in os.listdir(res) if f.endswith(".vtk"))[-1]
    assert dumpfix.compare_dump(open(os.path.join(res, res_bin), "rb").read(), files[last_bin], nx, 0, "bin", False, res_bin) == 0
    assert dumpfix.compare_dump(open(os.path.join(res, res_vtk), "rb").read(), files[last_vtk], nx, 0, "vtk", True, res_vtk) == 0
    r.eng.close()
    # the order is not in the file: resumed without the keyword the run is a second-order one and ends elsewhere
    r2 = D.Driver.from_restart(os.path.join(full, "Blast.0001.rst"), strict=True)
    assert r2.eng.g.order == 2
    r2.main(O.OutputSet.from_par(r2.par, r2.time, str(tmp_path / "second")))
    assert not np.array_equal(r2.eng.download(), Ufull)
    r2.eng.close()
