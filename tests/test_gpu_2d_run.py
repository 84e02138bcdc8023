"""aa_run_2d / Grid.run_2d on an MI355X: many steps of a 2-D Grid per host visit, the time step picked on the device
(csrc/hydro2d_kernels.hip k2d_advance and the *_dc entry points of the step chain; csrc/api2d.hip).

Two references.  The restart states the unmodified reference executables left (tests/golden/g2d_*.npz): the strict library
reproduces them bit for bit, the default library within the bars of test_gpu_2d.py (1e-11 of each field's maximum, 1e-12 in
dt).  And the per-step path (Grid.step) of the same library: run_2d gives its bits in BOTH libraries -- the whole block, ghost
zones included, and (time, dt, nstep) -- because the queued kernels run the same code on the same operands."""
import ctypes as C
import json
import math
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
# CTU with H-correction across two x1 tiles and five row blocks; van Leer one zone above the tile; CTU without H-correction on
# three tiles; a reflecting shock tube along x2
STOP_CASES = ["g2d_blast_ctu_c4_67x35_s5", "g2d_blast_vl_c4_65x8_s6", "g2d_blast_ctu-noh_c8_130x9_s6", "g2d_shk_ctu_d2_refl_8x48_s12"]
NTRAJ = 9


def relerr(a, b):
    out = []
    for c in range(a.shape[-1]):
        scale = np.abs(b[..., c]).max()
        diff = float(np.abs(a[..., c] - b[..., c]).max())
        out.append(diff / scale if scale > 0 else (0.0 if diff == 0.0 else np.inf))
    return out


def started(fx, strict, extra=()):
    lib = pkg("lib")
    gc = twodfix.grid_config(fx, extra)
    g = lib.Grid(gc, 0, strict)
    g.upload(twodfix.host_block(gc, fx["U0"]))
    g.start()
    return g


def state(g):
    return (g.time, g.dt, g.nstep), g.download()


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


_traj = {}


def trajectory(name, strict, extra=()):
    """the per-step path: [(time, dt, nstep), whole block] after 0 .. NTRAJ calls of step(); run once and shared"""
    key = (name, strict, tuple(extra))
    if key not in _traj:
        g = started(fixture(name), strict, extra)
        out = [state(g)]
        for _ in range(NTRAJ):
            g.step()
            out.append(state(g))
        g.close()
        for _, U in out:
            U.setflags(write=False)
        _traj[key] = out
    return _traj[key]


# ---- 1. every fixture: the reference's states, and the per-step path's bits ------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", twodfix.STEP_FIXTURES)
def test_run_2d_reproduces_the_reference_and_the_per_step_path(name, strict, monkeypatch):
    monkeypatch.setenv("AA_2D_BATCH", "8")      # (the fixtures are 4 .. 12 steps: calls of one batch with steps behind the stop, and of two)
    fx = fixture(name)
    n = int(fx["nstep"])
    g = started(fx, strict)
    assert g.can_run_2d() and g.run_2d_batch() == 8
    dt0 = g.dt
    assert g.run_2d(FAR, nstep_stop=n) == n
    s = state(g)
    g.close()
    h = started(fx, strict)
    for _ in range(n):
        h.step()
    per_step = state(h)
    h.close()
    Ua = s[1][:, NG:-NG, NG:-NG, :]
    err = relerr(Ua, fx["U"])
    print(f"{name} strict={strict}: relerr {err} state {s[0]!r} per step {per_step[0]!r} fixture ({float(fx['time'])!r}, {float(fx['dt'])!r})")
    assert s[0][2] == n
    if strict:
        assert dt0 == float(fx["dt0"])
        assert np.array_equal(Ua, fx["U"]), err
        assert s[0][0] == float(fx["time"]) and s[0][1] == float(fx["dt"])
    else:
        assert max(err) < 1e-11, err
        assert abs(s[0][1] / float(fx["dt"]) - 1) < 1e-12
    assert s[0] == per_step[0]
    assert np.array_equal(s[1], per_step[1]), relerr(s[1], per_step[1])


# ---- 2. the stop rules against the per-step path, four steps queued per read-back -------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", STOP_CASES)
def test_stop_rules_leave_the_per_step_paths_state(name, strict, monkeypatch):
    """nstep_stop one below, on and one above a batch of 4 and inside the third; a t_stop inside the second batch; t_stop at the
    Grid's own time.  The whole block is compared, so a step queued behind the stop that stored anything would show."""
    monkeypatch.setenv("AA_2D_BATCH", "4")
    fx = fixture(name)
    tr = trajectory(name, strict)
    for n in (1, 3, 4, 5, 9):
        g = started(fx, strict)
        assert g.run_2d_batch() == 4
        assert g.run_2d(FAR, nstep_stop=n) == n
        s = state(g)
        print(f"{name} strict={strict} nstep_stop={n}: {s[0]!r} / {tr[n][0]!r}")
        assert same(s, tr[n]), (n, s[0], tr[n][0])
        # ... and called again at the stop it takes no step and touches nothing
        g.host_syncs(True)
        assert g.run_2d(FAR, nstep_stop=n) == 0 and g.host_syncs() == 0
        assert same(state(g), tr[n])
        g.close()
    (t5, dt5, _), _ = tr[5]
    g = started(fx, strict)
    assert g.run_2d(t5 + 0.5 * dt5) == 6              # time >= t_stop first holds after the sixth step
    assert same(state(g), tr[6])
    assert g.run_2d(g.time) == 0 and g.run_2d(0.0) == 0 and same(state(g), tr[6])
    g.close()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", STOP_CASES[:2])
def test_the_last_dt_is_clipped_at_tlim(name, strict, monkeypatch):
    monkeypatch.setenv("AA_2D_BATCH", "4")
    fx = fixture(name)
    (t6, dt6, _), _ = trajectory(name, strict)[6]
    tlim = t6 + 0.5 * dt6
    extra = [f"time/tlim={tlim!r}"]
    h = started(fx, strict, extra)
    dts = []
    while h.time < tlim:
        dts.append(h.dt)
        h.step()
    per_step = state(h)
    h.close()
    assert len(dts) == 7 and dts[6] == tlim - t6 < dt6 and per_step[0][0] == tlim
    g = started(fx, strict, extra)
    assert g.cfg.run.tlim == tlim
    assert g.run_2d(tlim) == 7
    s = state(g)
    print(f"{name} strict={strict}: {s[0]!r} / {per_step[0]!r}")
    assert same(s, per_step)
    g.close()


# ---- 3. mixed with step(), and on a resumed Grid -------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", STOP_CASES[:3])
def test_run_2d_mixes_with_single_steps_and_follows_a_resume(name, strict, monkeypatch):
    monkeypatch.setenv("AA_2D_BATCH", "4")
    fx = fixture(name)
    tr = trajectory(name, strict)
    g = started(fx, strict)
    assert g.run_2d(FAR, nstep_stop=3) == 3
    g.step(); g.step()
    assert same(state(g), tr[5])
    assert g.run_2d(FAR, nstep_stop=9) == 4
    assert same(state(g), tr[9])
    g.close()
    # a Grid that takes the state after four steps as a restarted run does (aa_resume: the ghost zones, no new_dt)
    lib = pkg("lib")
    r = lib.Grid(twodfix.grid_config(fx), 0, strict)
    (t4, dt4, n4), U4 = tr[4]
    blk = np.zeros_like(U4)
    blk[:, NG:-NG, NG:-NG, :] = U4[:, NG:-NG, NG:-NG, :]
    r.upload(blk)
    r.set_mesh_state(t4, dt4, n4)
    r.resume()
    assert r.run_2d(FAR, nstep_stop=9) == 5
    assert same(state(r), tr[9])
    r.close()


# ---- 4. the point of it: read-backs per call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_a_call_reads_back_once_per_batch(strict, monkeypatch):
    fx = fixture("g2d_blast_ctu_c4_67x35_s5")
    out = {}
    for k in ("4", "0"):
        monkeypatch.setenv("AA_2D_BATCH", k)
        g = started(fx, strict)
        assert g.run_2d_batch() == int(k)
        g.host_syncs(True)
        assert g.run_2d(FAR, nstep_stop=12) == 12
        out[k] = (g.host_syncs(), state(g))
        g.close()
    print(f"strict={strict}: host_syncs {out['4'][0]} with AA_2D_BATCH=4, {out['0'][0]} with AA_2D_BATCH=0")
    assert out["4"][0] <= 4
    assert out["0"][0] >= 12
    assert same(out["4"][1], out["0"][1])
    monkeypatch.setenv("AA_2D_BATCH", "-1")
    lib = pkg("lib")
    with pytest.raises(lib.AthenaError, match="AA_2D_BATCH"):
        lib.Grid(twodfix.grid_config(fx), 0, strict)


# ---- 5. what aa_run_2d refuses --------------------------------------------------------------------------------------------------------
def test_refusals_set_the_last_error():
    aa = pkg(); lib = pkg("lib"); cfg = pkg("config")
    L = lib.load(True)
    n = C.c_int()

    def refused(rc, *words):
        msg = L.aa_last_error().decode()
        assert rc != 0 and msg.startswith("[aa_run_2d]") and all(w in msg for w in words), (rc, msg)
    run1 = cfg.load(os.path.join(twodfix.DECKS, "athinput.blast1d"), ["domain1/Nx1=8"], "blast")
    g1 = lib.Grid(cfg.slab(run1), 0, True)
    refused(L.aa_run_2d(g1._h, 1.0, run1.tlim, 1, C.byref(n)), "1-D")
    assert not g1.can_run_2d() and g1.run_2d_batch() == 0
    g1.close()
    run3 = cfg.load(os.path.join(twodfix.DECKS, "athinput.blast"), ["domain1/Nx1=8", "domain1/Nx2=8", "domain1/Nx3=8"], "blast")
    g3 = lib.Grid(cfg.slab(run3), 0, True)
    refused(L.aa_run_2d(g3._h, 1.0, run3.tlim, 1, C.byref(n)), "3-D")
    assert not g3.can_run_2d()
    g3.close()
    fx = fixture("g2d_blast_ctu_c4_5x7_s5")
    g = started(fx, True)
    tlim = g.cfg.run.tlim
    with pytest.raises(lib.AthenaError, match="tlim"):
        g.run_2d(tlim, tlim=2.0 * tlim)
    with pytest.raises(lib.AthenaError, match="2\\^20"):
        g.run_2d(tlim, nstep_stop=(1 << 20) + 1)
    with pytest.raises(lib.AthenaError, match="2\\^20"):
        g.run_2d(tlim, nstep_stop=-1)
    with pytest.raises(lib.AthenaError, match="2-D"):
        g.run_until(tlim)                           # the 1-D call still refuses a 2-D Grid
    assert g.can_run_2d() and not g.can_run_until()
    m = (NG + 2) * g.N[0] + NG + 1
    pin = np.array([[1.0, 0.0, 0.0, 0.0, 2.5]])
    g.set_pinned_cells(np.array([m]), pin)
    assert not g.can_run_2d()
    refused(L.aa_run_2d(g._h, tlim, tlim, 3, C.byref(n)), "pinned")
    assert g.nstep == 0
    g.step()                                        # ... and the per-step path takes them
    assert g.nstep == 1 and np.array_equal(g.download()[0, NG + 2, NG + 1], pin[0])
    g.close()
    # a level of a Mesh
    deck = os.path.join(twodfix.DECKS, "athinput.blast2d_smr")
    sfx = fixture("g2dsmr_A_ctu_s8")
    ov = [str(o) for o in sfx["overrides"]]
    par = aa.athinput.ParTable.from_file(deck).cmdline(ov)
    runm = cfg.load(deck, ov, "blast", "ctu")
    mesh = lib.Mesh(cfg.levels_2d(par, runm), 0, True)
    try:
        for lev in mesh.lev:
            assert not lev.can_run_2d()
            refused(L.aa_run_2d(lev._h, 1.0, runm.tlim, 1, C.byref(n)), "Mesh")
    finally:
        mesh.close()


# ---- 6. Driver.main on the 2-D deck with hst + bin + vtk + rst blocks: batched, by the knob, overlapped -----------------------------
def _tree(d):
    return sorted(os.path.relpath(os.path.join(dp, f), d) for dp, _, fs in os.walk(d) for f in fs)


def _payload(b):
    return b[b.index(b"<par_end>\n") + len(b"<par_end>\n"):]


def _driver_run(fx, mode, out, monkeypatch, extra=()):
    cfg = pkg("config"); D = pkg("driver"); O = pkg("outputs"); A = pkg("athinput")
    monkeypatch.setenv("AA_2D_BATCH", "0" if mode == "knob" else "4")
    blocks = json.loads(str(fx["blocks"]))
    ov = [str(o) for o in fx["overrides"]] + [f"job/maxout={max(int(n) for n in blocks)}"]
    for n, kv in blocks.items():
        ov += [f"output{n}/{k}={v}" for k, v in kv.items()]
    ov += list(extra)
    par = A.ParTable.from_file(os.path.join(twodfix.DECKS, "athinput.blast2d")).cmdline(ov)
    d = D.Driver(cfg.from_par(par, "blast"), strict=True)
    assert d.may_batch() == (mode != "knob")
    calls = []
    adv = d.advance
    monkeypatch.setattr(d, "advance", lambda *a: (calls.append(adv(*a)), calls[-1])[1])
    d.eng.host_syncs(True)
    d.main(O.OutputSet.from_par(par, 0.0, out, overlap=(mode == "overlap")))
    res = dict(syncs=d.eng.host_syncs(), nstep=d.nstep, trace=list(d.niter_trace), calls=calls, state=(d.time, d.dt, d.nstep),
               U=d.eng.download(), blocks=blocks, par=par)
    d.eng.close()
    return res


def test_driver_main_batches_a_2d_run_and_writes_the_same_files(tmp_path, monkeypatch):
    """The three trees are the same byte for byte, every file (hst and the whole rst included).  Against the fixture: vtk and bin
    byte for byte; rst everything behind the parameter dump (the dump is this project's table, not the reference's); hst as
    test_gpu_2d.py holds it -- every column as printed except the net momenta, which in this symmetric run are the rounding
    noise of the order in which the reference adds the zones up.

    Read-backs: the fixture's run is THREE steps, one per stretch between two output times (its hst rows: t = 0.0082, 0.0159,
    0.02), so a call of advance() covers one step and costs the one read-back that step costs anyway: 3 against 3, "fewer" cannot
    hold there, and the run is held to "no more".  "Fewer" is asserted on the same deck and output blocks at 67 x 35 zones and
    cour_no 0.4, where a stretch is several steps -- with the same byte-for-byte comparison of the trees."""
    fx = fixture("g2d_out_blast_24x20")
    paths = [str(p) for p in fx["paths"]]
    files = {p: fx[f"file_{i}"].tobytes() for i, p in enumerate(paths)}
    res = {m: _driver_run(fx, m, str(tmp_path / m), monkeypatch) for m in ("batched", "knob", "overlap")}
    for m, r in res.items():
        print(f"{m}: {r['nstep']} steps, host_syncs {r['syncs']}, advance() -> {r['calls']}")
        assert _tree(str(tmp_path / m)) == paths
        assert len(r["trace"]) == r["nstep"] and r["state"] == res["knob"]["state"] and np.array_equal(r["U"], res["knob"]["U"])
        for rel in paths:
            assert open(os.path.join(tmp_path / m, rel), "rb").read() == open(os.path.join(tmp_path / "knob", rel), "rb").read(), (m, rel)
    assert res["knob"]["calls"] == []
    for m in ("batched", "overlap"):      # a call per stretch between two output times (a pass with an output overdue takes a single step)
        assert 0 < sum(res[m]["calls"]) <= res[m]["nstep"] and len(res[m]["calls"]) <= 4
        assert res[m]["syncs"] <= res["knob"]["syncs"]
    for rel in paths:
        ours = open(os.path.join(tmp_path / "batched", rel), "rb").read(); ref = files[rel]
        ext = rel.rsplit(".", 1)[1]
        if ext in ("vtk", "bin"):
            assert ours == ref, rel
        elif ext == "rst":
            assert _payload(ours) == _payload(ref), rel
        else:
            lo, lr = ours.decode().splitlines(), ref.decode().splitlines()
            assert lo[:3] == lr[:3] and len(lo) == len(lr) == 7
            for a, b in zip(lo[3:], lr[3:]):
                ca, cb = a.split(), b.split()
                assert ca[:4] == cb[:4] and ca[7:] == cb[7:], (a, b)
                assert all(abs(float(x) - float(y)) <= 1e-9 * float(cb[2]) for x, y in zip(ca[4:7], cb[4:7])), (a, b)
    assert math.isfinite(res["batched"]["state"][0])


def test_driver_main_reads_back_less_often_when_it_batches(tmp_path, monkeypatch):
    """the deck and the output blocks of the run above at 67 x 35 zones and cour_no 0.4: several steps per stretch"""
    fx = fixture("g2d_out_blast_24x20")
    extra = ["domain1/Nx1=67", "domain1/Nx2=35", "time/cour_no=0.4"]
    res = {m: _driver_run(fx, m, str(tmp_path / m), monkeypatch, extra) for m in ("batched", "knob", "overlap")}
    paths = _tree(str(tmp_path / "knob"))
    assert {p.rsplit(".", 1)[1] for p in paths} == {"hst", "bin", "vtk", "rst"}
    for m, r in res.items():
        print(f"{m}: {r['nstep']} steps, host_syncs {r['syncs']}, advance() -> {r['calls']}")
        assert _tree(str(tmp_path / m)) == paths
        assert len(r["trace"]) == r["nstep"] and r["state"] == res["knob"]["state"] and np.array_equal(r["U"], res["knob"]["U"])
        for rel in paths:
            assert open(os.path.join(tmp_path / m, rel), "rb").read() == open(os.path.join(tmp_path / "knob", rel), "rb").read(), (m, rel)
    assert res["knob"]["nstep"] >= 12 and res["knob"]["syncs"] >= res["knob"]["nstep"]
    for m in ("batched", "overlap"):
        single = res[m]["nstep"] - sum(res[m]["calls"])      # (a pass with an output overdue takes a single step)
        assert 0 <= single <= 4 and len(res[m]["calls"]) <= 4
        assert res[m]["syncs"] < res["knob"]["syncs"]
        # new_dt of the start, one per single step, ceil(steps / K) + 1 per call at the most
        assert res[m]["syncs"] <= 1 + single + sum(-(-n // 4) + 1 for n in res[m]["calls"])
