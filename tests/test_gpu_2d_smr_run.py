"""aa_mesh_run_2d / Mesh.run_2d on an MI355X: many steps of a refined 2-D mesh per host visit, ONE clock in device memory for all
levels (csrc/smr.hip mesh_queue_step_2d; csrc/hydro2d_kernels.hip k2d_step_keep_dc, k2d_mesh_advance; the frame is csrc/run.hip's).

Two references, as tests/test_gpu_2d_run.py has them for a stand-alone Grid.  The states the reference's own SMR builds left
(tests/golden/g2dsmr_*.npz): the strict library bit for bit on every level with time, dt and dt0, the default library within the
project's 2-D bars (1e-11 of each field's maximum, 1e-12 in dt).  And Mesh.step() of the same library: run_2d gives its bits in
BOTH libraries -- the whole block of every level, ghost zones included, and (time, dt, nstep) -- so a step queued behind the stop
that stored anything, anywhere, shows."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import twodfix                      # noqa: E402
from twodfix import DECKS, NG, pkg  # noqa: E402

pytestmark = pytest.mark.gpu

DECK = os.path.join(DECKS, "athinput.blast2d_smr")
CASES = [("A", 8), ("A", 1), ("B", 8), ("C", 6), ("D", 8), ("E", 6)]
STOP_CASES = [("A", "ctu", 8), ("C", "vl", 6), ("D", "ctu", 8)]
TOL_U, TOL_DT = 1e-11, 1e-12          # the project's bars for 2-D Grids in the default build
FAR = 1.0e300                         # a t_stop no run reaches: the step count ends the call
NTRAJ = 9


def fixture(case, integ, n):
    return twodfix.fixture(f"g2dsmr_{case}_{integ}_s{n}")


def make_mesh(fx, strict, integ=None, extra=()):
    aa, cfg, lib = pkg(), pkg("config"), pkg("lib")
    ov = [str(o) for o in fx["overrides"]] + list(extra)
    par = aa.athinput.ParTable.from_file(DECK).cmdline(ov)
    run = cfg.load(DECK, ov, "blast", integ or str(fx["integrator"]))
    return lib.Mesh(cfg.levels_2d(par, run), 0, strict)


def active(U):
    return U[:, NG:-NG, NG:-NG, :]


def relerr(a, b):
    out = []
    for c in range(a.shape[-1]):
        scale = np.abs(b[..., c]).max()
        diff = float(np.abs(a[..., c] - b[..., c]).max())
        out.append(diff / scale if scale > 0 else (0.0 if diff == 0.0 else np.inf))
    return out


def state(m):
    return (m.time, m.dt, m.nstep), [g.download() for g in m.lev]


def same(a, b):
    return a[0] == b[0] and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def syncs(m, reset=False):
    return sum(g.host_syncs(reset) for g in m.lev)


_traj = {}


def trajectory(case, integ, n, strict, extra=()):
    """the per-step path: [(time, dt, nstep), whole block of every level] after 0 .. NTRAJ calls of Mesh.step(); run once and shared"""
    key = (case, integ, n, strict, tuple(extra))
    if key not in _traj:
        m = make_mesh(fixture(case, integ, n), strict, extra=extra)
        try:
            m.start()
            out = [state(m)]
            for _ in range(NTRAJ):
                m.step()
                out.append(state(m))
        finally:
            m.close()
        for _, Us in out:
            for U in Us:
                U.setflags(write=False)
        _traj[key] = out
    return _traj[key]


# ---- 1. the cases of the fixtures, both integrators, both builds ---------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("integ", ["ctu", "vl"])
@pytest.mark.parametrize("case,n", CASES, ids=[f"{c}{n}" for c, n in CASES])
def test_run_2d_reproduces_the_reference_and_the_per_step_path(case, n, integ, strict, monkeypatch):
    """K = 4: the 8-step cases are two full batches, the 6-step cases leave two queued steps behind the stop, A1 leaves three."""
    monkeypatch.setenv("AA_2D_BATCH", "4")
    fx = fixture(case, integ, n)
    m = make_mesh(fx, strict)
    try:
        assert m.can_run_2d() and m.run_2d_batch() == 4
        m.start()
        dt0 = m.dt
        assert m.run_2d(FAR, nstep_stop=n) == n
        s = state(m)
        assert [(g.time, g.dt, g.nstep) for g in m.lev] == [s[0]] * len(m.lev)       # every level's copy of MeshS
    finally:
        m.close()
    per_step = trajectory(case, integ, n, strict)[n]
    assert s[0][2] == n == int(fx["nstep"]) and len(s[1]) == int(fx["nlevels"])
    err = [relerr(active(U), fx[f"U_{l}"]) for l, U in enumerate(s[1])]
    e_dt0, e_dt, e_t = abs(dt0 / float(fx["dt0"]) - 1), abs(s[0][1] / float(fx["dt"]) - 1), abs(s[0][0] / float(fx["time"]) - 1)
    print(f"{case}{n} {integ} {'strict' if strict else 'default'}: max error / field maximum per level {[max(e) for e in err]}, "
          f"dt0 {e_dt0:.2e} dt {e_dt:.2e} time {e_t:.2e}; state {s[0]!r} per step {per_step[0]!r}")
    if strict:
        assert dt0 == float(fx["dt0"]) and s[0][0] == float(fx["time"]) and s[0][1] == float(fx["dt"])
        for l, U in enumerate(s[1]):
            assert np.array_equal(active(U), fx[f"U_{l}"]), f"level {l}: {err[l]}"
    else:
        assert e_dt0 < TOL_DT and e_dt < TOL_DT and e_t < TOL_DT
        for l in range(len(err)):
            assert max(err[l]) < TOL_U, f"level {l}: {err[l]}"
    assert s[0] == per_step[0], (s[0], per_step[0])
    for l, (U, V) in enumerate(zip(s[1], per_step[1])):
        assert np.array_equal(U, V), f"level {l} against step(): {relerr(U, V)}"


# ---- 2. the stop rules against the per-step path, four steps queued per read-back -------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("case,integ,n", STOP_CASES, ids=[f"{c}-{i}" for c, i, _ in STOP_CASES])
def test_stop_rules_leave_the_per_step_paths_state(case, integ, n, strict, monkeypatch):
    """nstep_stop one below, on and one above a batch of 4 and inside the third; a t_stop inside the second batch; t_stop at the
    mesh's own time and at 0.  A second call at the stop takes no step, costs no read-back and changes no byte."""
    monkeypatch.setenv("AA_2D_BATCH", "4")
    fx = fixture(case, integ, n)
    tr = trajectory(case, integ, n, strict)
    for k in (1, 3, 4, 5, 9):
        m = make_mesh(fx, strict)
        try:
            m.start()
            assert m.run_2d(FAR, nstep_stop=k) == k
            s = state(m)
            print(f"{case} {integ} strict={strict} nstep_stop={k}: {s[0]!r} / {tr[k][0]!r}")
            assert same(s, tr[k]), (k, s[0], tr[k][0])
            syncs(m, True)
            assert m.run_2d(FAR, nstep_stop=k) == 0 and syncs(m) == 0
            assert same(state(m), tr[k])
        finally:
            m.close()
    (t5, dt5, _), _ = tr[5]
    m = make_mesh(fx, strict)
    try:
        m.start()
        assert m.run_2d(t5 + 0.5 * dt5) == 6              # time >= t_stop first holds after the sixth step
        assert same(state(m), tr[6])
        assert m.run_2d(m.time) == 0 and m.run_2d(0.0) == 0 and same(state(m), tr[6])
    finally:
        m.close()


# ---- 3. the clip at tlim ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("case,integ,n", STOP_CASES[:2], ids=[f"{c}-{i}" for c, i, _ in STOP_CASES[:2]])
def test_the_last_dt_is_clipped_at_tlim(case, integ, n, strict, monkeypatch):
    monkeypatch.setenv("AA_2D_BATCH", "4")
    fx = fixture(case, integ, n)
    (t6, dt6, _), _ = trajectory(case, integ, n, strict)[6]
    tlim = t6 + 0.5 * dt6
    extra = [f"time/tlim={tlim!r}"]
    h = make_mesh(fx, strict, extra=extra)
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
    m = make_mesh(fx, strict, extra=extra)
    try:
        m.start()
        assert m.lev[0].cfg.run.tlim == tlim
        assert m.run_2d(tlim) == 7
        s = state(m)
        print(f"{case} {integ} strict={strict}: {s[0]!r} / {per_step[0]!r}")
        assert same(s, per_step)
    finally:
        m.close()


# ---- 4. mixed with step(): the hand-over between the host's dt and the device clock, both ways -------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("case,integ,n", STOP_CASES, ids=[f"{c}-{i}" for c, i, _ in STOP_CASES])
def test_run_2d_mixes_with_single_steps(case, integ, n, strict, monkeypatch):
    monkeypatch.setenv("AA_2D_BATCH", "4")
    tr = trajectory(case, integ, n, strict)
    m = make_mesh(fixture(case, integ, n), strict)
    try:
        m.start()
        assert m.run_2d(FAR, nstep_stop=3) == 3
        m.step(); m.step()
        assert same(state(m), tr[5])
        assert m.run_2d(FAR, nstep_stop=8) == 3
        assert same(state(m), tr[8])
    finally:
        m.close()


# ---- 5. the point of it: read-backs per call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_a_call_reads_back_once_per_batch(strict, monkeypatch):
    out = {}
    for k in ("4", "0"):
        monkeypatch.setenv("AA_2D_BATCH", k)
        m = make_mesh(fixture("A", "ctu", 8), strict)
        try:
            assert m.run_2d_batch() == int(k) and m.can_run_2d() == (k != "0")
            m.start()
            syncs(m, True)
            assert m.run_2d(FAR, nstep_stop=8) == 8
            out[k] = (syncs(m), m.lev[0].host_syncs(), state(m))
        finally:
            m.close()
    print(f"strict={strict}: host_syncs {out['4'][0]} with AA_2D_BATCH=4, {out['0'][0]} with AA_2D_BATCH=0")
    assert out["4"][0] == out["4"][1] == 2                 # one per batch, counted on the root
    assert out["0"][0] >= 8 and out["4"][0] < out["0"][0]
    assert same(out["4"][2], out["0"][2])                  # AA_2D_BATCH=0: run_2d steps to the same bits
    assert same(out["0"][2], trajectory("A", "ctu", 8, strict)[8])
    monkeypatch.setenv("AA_2D_BATCH", "-1")
    lib = pkg("lib")
    with pytest.raises(lib.AthenaError, match="AA_2D_BATCH"):
        make_mesh(fixture("A", "ctu", 8), strict)


# ---- 6. what aa_mesh_run_2d refuses ---------------------------------------------------------------------------------------------------
def test_refusals_set_the_last_error(monkeypatch):
    import ctypes as C
    import orc
    monkeypatch.setenv("AA_2D_BATCH", "4")
    aa, lib = pkg(), pkg("lib")
    L = lib.load(True)
    n = C.c_int()

    def refused(rc, *words):
        msg = L.aa_last_error().decode()
        assert rc != 0 and msg.startswith("[aa_mesh_run_2d]") and all(w in msg for w in words), (rc, msg)
    refused(L.aa_mesh_run_2d(None, 1.0, 1.0, 1, C.byref(n)), "null")
    assert L.aa_mesh_run_2d_batch(None) == 0
    # a Mesh of 3-D Grids
    gz = np.load(os.path.join(HERE, "golden", "smr_blast_3lev_s6.npz"))
    par = aa.athinput.ParTable.from_file(orc.deck_for("blast", gz)).cmdline([str(o) for o in gz["overrides"]])
    run3 = aa.config.from_par(par, "blast")
    m3 = lib.Mesh(aa.config.levels(par, run3), 0, True)
    try:
        assert not m3.can_run_2d() and m3.run_2d_batch() == 0
        refused(L.aa_mesh_run_2d(m3._h, 1.0, run3.tlim, 1, C.byref(n)), "3-D")
        with pytest.raises(lib.AthenaError, match="3-D"):
            m3.run_2d(1.0)
    finally:
        m3.close()
    fx = fixture("A", "ctu", 8)
    tr = trajectory("A", "ctu", 8, True)
    m = make_mesh(fx, True)
    try:
        m.start()
        tlim = m.lev[0].cfg.run.tlim
        with pytest.raises(lib.AthenaError, match="tlim"):
            m.run_2d(tlim, tlim=2.0 * tlim)
        with pytest.raises(lib.AthenaError, match="2\\^20"):
            m.run_2d(tlim, nstep_stop=(1 << 20) + 1)
        with pytest.raises(lib.AthenaError, match="2\\^20"):
            m.run_2d(tlim, nstep_stop=-1)
        assert same(state(m), tr[0])                       # a refused call touches nothing
        for lev in m.lev:                                  # aa_run_2d on a level keeps refusing
            assert L.aa_run_2d(lev._h, 1.0, tlim, 1, C.byref(n)) != 0 and "Mesh" in L.aa_last_error().decode()
        # a pinned zone on level 1: refused, and step() still takes it
        g = m.lev[1]
        idx = (NG + 2) * g.N[0] + NG + 1
        pin = np.array([[1.0, 0.0, 0.0, 0.0, 2.5]])
        g.set_pinned_cells(np.array([idx]), pin)
        assert not m.can_run_2d()
        refused(L.aa_mesh_run_2d(m._h, tlim, tlim, 3, C.byref(n)), "pinned")
        assert m.nstep == 0
        m.step()
        assert m.nstep == 1 and np.array_equal(g.download()[0, NG + 2, NG + 1], pin[0])
    finally:
        m.close()


# ---- 7. MeshRun.main with <outputN> blocks: batched, by the knob, overlapped ----------------------------------------------------------
def _tree(d):
    return sorted(os.path.relpath(os.path.join(dp, f), d) for dp, _, fs in os.walk(d) for f in fs)


def _payload(b):
    return b[b.index(b"<par_end>\n") + len(b"<par_end>\n"):]


def _meshrun(fx, mode, out, monkeypatch, extra=()):
    cfg, D, O, A, lib = pkg("config"), pkg("driver"), pkg("outputs"), pkg("athinput"), pkg("lib")
    monkeypatch.setenv("AA_2D_BATCH", "0" if mode == "knob" else "4")
    blocks = json.loads(str(fx["blocks"]))
    ov = [str(o) for o in fx["overrides"]] + [f"job/maxout={max(int(n) for n in blocks)}"]
    for n, kv in blocks.items():
        ov += [f"output{n}/{k}={v}" for k, v in kv.items()]
    ov += list(extra)
    par = A.ParTable.from_file(DECK).cmdline(ov)
    run = cfg.load(DECK, ov, "blast", "ctu")
    m = D.MeshRun(lib.Mesh(cfg.levels_2d(par, run), 0, True), run)
    try:
        assert m.may_batch() == (mode != "knob")
        calls = []
        adv = m.advance
        monkeypatch.setattr(m, "advance", lambda *a: (calls.append(adv(*a)), calls[-1])[1])
        syncs(m.mesh, True)
        m.main(O.OutputSet.from_par(par, 0.0, out, overlap=(mode == "overlap")))
        return dict(syncs=syncs(m.mesh), nstep=m.nstep, calls=calls, state=state(m.mesh), blocks=blocks)
    finally:
        m.mesh.close()


def _same_trees(res, tmp_path, paths):
    for mode, r in res.items():
        print(f"{mode}: {r['nstep']} steps, host_syncs {r['syncs']}, advance() -> {r['calls']}")
        assert _tree(str(tmp_path / mode)) == paths
        assert same(r["state"], res["knob"]["state"])
        for rel in paths:
            assert open(os.path.join(tmp_path / mode, rel), "rb").read() == open(os.path.join(tmp_path / "knob", rel), "rb").read(), (mode, rel)
    assert res["knob"]["calls"] == []


def test_meshrun_main_batches_and_writes_the_same_files(tmp_path, monkeypatch):
    """g2dsmr_out_A (hst + bin + vtk + rst), three ways: the three trees byte for byte the same, every file; against the fixture as
    tests/test_gpu_2d_smr.py compares them.  advance() is called once per stretch between two output times."""
    import dumpfix
    A = pkg("athinput")
    fx = twodfix.fixture("g2dsmr_out_A")
    paths = [str(p) for p in fx["paths"]]
    files = {p: fx[f"file_{i}"].tobytes() for i, p in enumerate(paths)}
    res = {mode: _meshrun(fx, mode, str(tmp_path / mode), monkeypatch) for mode in ("batched", "knob", "overlap")}
    _same_trees(res, tmp_path, paths)
    blocks = res["knob"]["blocks"]
    for mode in ("batched", "overlap"):      # (a pass with an output overdue takes a single step)
        assert 0 < sum(res[mode]["calls"]) <= res[mode]["nstep"] and all(c > 0 for c in res[mode]["calls"])
        assert res[mode]["syncs"] <= res["knob"]["syncs"]
    nxs = [tuple(int(v) for v in nx) for nx in fx["nxs"]]
    full = str(tmp_path / "batched")
    for rel in paths:
        ours = open(os.path.join(full, rel), "rb").read(); ref = files[rel]
        ext = rel.rsplit(".", 1)[1]
        lev = int(rel[3]) if rel.startswith("lev") else 0
        if ext in ("vtk", "bin"):
            k = {"bin": "2", "vtk": "3"}[ext]
            assert dumpfix.compare_dump(ours, ref, nxs[lev], 0, ext, blocks[k].get("out", "cons") == "prim", rel) == 0
        elif ext == "rst":
            assert _payload(ours) == _payload(ref), rel
            po = A.ParTable.from_text(ours[:ours.index(b"<par_end>")].decode())
            pr = A.ParTable.from_text(ref[:ref.index(b"<par_end>")].decode(errors="replace"))
            for k in blocks:
                assert po.geti(f"output{k}", "num") == pr.geti(f"output{k}", "num"), (rel, k)
                assert po.getd(f"output{k}", "time") == pr.getd(f"output{k}", "time"), (rel, k)
            assert po.getd("time", "time") == pr.getd("time", "time") and po.geti("time", "nstep") == pr.geti("time", "nstep")
        else:
            lo, lr = ours.decode().splitlines(), ref.decode().splitlines()
            assert lo[:3] == lr[:3] and len(lo) == len(lr) > 4, (rel, lo[:3], lr[:3])
            for a, b in zip(lo[3:], lr[3:]):
                ca, cb = a.split(), b.split()
                assert ca[:4] == cb[:4] and ca[7:] == cb[7:], (rel, a, b)
                assert all(abs(float(x) - float(y)) <= 1e-9 * float(cb[2]) for x, y in zip(ca[4:7], cb[4:7])), (rel, a, b)


def test_meshrun_main_reads_back_less_often_when_it_batches(tmp_path, monkeypatch):
    """the same deck and output blocks at cour_no 0.2: a stretch between two output times is several steps, so the batched runs
    must read back FEWER times than the stepping one -- with the same byte-for-byte comparison of the trees"""
    fx = twodfix.fixture("g2dsmr_out_A")
    extra = ["time/cour_no=0.2"]
    res = {mode: _meshrun(fx, mode, str(tmp_path / mode), monkeypatch, extra) for mode in ("batched", "knob", "overlap")}
    paths = _tree(str(tmp_path / "knob"))
    assert {p.rsplit(".", 1)[1] for p in paths} == {"hst", "bin", "vtk", "rst"}
    _same_trees(res, tmp_path, paths)
    nl = len(res["knob"]["state"][1])
    assert res["knob"]["nstep"] >= 8 and res["knob"]["syncs"] >= nl * res["knob"]["nstep"]      # aa_mesh_new_dt: a read-back per level and step
    for mode in ("batched", "overlap"):
        single = res[mode]["nstep"] - sum(res[mode]["calls"])      # (a pass with an output overdue takes a single step)
        assert 0 <= single <= 4 and sum(res[mode]["calls"]) > len(res[mode]["calls"])
        assert res[mode]["syncs"] < res["knob"]["syncs"]
        # aa_mesh_new_dt of the start and of every single step (a read-back per level), ceil(steps / K) + 1 per call at the most
        assert res[mode]["syncs"] <= nl * (1 + single) + sum(-(-c // 4) + 1 for c in res[mode]["calls"])


# ---- 8. a restarted run ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("integ", ["ctu", "vl"])
def test_resume_from_the_reference_s_dump_batched(integ, strict, tmp_path, monkeypatch):
    """MeshRun.from_restart on the reference's dump of case A after 4 steps, then main() with time/nlim = 8 and no output block:
    ONE advance() call of four steps arrives where the reference arrives with -r at step 8 (strict: bit for bit, time and dt)."""
    monkeypatch.setenv("AA_2D_BATCH", "4")
    D, O = pkg("driver"), pkg("outputs")
    fx = twodfix.fixture(f"g2dsmr_restart_A_{integ}")
    seed = str(tmp_path / "seed.rst")
    with open(seed, "wb") as f:
        f.write(fx["seed"].tobytes())
    r = D.MeshRun.from_restart(seed, [f"time/nlim={int(fx['nstep'])}", "job/maxout=0"], "blast", integ, strict=strict)
    try:
        assert r.restarted and r.nstep == 4 and r.may_batch()
        calls = []
        adv = r.advance
        monkeypatch.setattr(r, "advance", lambda *a: (calls.append(adv(*a)), calls[-1])[1])
        r.main(O.OutputSet.from_par(r.par, r.time, str(tmp_path / "run")))
        assert r.nstep == int(fx["nstep"]) == 8 and calls == [4]
        err = [relerr(active(g.download()), fx[f"U_{l}"]) for l, g in enumerate(r.mesh.lev)]
        print(f"resumed {integ} {'strict' if strict else 'default'}: {[max(e) for e in err]}")
        if strict:
            assert r.time == float(fx["time"]) and r.dt == float(fx["dt"])
            for l, g in enumerate(r.mesh.lev):
                assert np.array_equal(active(g.download()), fx[f"U_{l}"]), (l, err[l])
        else:
            assert abs(r.time / float(fx["time"]) - 1) < TOL_DT and abs(r.dt / float(fx["dt"]) - 1) < TOL_DT
            assert max(max(e) for e in err) < TOL_U, err
    finally:
        r.mesh.close()
