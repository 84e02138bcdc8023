"""History rows of a queued run on an MI355X: aa_run_hst_arm / aa_mesh_run_hst_arm put the decision when a row of an ``hst`` block
is due, and the last additions of the row, behind every queued step (csrc/history_dc.hip k_history_dc, csrc/run.hip k_hst_row;
the rule is csrc/time_step.h hst_row_due), so that ``OutputSet(hst_queued=True)`` keeps Driver.main / MeshRun.main queued through
the history outputs.

The yardstick is the per-step path: step(), the rule of outputs.data_output restated below, Grid.history().  Every comparison is
BIT FOR BIT in both libraries -- k_history_dc shares k_history's body and launch geometry, k_hst_row adds the partial rows in
aa_history's order -- rows (time, dt, nine sums), end states, files."""
import ctypes as C
import json
import os
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import orc                                   # noqa: E402
import twodfix                               # noqa: E402
from twodfix import DECKS, pkg               # noqa: E402
import test_gpu_2d as g2                     # noqa: E402   (_out_par, _payload: the rule of the 24 x 20 output fixture)
import test_gpu_2d_smr_run as m2             # noqa: E402   (make_mesh, fixture, state, same, syncs)
import test_gpu_3d_run as t3                 # noqa: E402   (blast, matrix, BIG)
import test_gpu_3d_smr_run as m3             # noqa: E402   (blast_mesh)

pytestmark = pytest.mark.gpu
FAR = 1.0e300
BOTH = pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
DECK2D = os.path.join(DECKS, "athinput.blast2d")
MESH2D = ("A", "ctu", 8)                     # the smallest Mesh of tests/test_gpu_2d_smr_run.py
MESH3D = "smr_blast_3lev_s6"                 # ... and of tests/test_gpu_3d_smr_run.py


def rule(time, nstep, tlim, nlim, t_next, dt_out):
    """outputs.run + OutputSet.data_output for one block behind a taken step (tests/test_hst_run_host.py holds
    csrc/time_step.h hst_row_due to the same restatement)"""
    if not (time < tlim and (nlim is None or nstep < nlim)):
        return False, t_next
    if time >= t_next:
        return True, t_next + dt_out
    return False, t_next


def grids_of(x):
    return list(x.lev) if hasattr(x, "lev") else [x]


def snapshot(x):
    return (x.time, x.dt, x.nstep), [g.download() for g in grids_of(x)]


def same(a, b):
    return a[0] == b[0] and all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a[1], b[1]))


def stepped(x, live, arm, tlim):
    """the per-step path on a started Grid or Mesh: step() while live(x), the rule behind every step, history() of every Grid
    where a row is due -> ([rows of Grid 0, ...], t_next)"""
    t_next, dt_out, nlim = arm
    rows = [[] for _ in grids_of(x)]
    while live(x):
        x.step()
        due, t_next = rule(x.time, x.nstep, tlim, nlim, t_next, dt_out)
        if due:
            for r, g in zip(rows, grids_of(x)):
                r.append([x.time, x.dt] + list(g.history()))
    return [np.array(r).reshape(-1, 11) for r in rows], t_next


def queued(x, t_stop, nstep_stop, arm):
    """the same through one armed run call -> (steps, [rows of Grid 0, ...], t_next)"""
    run = (x.run_2d if x.can_run_2d() else x.run_3d) if hasattr(x, "lev") else (x.run_2d if x.ndim == 2 else x.run_3d)
    x.run_hst_arm(*arm)
    n = run(t_stop, nstep_stop=nstep_stop)
    rows, t_next = x.run_hst_rows()
    return n, (rows if hasattr(x, "lev") else [rows]), t_next


def rows_equal(a, b):
    return len(a) == len(b) and all(p.shape == q.shape and p.tobytes() == q.tobytes() for p, q in zip(a, b))


def compare(make, n, arm, tlim=None, t_stop=FAR, label=""):
    """n steps (or up to t_stop) both ways on twins: rows, the schedule's next time, end state"""
    a = make()
    try:
        tl = a.lev[0].cfg.run.tlim if hasattr(a, "lev") else a.cfg.run.tlim
        tl = tl if tlim is None else tlim
        want, t_want = stepped(a, lambda x: x.time < t_stop and x.nstep != n and x.dt > 0.0, arm, tl)
        end = snapshot(a)
    finally:
        a.close()
    b = make()
    try:
        taken, got, t_got = queued(b, t_stop, n, arm)
        print(f"{label}: {taken} steps, {len(got[0])} rows per Grid on {len(got)} Grid(s), t_next {t_got!r} / {t_want!r}, "
              f"state {snapshot(b)[0]!r}")
        assert taken == end[0][2] and same(snapshot(b), end)
        assert rows_equal(got, want), [(p.tolist(), q.tolist()) for p, q in zip(got, want)][:1]
        assert t_got == t_want or (t_got != t_got and t_want != t_want)
    finally:
        b.close()
    return want


def blast2d(nx, strict, extra=()):
    cfg, lib = pkg("config"), pkg("lib")
    run = cfg.load(DECK2D, [f"domain1/Nx1={nx[0]}", f"domain1/Nx2={nx[1]}"] + list(extra), "blast")
    g = lib.setup_problem(cfg.slab(run), 0, strict)
    g.start()
    return g


def mesh2d(strict):
    m = m2.make_mesh(m2.fixture(*MESH2D), strict)
    m.start()
    return m


def mesh3d(strict):
    m = m3.blast_mesh(MESH3D, strict)
    m.start()
    return m


# ---- 1. rows equal the per-step path's ---------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("nx", [(24, 20), (67, 35)], ids=["24x20", "67x35"])
def test_rows_of_a_2d_grid(nx, strict, monkeypatch):
    """67 x 35: ten partial rows, dx1 != dx2; nine steps at K = 4 leave three queued steps behind the stop"""
    monkeypatch.setenv("AA_2D_BATCH", "4")
    want = compare(lambda: blast2d(nx, strict), 9, (0.0, 1.0e-6, None), label=f"2-D {nx} strict={strict}")
    assert len(want[0]) == 9 and np.all(want[0][:, 2] > 0)


@BOTH
@pytest.mark.parametrize("nscal", [0, 1], ids=["hydro", "scalar"])
def test_rows_of_a_3d_grid(nscal, strict, monkeypatch):
    """24 x 20 x 16 on the queued chain (AA_CORRECT_ALL=1, as tests/test_gpu_3d_run.py forces it); column 9 with the scalar"""
    t3.set_knobs(monkeypatch, t3.BIG)
    monkeypatch.setenv("AA_3D_BATCH", "4")

    def make():
        g = t3.matrix("ctu", (24, 20, 16), strict, nscal)
        assert g.run_3d_batch() == 4
        return g
    want = compare(make, 6, (0.0, 1.0e-9, None), label=f"3-D nscal={nscal} strict={strict}")
    assert len(want[0]) == 6 and (np.all(want[0][:, 10] > 0) if nscal else np.all(want[0][:, 10] == 0))


@BOTH
def test_rows_of_a_3d_grid_beyond_the_block_cap(strict, monkeypatch):
    """72 x 64 x 64 = 294912 zones > 1024 x 256: k_history's cap of 1024 blocks and its grid-stride loop"""
    t3.set_knobs(monkeypatch, t3.BIG)
    monkeypatch.setenv("AA_3D_BATCH", "2")
    want = compare(lambda: t3.blast((72, 64, 64), strict), 3, (0.0, 1.0e-9, None), label=f"3-D 72x64x64 strict={strict}")
    assert len(want[0]) == 3


@BOTH
def test_rows_of_every_level_of_a_2d_mesh(strict, monkeypatch):
    monkeypatch.setenv("AA_2D_BATCH", "4")
    want = compare(lambda: mesh2d(strict), 6, (0.0, 1.0e-9, None), label=f"2-D Mesh strict={strict}")
    assert len(want) >= 2 and all(len(r) == 6 for r in want)
    assert len({r[:, 2].tobytes() for r in want}) == len(want)      # every level its own sums


@BOTH
def test_rows_of_every_level_of_a_3d_mesh(strict, monkeypatch):
    monkeypatch.setenv("AA_CORRECT_ALL", "1")
    monkeypatch.setenv("AA_3D_BATCH", "2")

    def make():
        m = mesh3d(strict)
        assert m.run_3d_batch() == 2
        return m
    want = compare(make, 5, (0.0, 1.0e-9, None), label=f"3-D Mesh strict={strict}")
    assert len(want) == 3 and all(len(r) == 5 for r in want)


# ---- 2. the rule's cases, four steps queued per read-back -----------------------------------------------------------------------------
_traj = {}


def trajectory(strict):
    """(time, dt, nstep) behind 0 .. 12 steps of the 24 x 20 blast, run once and shared"""
    if strict not in _traj:
        g = blast2d((24, 20), strict)
        out = [(g.time, g.dt, g.nstep)]
        for _ in range(12):
            g.step()
            out.append((g.time, g.dt, g.nstep))
        g.close()
        _traj[strict] = out
    return _traj[strict]


@BOTH
def test_rule_cases(strict, monkeypatch):
    monkeypatch.setenv("AA_2D_BATCH", "4")
    tr = trajectory(strict)
    make = lambda: blast2d((24, 20), strict)      # noqa: E731
    step = tr[5][1]
    # every step fires: the next time lags behind the clock and still advances once per row
    w = compare(make, 10, (0.0, 1.0e-7, None), label="every step")
    assert len(w[0]) == 10
    # about 2.5 steps between two rows
    w = compare(make, 10, (tr[2][0], 2.5 * step, None), label="2.5 steps")
    assert 3 <= len(w[0]) <= 5
    # beyond the span: no row, the schedule's next time as armed
    w = compare(make, 10, (1.0e3, 1.0, None), label="beyond")
    assert len(w[0]) == 0
    # a stop inside a batch (nstep_stop = 6 at K = 4): a row behind the stop step, none behind the two empty steps
    w = compare(make, 6, (0.0, 1.0e-7, None), label="stop inside a batch")
    assert len(w[0]) == 6 and w[0][-1, 0] == tr[6][0]
    # a call that ends at t_stop < tlim with a row due behind its last step: that row comes from the device
    t_stop = tr[6][0]
    w = compare(make, None, (tr[6][0], 1.0, None), t_stop=t_stop, label="t_stop with a row due")
    assert len(w[0]) == 1 and w[0][0, 0] == tr[6][0]
    # the loop's end by nlim: no row behind the last step (the forced output writes that one)
    w = compare(make, 7, (0.0, 1.0e-7, 7), label="nlim")
    assert len(w[0]) == 6 and w[0][-1, 0] == tr[6][0]
    # ... and by tlim, the last dt clipped
    tlim = tr[6][0] + 0.5 * tr[6][1]
    mk = lambda: blast2d((24, 20), strict, [f"time/tlim={tlim!r}"])      # noqa: E731
    w = compare(mk, None, (0.0, 1.0e-7, None), tlim=tlim, t_stop=tlim, label="tlim")
    assert len(w[0]) == 6 and w[0][-1, 0] == tr[6][0]


@BOTH
def test_queued_and_stepwise_calls_give_the_same_rows(strict, monkeypatch):
    """AA_2D_BATCH=0 and a Grid with fewer zones than ghost zones along x2: the frame applies the rule on the host behind aa_step"""
    tr = trajectory(strict)
    arm = (tr[1][0], 2.5 * tr[5][1], None)
    out = {}
    for k in ("4", "0"):
        monkeypatch.setenv("AA_2D_BATCH", k)
        g = blast2d((24, 20), strict)
        assert g.run_2d_batch() == int(k)
        out[k] = queued(g, FAR, 10, arm) + (snapshot(g),)
        g.close()
    assert out["4"][0] == out["0"][0] == 10 and rows_equal(out["4"][1], out["0"][1]) and out["4"][2] == out["0"][2]
    assert same(out["4"][3], out["0"][3]) and len(out["4"][1][0]) >= 3
    monkeypatch.setenv("AA_2D_BATCH", "4")
    compare(lambda: blast2d((24, 3), strict), 5, (0.0, 1.0e-7, None), label="24x3: stepwise inside the call")


# ---- 3. whole runs --------------------------------------------------------------------------------------------------------------------
def _tree(d):
    return sorted(os.path.relpath(os.path.join(dp, f), d) for dp, _, fs in os.walk(d) for f in fs)


def _read(d, rel):
    return open(os.path.join(str(d), rel), "rb").read()


def _driver_main(par, out, queued_, monkeypatch, restart=None):
    cfg, D, O = pkg("config"), pkg("driver"), pkg("outputs")
    monkeypatch.setenv("AA_2D_BATCH", "4" if queued_ else "0")
    d = D.Driver.from_restart(restart, strict=True) if restart else D.Driver(cfg.from_par(par, "blast"), strict=True)
    try:
        calls = []
        adv = d.advance

        def advance(*a, **k):
            s0 = d.eng.host_syncs()
            n = adv(*a, **k)
            calls.append((n, d.eng.host_syncs() - s0, "hst" in k))
            return n
        monkeypatch.setattr(d, "advance", advance)
        d.eng.host_syncs(True)
        outs = O.OutputSet.from_par(d.par if restart else par, d.time if restart else 0.0, out, hst_queued=queued_)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                     # no fallback here
            d.main(outs)
        return dict(syncs=d.eng.host_syncs(), state=(d.time, d.dt, d.nstep), U=d.eng.download(), calls=calls, written=set(outs.written))
    finally:
        d.eng.close()


def _same_trees(a, b, da, db):
    paths = _tree(da)
    assert _tree(db) == paths and a["written"] == b["written"] == set(paths)
    for rel in paths:
        assert _read(da, rel) == _read(db, rel), rel
    assert a["state"] == b["state"] and np.array_equal(a["U"], b["U"])
    return paths


def test_driver_main_writes_the_same_tree_and_the_fixtures_files(tmp_path, monkeypatch):
    """the 24 x 20 run of g2d_out_blast_24x20 (hst, bin, vtk prim, rst): per step against hst_queued at K = 4 byte for byte, and
    the queued tree against the reference's files by the rule of tests/test_gpu_2d.py"""
    import dumpfix
    A = pkg("athinput")
    fx = twodfix.fixture("g2d_out_blast_24x20")
    par, blocks = g2._out_par(fx)
    ref = _driver_main(par, str(tmp_path / "step"), False, monkeypatch)
    par, _ = g2._out_par(fx)
    got = _driver_main(par, str(tmp_path / "queued"), True, monkeypatch)
    paths = _same_trees(ref, got, str(tmp_path / "step"), str(tmp_path / "queued"))
    assert ref["calls"] == [] and got["calls"] and all(c[2] for c in got["calls"])
    assert paths == [str(p) for p in fx["paths"]]
    files = {p: fx[f"file_{i}"].tobytes() for i, p in enumerate(paths)}
    nx = (int(fx["nx"][0]), int(fx["nx"][1]), 1)
    for rel in paths:
        ours, theirs = _read(tmp_path / "queued", rel), files[rel]
        ext = rel.rsplit(".", 1)[1]
        if ext in ("vtk", "bin"):
            n = {"bin": "2", "vtk": "3"}[ext]
            assert dumpfix.compare_dump(ours, theirs, nx, 0, ext, blocks[n].get("out", "cons") == "prim", rel) == 0
        elif ext == "rst":
            assert g2._payload(ours) == g2._payload(theirs), rel
            po = A.ParTable.from_text(ours[:ours.index(b"<par_end>")].decode())
            pr = A.ParTable.from_text(theirs[:theirs.index(b"<par_end>")].decode(errors="replace"))
            for n in blocks:
                assert po.geti(f"output{n}", "num") == pr.geti(f"output{n}", "num"), (rel, n)
                assert po.getd(f"output{n}", "time") == pr.getd(f"output{n}", "time"), (rel, n)
        else:
            lo, lr = ours.decode().splitlines(), theirs.decode().splitlines()
            assert lo[:3] == lr[:3] and len(lo) == len(lr) == 7
            for a, b in zip(lo[3:], lr[3:]):
                ca, cb = a.split(), b.split()
                assert ca[:4] == cb[:4] and ca[7:] == cb[7:], (a, b)
                assert all(abs(float(x) - float(y)) <= 1e-9 * float(cb[2]) for x, y in zip(ca[4:7], cb[4:7])), (a, b)


# (cour_no 0.02: some sixty steps of 2e-4 up to tlim, a history row due behind nearly every one)
MANY_ROWS = ["time/cour_no=0.02", "time/tlim=0.012", "output1/dt=0.00015", "output2/dt=0.005", "output3/dt=0.007", "output4/dt=0.004"]


def test_driver_main_with_a_row_behind_nearly_every_step_and_a_resume(tmp_path, monkeypatch):
    """the same deck and blocks with the history block a fraction of a step apart and restart dumps between: trees byte for byte
    (every rst with its table), then a run resumed from the second rst with hst_queued leaves the rows of the uninterrupted run"""
    fx = twodfix.fixture("g2d_out_blast_24x20")

    def par():
        return g2._out_par(fx)[0].cmdline(MANY_ROWS)
    ref = _driver_main(par(), str(tmp_path / "step"), False, monkeypatch)
    got = _driver_main(par(), str(tmp_path / "queued"), True, monkeypatch)
    paths = _same_trees(ref, got, str(tmp_path / "step"), str(tmp_path / "queued"))
    assert {p.rsplit(".", 1)[1] for p in paths} == {"hst", "bin", "vtk", "rst"}
    rsts = [p for p in paths if p.endswith(".rst")]
    assert len(rsts) >= 4
    rows = _read(tmp_path / "step", "Blast.hst").decode().splitlines()[3:]
    print(f"{ref['state'][2]} steps, {len(rows)} rows, advance() -> {got['calls']}, host_syncs {got['syncs']} / {ref['syncs']}")
    assert len(rows) > 0.7 * ref["state"][2] and sum(c[0] for c in got["calls"]) > 2 * len(got["calls"])
    assert got["syncs"] < ref["syncs"]
    # resumed from the second dump, both ways
    seed = os.path.join(str(tmp_path / "step"), rsts[1])
    r_ref = _driver_main(None, str(tmp_path / "r_step"), False, monkeypatch, restart=seed)
    r_got = _driver_main(None, str(tmp_path / "r_queued"), True, monkeypatch, restart=seed)
    _same_trees(r_ref, r_got, str(tmp_path / "r_step"), str(tmp_path / "r_queued"))
    assert r_got["state"] == ref["state"] and np.array_equal(r_got["U"], ref["U"])
    tail = _read(tmp_path / "r_queued", "Blast.hst").decode().splitlines()
    assert tail and not tail[0].startswith("#") and rows[-len(tail):] == tail      # no header, the uninterrupted run's last rows


def _meshrun_main(out, queued_, monkeypatch, extra=()):
    cfg, D, O, A, lib = pkg("config"), pkg("driver"), pkg("outputs"), pkg("athinput"), pkg("lib")
    monkeypatch.setenv("AA_2D_BATCH", "4" if queued_ else "0")
    fx = twodfix.fixture("g2dsmr_out_A")
    blocks = json.loads(str(fx["blocks"]))
    ov = [str(o) for o in fx["overrides"]] + [f"job/maxout={max(int(n) for n in blocks)}"]
    for n, kv in blocks.items():
        ov += [f"output{n}/{k}={v}" for k, v in kv.items()]
    ov += list(extra)
    par = A.ParTable.from_file(m2.DECK).cmdline(ov)
    run = cfg.load(m2.DECK, ov, "blast", "ctu")
    m = D.MeshRun(lib.Mesh(cfg.levels_2d(par, run), 0, True), run)
    try:
        calls = []
        adv = m.advance

        def advance(*a, **k):
            s0 = m2.syncs(m.mesh)
            n = adv(*a, **k)
            calls.append((n, m2.syncs(m.mesh) - s0, "hst" in k))
            return n
        monkeypatch.setattr(m, "advance", advance)
        m2.syncs(m.mesh, True)
        outs = O.OutputSet.from_par(par, 0.0, out, hst_queued=queued_)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            m.main(outs)
        st = m2.state(m.mesh)
        return dict(syncs=m2.syncs(m.mesh), state=st[0], U=np.concatenate([u.reshape(-1) for u in st[1]]), calls=calls,
                    written=set(outs.written), nl=len(m.mesh.lev))
    finally:
        m.mesh.close()


def test_meshrun_main_writes_the_same_tree(tmp_path, monkeypatch):
    """g2dsmr_out_A (hst of every level, bin, vtk, rst), then the same with a history row behind nearly every step"""
    for tag, extra in (("deck", ()), ("rows", ("time/cour_no=0.2", "output1/dt=0.0005"))):
        ref = _meshrun_main(str(tmp_path / f"{tag}_step"), False, monkeypatch, extra)
        got = _meshrun_main(str(tmp_path / f"{tag}_queued"), True, monkeypatch, extra)
        paths = _same_trees(ref, got, str(tmp_path / f"{tag}_step"), str(tmp_path / f"{tag}_queued"))
        assert {p.rsplit(".", 1)[1] for p in paths} == {"hst", "bin", "vtk", "rst"}
        assert sum(1 for p in paths if p.endswith(".hst")) == ref["nl"]
        print(f"{tag}: {ref['state'][2]} steps, advance() -> {got['calls']}, read-backs {got['syncs']} / {ref['syncs']}")
        assert ref["calls"] == [] and got["calls"] and all(c[2] for c in got["calls"])
    assert got["syncs"] < ref["syncs"]


# ---- 4. the point of it: read-backs -----------------------------------------------------------------------------------------------------
ONLY_HST = ["job/maxout=1", "output1/dt=1e-6", "time/nlim=24", "domain1/Nx1=24", "domain1/Nx2=20"]


def test_a_grid_reads_back_once_per_batch_with_a_row_behind_every_step(tmp_path, monkeypatch):
    """N = 24 steps, a row behind every one, no other block due: ceil(N/K) + 1 read-backs per call with hst_queued, fewer than the
    rows written; a read-back per step without"""
    A = pkg("athinput")
    res = {}
    for q in (True, False):
        monkeypatch.setenv("AA_2D_BATCH", "4")
        par = A.ParTable.from_file(DECK2D).cmdline(ONLY_HST)
        cfg, D, O = pkg("config"), pkg("driver"), pkg("outputs")
        d = D.Driver(cfg.from_par(par, "blast"), strict=True)
        try:
            calls = []
            adv = d.advance

            def advance(*a, adv=adv, d=d, calls=calls, **k):
                s0 = d.eng.host_syncs()
                n = adv(*a, **k)
                calls.append((n, d.eng.host_syncs() - s0))
                return n
            monkeypatch.setattr(d, "advance", advance)
            outs = O.OutputSet.from_par(par, 0.0, str(tmp_path / str(q)), hst_queued=q)
            d.eng.host_syncs(True)
            d.main(outs)
            rows = len(_read(tmp_path / str(q), "Blast.hst").decode().splitlines()) - 3
            res[q] = dict(calls=calls, syncs=d.eng.host_syncs(), rows=rows, nstep=d.nstep, hst=_read(tmp_path / str(q), "Blast.hst"))
        finally:
            d.eng.close()
    print({q: (r["calls"], r["syncs"], r["rows"]) for q, r in res.items()})
    assert res[True]["nstep"] == res[False]["nstep"] == 24 and res[True]["rows"] == res[False]["rows"] == 25
    assert res[True]["hst"] == res[False]["hst"]
    assert [n for n, _ in res[True]["calls"]] == [24]               # ONE call: the armed block is no stop time
    assert all(s <= -(-n // 4) + 1 for n, s in res[True]["calls"])
    assert res[True]["syncs"] < res[True]["rows"]
    assert res[False]["syncs"] >= 24


def test_a_mesh_reads_back_once_per_batch_with_a_row_behind_every_step(tmp_path, monkeypatch):
    """the read-backs of all levels added up, as tests/test_gpu_3d_smr_run.py counts them"""
    extra = ("job/maxout=1", "output1/dt=1e-6", "time/nlim=24", "time/tlim=1.0")
    got = _meshrun_main(str(tmp_path / "queued"), True, monkeypatch, extra)
    ref = _meshrun_main(str(tmp_path / "step"), False, monkeypatch, extra)
    _same_trees(ref, got, str(tmp_path / "step"), str(tmp_path / "queued"))
    rows = len(_read(tmp_path / "queued", sorted(got["written"])[0]).decode().splitlines()) - 3
    print(f"queued: advance() -> {got['calls']}, read-backs {got['syncs']}; stepping: {ref['syncs']}; rows {rows}")
    assert got["state"][2] == 24 and rows == 25
    assert [c[0] for c in got["calls"]] == [24] and all(s <= -(-n // 4) + 1 for n, s, _ in got["calls"])
    assert got["syncs"] < rows and ref["syncs"] >= 24 * ref["nl"]


# ---- 5. refusals and fall-backs ---------------------------------------------------------------------------------------------------------
def test_refusals_set_the_last_error(monkeypatch):
    aa, cfg, lib = pkg(), pkg("config"), pkg("lib")
    L = lib.load(True)

    def refused(rc, who, *words):
        msg = L.aa_last_error().decode()
        assert rc != 0 and msg.startswith(f"[{who}]") and all(w in msg for w in words), (rc, msg)
    refused(L.aa_run_hst_arm(None, 0.0, 1.0, -1), "aa_run_hst_arm", "null")
    refused(L.aa_mesh_run_hst_arm(None, 0.0, 1.0, -1), "aa_mesh_run_hst_arm", "null")
    # a 1-D Grid
    run1 = cfg.load(os.path.join(DECKS, "athinput.blast1d"), ["domain1/Nx1=8"], "blast")
    g1 = lib.Grid(cfg.slab(run1), 0, True)
    try:
        refused(L.aa_run_hst_arm(g1._h, 0.0, 1.0, -1), "aa_run_hst_arm", "1-D", "aa_run_1d")
        with pytest.raises(lib.AthenaError, match="1-D"):
            g1.run_hst_arm(0.0, 1.0)
    finally:
        g1.close()
    # a Grid cut into slabs (both on this device)
    monkeypatch.setenv("AA_SLAB_DEVICES", "0,0")
    run3 = cfg.load(os.path.join(orc.DECKS, "athinput.blast"), t3.nx_ov((24, 20, 16)), "blast")
    gs = lib.setup_problem(cfg.slab(run3), 0, True, nslab=2)
    try:
        refused(L.aa_run_hst_arm(gs._h, 0.0, 1.0, -1), "aa_run_hst_arm", "slabs")
    finally:
        gs.close()
    # a level of a Mesh through the Grid's call; the Mesh's own call takes it
    m = m2.make_mesh(m2.fixture(*MESH2D), True)
    try:
        for lev in m.lev:
            refused(L.aa_run_hst_arm(lev._h, 0.0, 1.0, -1), "aa_run_hst_arm", "Mesh", "aa_mesh_run_hst_arm")
        n, t = C.c_int(), C.c_double()
        refused(L.aa_mesh_run_hst_rows(m._h, len(m.lev), 0, None, C.byref(n), C.byref(t)), "aa_mesh_run_hst_rows", "grid")
        m.run_hst_arm(0.0, 1.0)
    finally:
        m.close()
    # a Mesh cut into slabs, and one rank's stack of slabs (aa_mesh_create_local)
    gz = m3.gold(MESH3D)
    par = aa.athinput.ParTable.from_file(orc.deck_for("blast", gz)).cmdline([str(o) for o in gz["overrides"]])
    runm = cfg.from_par(par, "blast")
    mc = lib.Mesh(cfg.levels(par, runm), 0, True, nslab=2)
    try:
        refused(L.aa_mesh_run_hst_arm(mc._h, 0.0, 1.0, -1), "aa_mesh_run_hst_arm", "slabs")
    finally:
        mc.close()
    ms = cfg.mesh_slabs(par, runm, 0, 1)
    ml = lib.Mesh(ms.levels, 0, True, links=ms.links)
    try:
        refused(L.aa_mesh_run_hst_arm(ml._h, 0.0, 1.0, -1), "aa_mesh_run_hst_arm", "aa_mesh_create_local")
    finally:
        ml.close()


@BOTH
def test_arming_does_not_outlive_one_call(strict, monkeypatch):
    monkeypatch.setenv("AA_2D_BATCH", "4")
    g = blast2d((24, 20), strict)
    try:
        n, rows, t = queued(g, FAR, 3, (0.0, 1.0e-7, None))
        assert n == 3 and len(rows[0]) == 3
        assert g.run_2d(FAR, nstep_stop=6) == 3                    # not armed: no new rows, the last call's stay readable
        again, t2 = g.run_hst_rows()
        assert again.tobytes() == rows[0].tobytes() and t2 == t
        # a refused call takes the schedule over and disarms it too: the rows are that call's, none, and the next call has none armed
        g.run_hst_arm(0.0, 1.0e-7)
        with pytest.raises(pkg("lib").AthenaError, match="tlim"):
            g.run_2d(FAR, tlim=2.0 * g.cfg.run.tlim)
        assert len(g.run_hst_rows()[0]) == 0
        assert g.run_2d(FAR, nstep_stop=8) == 2
        assert len(g.run_hst_rows()[0]) == 0
        # with nothing armed a queued step launches what it launched before: the per-step path's state
        h = blast2d((24, 20), strict)
        for _ in range(8):
            h.step()
        assert same(snapshot(g), snapshot(h))
        h.close()
    finally:
        g.close()


def test_a_1d_driver_keeps_todays_path_and_says_so_once(tmp_path):
    cfg, D, O, A = pkg("config"), pkg("driver"), pkg("outputs"), pkg("athinput")
    deck = os.path.join(DECKS, "athinput.blast1d")
    trees = {}
    for q in (True, False):
        par = A.ParTable.from_file(deck).cmdline(["domain1/Nx1=64", "time/nlim=12", "job/maxout=1"])
        d = D.Driver(cfg.from_par(par, "blast"), strict=True)
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                d.main(O.OutputSet.from_par(par, 0.0, str(tmp_path / str(q)), hst_queued=q))
            said = [str(x.message) for x in w if "hst_queued" in str(x.message)]
            assert (len(said) == 1 and "1-D" in said[0]) if q else not said, said
        finally:
            d.eng.close()
        trees[q] = {rel: _read(tmp_path / str(q), rel) for rel in _tree(str(tmp_path / str(q)))}
    assert trees[True] == trees[False] and trees[True]
