"""Overlapped restart dumps without a GPU: dumps.OverlapWriter with a trailer and the bookkeeping of outputs.OutputSet
(overlapped_restart / poll / finish) driven by FAKE restart snapshots -- labelled float64 sections whose ready() turns true after k
polls -- so that every order of events can be scripted.  What the device does is tests/test_gpu_rst_overlap.py's."""
import io
import os
import sys
import threading
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dumpfix                     # noqa: E402
from dumpfix import Fixture, pkg    # noqa: E402

NX = (5, 3, 2)
GEOM = dict(nx=NX, minx=(-0.5, -0.25, 0.0), dx=(0.2, 0.1, 0.05), gamma=5.0 / 3.0, level=0, domain=0)
LABELS = ("DENSITY", "1-MOMENTUM", "2-MOMENTUM", "3-MOMENTUM", "ENERGY")


def _state(seed, nscal, ion, nx=NX):
    """(U of the active zones [Nx3][Nx2][Nx1][nvar], EdgeFlux [Nx3+1][Nx2+1][Nx1+1] or None)"""
    rng = np.random.default_rng(seed)
    U = rng.uniform(0.5, 2.0, size=(nx[2], nx[1], nx[0], 5 + nscal))
    U[..., 4] += 10.0
    ef = rng.uniform(0.0, 1e9, size=(nx[2] + 1, nx[1] + 1, nx[0] + 1)) if ion else None
    return U, ef


def _sections(U, ef):
    """[(label, flat float64 array)] in file order: what lib.RstSnapshot.sections returns"""
    out = [(lab, np.ascontiguousarray(U[..., c]).reshape(-1)) for c, lab in enumerate(LABELS)]
    if ef is not None:
        out.append(("EDGEFLUX", np.ascontiguousarray(ef).reshape(-1)))
    out += [("SCALAR %d" % n, np.ascontiguousarray(U[..., 5 + n]).reshape(-1)) for n in range(U.shape[-1] - 5)]
    return out


class FakeRstSnapshot:
    def __init__(self, source, sections, after, held="rst_held"):
        self.source, self._sections, self._after, self._held = source, sections, after, held
        self.polls = 0
        self.waited = self.released = False
        self.thread_of_release = None

    def ready(self):
        self.polls += 1
        return self.waited or self.polls > self._after

    def wait(self):
        self.waited = True
        return self

    def sections(self):
        assert self.waited or self.polls > self._after, "sections() before the payload is on the host"
        return self._sections

    def release(self):
        assert not self.released
        self.released = True
        self.thread_of_release = threading.get_ident()
        setattr(self.source, self._held, getattr(self.source, self._held) - 1)


class FakeGrid:
    """what OutputSet.overlapped_restart (and overlapped_dump) asks of a source; the state is a host block that `advance` changes"""
    composite = False
    RST_SLOTS = 1
    DUMP_SLOTS = 2

    def __init__(self, nscal=0, ion=False, after=1, seed=100, nx=NX):
        self.nscal, self.ion, self.after, self.seed, self.nx = nscal, ion, after, seed, nx
        self.step = 0
        self.rst_held = self.rst_max_held = 0
        self.held = 0
        self.rst_snaps, self.snaps = [], []

    def state(self):
        return _state(self.seed + self.step, self.nscal, self.ion, self.nx)

    def advance(self):
        self.step += 1

    # restart snapshots
    def rst_snapshot_bytes(self):
        return 8 * sum((a.size + 1) // 2 * 2 for _, a in _sections(*self.state()))

    def rst_snapshot(self, max_bytes):
        assert self.rst_held < self.RST_SLOTS, "a restart snapshot was asked for with the slot held"
        assert self.rst_snapshot_bytes() <= max_bytes
        self.rst_held += 1
        self.rst_max_held = max(self.rst_max_held, self.rst_held)
        s = FakeRstSnapshot(self, _sections(*self.state()), self.after)
        self.rst_snaps.append(s)
        return s

    # vtk / bin snapshots (the protocol of tests/test_dump_overlap_host.py)
    def dump_snapshot_bytes(self, fmt):
        return 4 * sum(a.size for a in pkg("dumps").payload_from_block(self.state()[0], fmt, False, GEOM["gamma"], self.nscal))

    def dump_geometry(self, prim, level=None, domain=0, time=None, dt=None):
        return dict(GEOM, prim=prim, nscal=self.nscal, time=time, dt=dt)

    def dump_snapshot(self, fmt, prim, max_bytes):
        assert self.held < self.DUMP_SLOTS
        self.held += 1
        pay = pkg("dumps").payload_from_block(self.state()[0], fmt, prim, GEOM["gamma"], self.nscal)
        s = FakeRstSnapshot(self, [np.ascontiguousarray(a).view(np.uint8).view(np.float32) for a in pay], self.after, "held")
        self.snaps.append(s)
        return s


class NoRstGrid(FakeGrid):
    """a source that must never be asked for a restart snapshot"""
    rst_snapshot = property(lambda self: (_ for _ in ()).throw(AssertionError("rst_snapshot was looked up")))
    rst_snapshot_bytes = rst_snapshot


class FakeTarget:
    """a target of OutputSet.data_output over FakeGrids (one: a Driver; several: the levels of a MeshRun, root first): overlapped
    where OutputSet has the route, else the host writers -- as driver._Runner._rst_file does it"""

    def __init__(self, grids, dt=0.125):
        self.grids, self.time, self.dt, self.nstep = list(grids), 0.0, dt, 0
        self.sync_rst = 0

    grid = property(lambda s: s.grids[0])

    def start(self):
        pass

    def step(self):
        for g in self.grids:
            g.advance()
        self.time += self.dt
        self.nstep += 1

    def write_dump(self, out, outputs):
        D = pkg("dumps")
        rel = D.fname(outputs.basename, 0, 0, out.num, out.out_fmt)
        if outputs.overlapped_dump(self.grid, rel, out.out_fmt, out.prim, time=self.time, dt=self.dt):
            return
        D.write_dump_from_block(outputs.path(rel), out.out_fmt, self.grid.state()[0],
                                **self.grid.dump_geometry(out.prim, time=self.time, dt=self.dt))

    def write_history(self, out, outputs):
        rel = outputs.basename + ".hst"
        with open(outputs.path(rel), "a") as f:
            f.write("%d %.17g %.17g\n" % (self.nstep, self.time, float(self.grid.state()[0][..., 0].sum())))

    def write_restart(self, out, outputs):
        D = pkg("dumps"); R = pkg("restart")
        rel = D.fname(outputs.basename, 0, 0, out.num, "rst")
        if getattr(outputs, "overlap_rst", False):
            if outputs.overlapped_restart(self.grids, rel, self.nstep, self.time, self.dt):
                return
        self.sync_rst += 1
        par = outputs.par
        par.blocks.setdefault("time", {})["time"] = "%e" % self.time
        par.blocks["time"]["nstep"] = "%d" % self.nstep
        R.write_rst_levels(outputs.path(rel), R.par_dump(par), self.nstep, self.time, self.dt, [g.state() for g in self.grids])


PAR = """<job>
problem_id = Fake
maxout = 4
<output1>
out_fmt = rst
dt = 0.25
<output2>
out_fmt = vtk
out = prim
dt = 0.125
<output3>
out_fmt = hst
dt = 0.125
<output4>
out_fmt = bin
dt = 0.25
"""


def _outputs(rundir, **kw):
    par = pkg("athinput").ParTable.from_text(PAR)
    return pkg("outputs").OutputSet.from_par(par, 0.0, str(rundir), **kw)


def _tree(rundir):
    return {os.path.relpath(os.path.join(dp, f), rundir): open(os.path.join(dp, f), "rb").read()
            for dp, _, fs in os.walk(rundir) for f in fs}


def _run(rundir, nlim, grids=None, **kw):
    gk = {k: kw.pop(k) for k in ("nscal", "ion", "after") if k in kw}
    grids = grids or [FakeGrid(**gk)]
    tgt = FakeTarget(grids)
    outs = _outputs(rundir, **kw)
    pkg("outputs").run(tgt, outs, 1e9, nlim)
    return tgt, outs


# ---- 1. the writer with a trailer ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [NX, (7, 5, 1)], ids=["3d", "2d"])
@pytest.mark.parametrize("ion", [False, True])
@pytest.mark.parametrize("nscal", [0, 1])
def test_writer_with_a_trailer_leaves_the_bytes_of_write_rst(nscal, ion, nx, tmp_path):
    D = pkg("dumps"); R = pkg("restart")
    U, ef = _state(1, nscal, ion, nx)
    par_text = "<job>\nproblem_id = x\n\n<par_end>\n"
    want = str(tmp_path / "sync"); got = str(tmp_path / "sub" / "over")
    R.write_rst(want, par_text, 7, 0.375, 0.01, U, ef)
    os.makedirs(tmp_path / "sub")
    head, tail = io.BytesIO(), io.BytesIO()
    R.write_header(head, par_text, 7, 0.375, 0.01)
    R.write_trailer(tail)
    pairs = _sections(U, ef)
    assert len(pairs) == 5 + nscal + (1 if ion else 0)
    done = []
    w = D.OverlapWriter()
    t = w.submit(got, head.getvalue(), [R._tag(lab) for lab, _ in pairs], [a for _, a in pairs],
                 lambda: done.append(threading.get_ident()), tail.getvalue())
    w.wait(t)
    assert done == [threading.get_ident()]
    assert open(got, "rb").read() == open(want, "rb").read()
    assert open(got, "rb").read().endswith(b"\nUSER_DATA\n")
    w.finish()
    assert sorted(os.listdir(tmp_path / "sub")) == ["over"]   # no .part left
    # ... and the five-argument call of the data dumps still writes no trailer
    t = w.submit(got, b"h", [b"t"], [np.zeros(2, dtype=np.float32)], None)
    w.finish()
    assert open(got, "rb").read() == b"ht" + bytes(8)


# ---- 2. OutputSet with fake snapshots ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("after", [0, 1, 3, 1000])
@pytest.mark.parametrize("nscal,ion", [(0, False), (1, True)])
@pytest.mark.parametrize("overlap", [False, True])
def test_overlapped_run_leaves_the_synchronous_tree(overlap, nscal, ion, after, tmp_path):
    """rst + vtk + hst + bin blocks; ready() true at once, after one poll, after three, never (only wait() brings it): the same
    files, the same bytes -- every rst file's parameter table is the one of ITS firing --, the same order of `written`, every slot
    released on the driving thread, no .part left"""
    st, sync = _run(tmp_path / "s", 5, nscal=nscal, ion=ion)
    ot, over = _run(tmp_path / "o", 5, nscal=nscal, ion=ion, after=after, overlap=overlap, overlap_rst=True)
    assert st.sync_rst >= 3 and ot.sync_rst == 0
    assert over.written == sync.written and sum(1 for p in sync.written if p.endswith(".rst")) == st.sync_rst
    a, b = _tree(str(tmp_path / "s")), _tree(str(tmp_path / "o"))
    assert sorted(a) == sorted(b) == sorted(set(sync.written))
    for rel in a:
        assert a[rel] == b[rel], rel
    g = ot.grid
    assert len(g.rst_snaps) == st.sync_rst and all(s.released for s in g.rst_snaps)
    assert {s.thread_of_release for s in g.rst_snaps} == {threading.get_ident()}
    assert g.rst_held == 0 and g.rst_max_held == 1
    assert bool(g.snaps) == overlap and g.held == 0
    over.finish()                                          # again: nothing to do


def test_the_table_is_captured_when_the_block_fires(tmp_path):
    """a payload that never gets ready before finish(), and the table changed by hand behind the firing: the file carries the table
    and the state of ITS instant"""
    A = pkg("athinput"); R = pkg("restart")
    grid = FakeGrid(after=1000)
    tgt = FakeTarget([grid])
    outs = _outputs(tmp_path, overlap_rst=True)
    outs.data_output(tgt, 1)
    assert outs.written[0] == "Fake.0000.rst" and not os.path.exists(tmp_path / "Fake.0000.rst")
    assert outs.par.blocks["output2"]["num"] == "1"
    outs.par.blocks["output2"]["num"] = "99"
    outs.par.blocks["time"]["nstep"] = "77"
    tgt.step()
    outs.finish()
    head = R.read_head(str(tmp_path / "Fake.0000.rst"))
    text = open(tmp_path / "Fake.0000.rst", "rb").read().split(b"<par_end>")[0].decode()
    par = A.ParTable.from_text(text)
    assert par.geti("output2", "num") == 1 and par.geti("time", "nstep") == 0 and par.geti("output1", "num") == 1
    assert (head["nstep"], head["time"], head["dt"]) == (0, 0.0, 0.125)
    want = str(tmp_path / "want")
    R.write_rst(want, text + "<par_end>\n", 0, 0.0, 0.125, *_state(100, 0, False))
    assert open(tmp_path / "Fake.0000.rst", "rb").read() == open(want, "rb").read()


def test_a_mesh_is_one_job_with_every_level_root_first(tmp_path):
    """two sources: one file, ready when both are; the bytes of write_rst_levels"""
    R = pkg("restart")
    root, fine = FakeGrid(after=0, seed=100), FakeGrid(after=2, seed=500, nx=(6, 4, 2))
    outs = _outputs(tmp_path, overlap_rst=True)
    assert outs.overlapped_restart([root, fine], "m.rst", 3, 0.5, 0.25)
    outs.poll(); outs.poll()
    assert not outs._inflight and root.rst_held == fine.rst_held == 1      # the root's payload alone does not make the job ready
    outs.poll()
    outs.finish()
    assert root.rst_held == fine.rst_held == 0
    want = str(tmp_path / "want")
    R.write_rst_levels(want, R.par_dump(outs.par), 3, 0.5, 0.25, [root.state(), fine.state()])
    assert open(tmp_path / "m.rst", "rb").read() == open(want, "rb").read()


# ---- 3. one slot ---------------------------------------------------------------------------------------------------------------
def test_one_slot_the_second_rst_waits_for_the_first_file(tmp_path):
    grid = FakeGrid(after=1000)
    outs = _outputs(tmp_path, overlap=True, overlap_rst=True)
    assert outs.overlapped_restart([grid], "r0.rst", 0, 0.0, 0.1)
    assert outs.overlapped_dump(grid, "d0.vtk", "vtk", True, time=0.0, dt=0.1)
    assert grid.rst_held == 1 and not os.path.exists(tmp_path / "r0.rst")
    grid.advance()
    assert outs.overlapped_restart([grid], "r1.rst", 1, 0.1, 0.1)
    first, second = grid.rst_snaps
    assert first.released and first.waited and not second.waited and grid.rst_held == 1 and grid.rst_max_held == 1
    assert os.path.exists(tmp_path / "r0.rst") and not os.path.exists(tmp_path / "r1.rst")
    assert not os.path.exists(tmp_path / "d0.vtk")         # (queued behind r0: nobody had to wait for it)
    outs.finish()
    assert sorted(os.listdir(tmp_path)) == ["d0.vtk", "r0.rst", "r1.rst"] and grid.rst_held == 0 and grid.held == 0
    assert outs.written == ["r0.rst", "d0.vtk", "r1.rst"]


def test_one_slot_run_gives_back_pressure_and_the_synchronous_tree(tmp_path):
    _, sync = _run(tmp_path / "s", 4, ion=True)
    ot, over = _run(tmp_path / "o", 4, ion=True, after=1000, overlap_rst=True)
    assert ot.grid.rst_max_held == 1 and ot.grid.rst_held == 0 and all(s.waited for s in ot.grid.rst_snaps)
    assert over.written == sync.written
    assert _tree(str(tmp_path / "s")) == _tree(str(tmp_path / "o"))


# ---- 4. errors of the writer ---------------------------------------------------------------------------------------------------
def test_writer_error_surfaces_at_the_next_poll_or_finish(tmp_path):
    grid = FakeGrid(after=0)
    tgt = FakeTarget([grid])
    outs = _outputs(tmp_path / "run", overlap_rst=True)
    outs.data_output(tgt, 1)
    outs.finish()
    assert os.path.exists(tmp_path / "run" / "Fake.0000.rst")
    os.rename(tmp_path / "run", tmp_path / "gone")
    (tmp_path / "run").write_bytes(b"")
    outs.path = lambda rel: (outs.written.append(rel), os.path.join(outs.dir, rel))[1]      # (makedirs would meet the file first)
    assert outs.overlapped_restart([grid], "x.rst", 1, 0.1, 0.1)
    with pytest.raises(OSError):
        for _ in range(1000):                              # the job is written (and fails) on the other thread: some poll meets it
            outs.poll()
            if not outs._pending and not outs._inflight:
                break
            threading.Event().wait(0.001)
        outs.finish()
    assert grid.rst_held == 0 and all(s.released for s in grid.rst_snaps)
    assert outs.overlapped_restart([grid], "y.rst", 2, 0.2, 0.1)
    with pytest.raises(OSError):
        outs.finish()                                      # ... and finish() raises it when no poll came in between
    assert grid.rst_held == 0
    outs.finish()


# ---- 5. fall-backs -------------------------------------------------------------------------------------------------------------
def _told(rec):
    return [str(w.message) for w in rec if "overlap_rst = True" in str(w.message)]


@pytest.mark.parametrize("case", ["composite", "max_bytes", "none", "no_method"])
def test_sources_without_the_route_fall_back_with_one_warning(case, tmp_path):
    grid = FakeGrid(ion=True)
    kw = {}
    if case == "composite":
        grid.composite = True
    if case == "max_bytes":
        kw["overlap_max_bytes"] = grid.rst_snapshot_bytes() - 1
    tgt = FakeTarget([grid] if case not in ("none", "no_method") else [None if case == "none" else object()])
    outs = _outputs(tmp_path / "o", overlap_rst=True, **kw)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        if case in ("none", "no_method"):
            for n in range(3):
                assert not outs.overlapped_restart(tgt.grids, "f.rst", 0, 0.0, 0.1)
            assert not outs.overlapped_restart(None, "f.rst", 0, 0.0, 0.1)
        else:
            outs.data_output(tgt, 1); tgt.step(); outs.data_output(tgt, 1)
            outs.finish()
    told = _told(rec)
    assert len(told) == 1, told
    assert {"composite": "aa_rst_section_get", "max_bytes": "overlap_max_bytes", "none": "device", "no_method": "device"}[case] in told[0]
    if case in ("composite", "max_bytes"):
        assert not grid.rst_snaps and tgt.sync_rst == 2
        st = FakeTarget([FakeGrid(ion=True)]); so = _outputs(tmp_path / "s")
        so.data_output(st, 1); st.step(); so.data_output(st, 1)
        assert so.written == outs.written and _tree(str(tmp_path / "s")) == _tree(str(tmp_path / "o"))


def test_payload_at_the_cap_takes_the_route(tmp_path):
    grid = FakeGrid(ion=True, after=0)
    outs = _outputs(tmp_path, overlap_rst=True, overlap_max_bytes=grid.rst_snapshot_bytes())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert outs.overlapped_restart([grid], "f.rst", 0, 0.0, 0.1)
        outs.finish()


def _cadence_driver():
    from test_distributed_gloo import OracleEngine
    fx = Fixture("dump_blast_cadence_16x12x8_s8")
    par = fx.par(); run = fx.run_config(par)
    return fx, par, pkg("driver").Driver(run, OracleEngine)


def test_engine_without_a_device_falls_back_with_one_warning(tmp_path):
    fx, par, d = _cadence_driver()
    assert any(p.endswith(".rst") for p in fx.paths)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path), overlap_rst=True)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        d.main(outs)
    told = _told(rec)
    assert len(told) == 1 and "no state on a device" in told[0], [str(w.message) for w in rec]
    assert not [w for w in rec if "overlap = True" in str(w.message)]      # the other switch is off and says nothing
    dumpfix.compare_tree(fx, str(tmp_path))


def test_split_dumps_keep_the_box_path_with_one_warning(tmp_path):
    """rst_ngrid: the files of the run without the switch, one warning that names the reason"""
    res = {}
    for on in (False, True):
        fx, par, d = _cadence_driver()
        rundir = str(tmp_path / ("on" if on else "off"))
        outs = pkg("outputs").OutputSet.from_par(par, 0.0, rundir, rst_ngrid=(2, 1, 2), overlap_rst=on)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            d.main(outs)
        res[on] = (outs.written, _told(rec))
    assert res[False][1] == [] and len(res[True][1]) == 1 and "rst_ngrid" in res[True][1][0], res[True][1]
    assert res[True][0] == res[False][0] and any(p.startswith("id3/") for p in res[True][0])
    assert _tree(str(tmp_path / "on")) == _tree(str(tmp_path / "off"))


def test_mesh_driver_falls_back_with_one_warning(tmp_path):
    """driver.MeshDriver (a refined mesh over ranks; here one rank with the oracle as its engine) has no overlapped route"""
    from test_mesh_driver_outputs import OutputMeshEngine
    res = {}
    for on in (False, True):
        fx = Fixture("dump_blast_smr_16x12x8_s1")
        par = fx.par(); run = fx.run_config(par)
        d = pkg("driver").MeshDriver(par, run, OutputMeshEngine)
        rundir = str(tmp_path / ("on" if on else "off"))
        outs = pkg("outputs").OutputSet.from_par(par, 0.0, rundir, overlap_rst=on)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            d.main(outs)
        res[on] = (outs.written, _told(rec))
    assert res[False][1] == [] and len(res[True][1]) == 1 and "MeshDriver" in res[True][1][0], res[True][1]
    assert res[True][0] == res[False][0] and any(p.endswith(".rst") for p in res[True][0])
    assert _tree(str(tmp_path / "on")) == _tree(str(tmp_path / "off"))


# ---- 6. defaults ---------------------------------------------------------------------------------------------------------------
def test_the_switch_defaults_to_off_and_is_independent_of_overlap(tmp_path):
    O = pkg("outputs")
    o = _outputs(".")
    assert o.overlap_rst is False and o.overlap is False
    assert _outputs(".", overlap=True).overlap_rst is False and _outputs(".", overlap_rst=True).overlap is False
    par = pkg("athinput").ParTable.from_text(PAR)
    assert O.OutputSet(par, [], None, ".", 0, 1).overlap_rst is False
    # off: nothing is asked of the source, with either spelling of "off"
    assert not o.overlapped_restart([NoRstGrid()], "f.rst", 0, 0.0, 0.1)
    assert not _outputs(".", overlap=True).overlapped_restart([NoRstGrid()], "f.rst", 0, 0.0, 0.1)
    tgt, outs = _run(tmp_path / "off", 3, grids=[NoRstGrid()], overlap=True)
    assert tgt.sync_rst >= 2 and not tgt.grid.rst_snaps
    o.poll(); o.finish()


def test_with_the_switch_off_the_driver_takes_todays_path(tmp_path):
    """Driver.write_restart with the default OutputSet: the reference's tree, no warning, through an engine that has no snapshots"""
    fx, par, d = _cadence_driver()
    assert not hasattr(d.eng, "dump_source")
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d.main(outs)
    dumpfix.compare_tree(fx, str(tmp_path))
