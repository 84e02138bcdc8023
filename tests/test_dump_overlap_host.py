"""Overlapped vtk / bin dumps without a GPU: dumps.OverlapWriter (the background thread that writes the files) and the bookkeeping
of outputs.OutputSet (overlapped_dump / poll / finish) driven by FAKE snapshots -- numpy sections whose ready() turns true after k
polls -- so that every order of events can be scripted.  What the device does is tests/test_gpu_dump_overlap.py's."""
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


def _block(seed, nscal):
    rng = np.random.default_rng(seed)
    U = rng.uniform(0.5, 2.0, size=(NX[2], NX[1], NX[0], 5 + nscal))
    U[..., 4] += 10.0
    return U


class FakeSnapshot:
    def __init__(self, source, sections, after):
        self.source, self._sections, self._after = source, sections, after
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
        self.source.held -= 1


class FakeGrid:
    """what OutputSet.overlapped_dump asks of a source; the state is a host block that `advance` changes"""
    composite = False

    def __init__(self, nscal=0, slots=2, after=1):
        self.DUMP_SLOTS, self.nscal, self.after = slots, nscal, after
        self.step = 0
        self.held = 0
        self.max_held = 0
        self.snaps = []

    def block(self):
        return _block(100 + self.step, self.nscal)

    def advance(self):
        self.step += 1

    def dump_snapshot_bytes(self, fmt):
        return 4 * sum(a.size for a in pkg("dumps").payload_from_block(self.block(), fmt, False, GEOM["gamma"], self.nscal))

    def dump_geometry(self, prim, level=None, domain=0, time=None, dt=None):
        return dict(GEOM, prim=prim, nscal=self.nscal, time=time, dt=dt)

    def dump_snapshot(self, fmt, prim, max_bytes):
        assert self.held < self.DUMP_SLOTS, "a snapshot was asked for with every slot held"
        self.held += 1
        self.max_held = max(self.max_held, self.held)
        pay = pkg("dumps").payload_from_block(self.block(), fmt, prim, GEOM["gamma"], self.nscal)
        s = FakeSnapshot(self, [np.ascontiguousarray(a).view(np.uint8).view(np.float32) for a in pay], self.after)
        self.snaps.append(s)
        return s


class FakeTarget:
    """a target of OutputSet.data_output with one FakeGrid: overlapped where OutputSet has the route, else the host writer"""

    def __init__(self, grid, dt=0.125):
        self.grid, self.time, self.dt, self.nstep = grid, 0.0, dt, 0

    def start(self):
        pass

    def step(self):
        self.grid.advance()
        self.time += self.dt
        self.nstep += 1

    def write_dump(self, out, outputs):
        D = pkg("dumps")
        rel = D.fname(outputs.basename, 0, 0, out.num, out.out_fmt)
        if outputs.overlapped_dump(self.grid, rel, out.out_fmt, out.prim, time=self.time, dt=self.dt):
            return
        D.write_dump_from_block(outputs.path(rel), out.out_fmt, self.grid.block(), **self.grid.dump_geometry(out.prim, time=self.time, dt=self.dt))

    def write_history(self, out, outputs):
        raise AssertionError("no hst block here")

    def write_restart(self, out, outputs):
        raise AssertionError("no rst block here")


PAR = """<job>
problem_id = Fake
maxout = 3
<output1>
out_fmt = vtk
out = prim
dt = 0.125
<output2>
out_fmt = bin
dt = 0.25
<output3>
out_fmt = vtk
dt = 0.25
"""


def _outputs(rundir, **kw):
    par = pkg("athinput").ParTable.from_text(PAR)
    return pkg("outputs").OutputSet.from_par(par, 0.0, str(rundir), **kw)


def _tree(rundir):
    return {os.path.relpath(os.path.join(dp, f), rundir): open(os.path.join(dp, f), "rb").read()
            for dp, _, fs in os.walk(rundir) for f in fs}


# ---- 1. the writer alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nscal", [0, 1])
@pytest.mark.parametrize("prim", [False, True])
@pytest.mark.parametrize("fmt", ["vtk", "bin"])
def test_writer_leaves_the_bytes_of_write_dump(fmt, prim, nscal, tmp_path):
    D = pkg("dumps")
    U = _block(1, nscal)
    pay = D.payload_from_block(U, fmt, prim, GEOM["gamma"], nscal)
    kw = dict(GEOM, prim=prim, nscal=nscal, time=0.375, dt=0.01)
    want = str(tmp_path / "sync"); got = str(tmp_path / "sub" / "over")
    D.write_dump(want, fmt, lambda i: pay[i], **kw)
    os.makedirs(tmp_path / "sub")
    header, titles = D.dump_head(fmt, **kw)
    assert len(titles) == D.nsections(D.FORMATS[fmt], nscal)
    done = []
    w = D.OverlapWriter()
    t = w.submit(got, header, titles, pay, lambda: done.append(threading.get_ident()))
    w.wait(t)
    assert done == [threading.get_ident()]                 # on_done runs on the thread that waits, not on the worker
    assert open(got, "rb").read() == open(want, "rb").read()
    w.finish()
    w.finish()                                             # idempotent
    assert sorted(os.listdir(tmp_path / "sub")) == ["over"]   # no .part left


def test_writer_keeps_the_order_and_the_later_job_of_a_path_stays(tmp_path):
    D = pkg("dumps")
    w = D.OverlapWriter()
    order = []
    p = str(tmp_path / "f")
    for n in range(6):
        w.submit(p if n % 2 else p + str(n), b"head%d" % n, [b"t"], [np.full(3, n, dtype=np.float32)], lambda n=n: order.append(n))
    w.finish()
    assert order == list(range(6))
    assert w.pending == 0
    assert open(p, "rb").read() == b"head5t" + np.full(3, 5, dtype=np.float32).tobytes()
    assert sorted(os.listdir(tmp_path)) == ["f", "f0", "f2", "f4"]


def test_worker_error_surfaces_at_the_next_poll_and_not_later(tmp_path):
    """the target directory replaced by a file: the worker's exception is kept and re-raised in the driving thread by the next
    poll() after the job (here through wait(), which polls), once; the job's on_done has run all the same -- the slot is free"""
    D = pkg("dumps")
    (tmp_path / "dir").write_bytes(b"a file where the run directory was")
    w = D.OverlapWriter()
    done = []
    t = w.submit(str(tmp_path / "dir" / "x.vtk"), b"h", [b""], [np.zeros(2, dtype=np.float32)], lambda: done.append(1))
    t2 = w.submit(str(tmp_path / "ok.vtk"), b"h", [b""], [np.zeros(2, dtype=np.float32)], lambda: done.append(2))
    with pytest.raises(OSError):
        w.wait(t)                                          # (wait polls)
    w.wait(t2)                                             # raised once; the job behind the failure is written all the same
    assert done == [1, 2]
    assert os.path.exists(tmp_path / "ok.vtk")
    w.poll()
    w.finish()
    # ... and finish() raises it when no poll came in between
    w.submit(str(tmp_path / "dir" / "y.vtk"), b"h", [b""], [np.zeros(2, dtype=np.float32)])
    with pytest.raises(OSError):
        w.finish()
    w.finish()


# ---- 2. OutputSet with fake snapshots ------------------------------------------------------------------------------------------
def _run(rundir, nlim, **kw):
    grid = FakeGrid(**{k: kw.pop(k) for k in ("nscal", "slots", "after") if k in kw})
    tgt = FakeTarget(grid)
    outs = _outputs(rundir, **kw)
    pkg("outputs").run(tgt, outs, 1e9, nlim)
    return grid, outs


@pytest.mark.parametrize("after", [0, 1, 3, 1000])
@pytest.mark.parametrize("nscal", [0, 1])
def test_overlapped_run_leaves_the_synchronous_tree(nscal, after, tmp_path):
    """ready() true at once, after one poll, after three, never (only wait() brings it): the same files, the same bytes, the same
    order of `written`, every slot released on the driving thread, no .part left"""
    _, sync = _run(tmp_path / "s", 5, nscal=nscal)
    grid, over = _run(tmp_path / "o", 5, nscal=nscal, after=after, overlap=True)
    assert over.written == sync.written and len(sync.written) >= 10
    a, b = _tree(str(tmp_path / "s")), _tree(str(tmp_path / "o"))
    assert sorted(a) == sorted(b) == sorted(set(sync.written))
    for rel in a:
        assert a[rel] == b[rel], rel
    assert len(grid.snaps) == len(over.written) and all(s.released for s in grid.snaps)
    assert {s.thread_of_release for s in grid.snaps} == {threading.get_ident()}
    assert grid.held == 0 and grid.max_held <= 2
    over.finish()                                          # again: nothing to do


def test_snapshot_is_taken_when_the_block_fires_not_when_it_is_written(tmp_path):
    """a payload that never gets ready before finish(): every file still holds the state of ITS instant"""
    D = pkg("dumps")
    grid, over = _run(tmp_path, 3, after=1000, overlap=True, slots=100)
    nums = {}
    for rel in over.written:
        nums.setdefault(rel.rsplit(".", 1)[1], []).append(rel)
    steps = [0, 2, 3]                                      # output2, dt = 0.25: the forced dump, the one due at t = 0.25, the forced last one
    assert len(nums["bin"]) == len(steps)
    for rel, n in zip(nums["bin"], steps):
        U = _block(100 + n, 0)
        q = str(tmp_path / "host")
        D.write_dump_from_block(q, "bin", U, **dict(GEOM, prim=False, nscal=0, time=0.125 * n, dt=0.125))
        assert open(tmp_path / rel, "rb").read() == open(q, "rb").read(), rel


def test_one_slot_gives_back_pressure(tmp_path):
    """one slot, payloads that never get ready by polling: every overlapped_dump after the first must wait for the file before
    -- never two snapshots held, and still the synchronous tree"""
    _, sync = _run(tmp_path / "s", 4)
    grid, over = _run(tmp_path / "o", 4, slots=1, after=1000, overlap=True)
    assert grid.max_held == 1 and grid.held == 0
    assert all(s.waited for s in grid.snaps)
    assert over.written == sync.written
    assert _tree(str(tmp_path / "s")) == _tree(str(tmp_path / "o"))


def test_two_slots_hold_two_and_wait_for_the_third(tmp_path):
    grid = FakeGrid(after=1000)
    outs = _outputs(tmp_path, overlap=True)
    for n in range(3):
        assert outs.overlapped_dump(grid, "f%d.vtk" % n, "vtk", True, time=0.0, dt=0.0)
        assert grid.held == min(n + 1, 2)
    assert grid.snaps[0].released and grid.snaps[0].waited and not grid.snaps[1].waited
    assert os.path.exists(tmp_path / "f0.vtk") and not os.path.exists(tmp_path / "f1.vtk")
    outs.finish()
    assert sorted(os.listdir(tmp_path)) == ["f0.vtk", "f1.vtk", "f2.vtk"] and grid.held == 0


def test_writer_error_reaches_data_output(tmp_path):
    """the run directory replaced by a file after the first dump was queued: the next data_output (its poll) or, at the latest,
    the finish() of outputs.run raises in the driving thread; every slot is free afterwards"""
    grid = FakeGrid(after=0)
    tgt = FakeTarget(grid)
    outs = _outputs(tmp_path / "run", overlap=True)
    outs.data_output(tgt, 1)
    outs.finish()
    assert len(os.listdir(tmp_path / "run")) == 2           # (the two vtk blocks write the same name)
    os.rename(tmp_path / "run", tmp_path / "gone")
    (tmp_path / "run").write_bytes(b"")
    outs.dir = str(tmp_path / "run")
    outs.path = lambda rel: (outs.written.append(rel), os.path.join(outs.dir, rel))[1]      # (makedirs would meet the file first)
    tgt.step()
    with pytest.raises(OSError):
        try:
            outs.data_output(tgt, 1)
        finally:                                           # (as outputs.run does)
            outs.finish()
    assert grid.held == 0 and all(s.released for s in grid.snaps)
    outs.finish()


# ---- 3. targets without the route ------------------------------------------------------------------------------------------------
def test_engine_without_a_device_falls_back_with_one_warning(tmp_path):
    from test_distributed_gloo import OracleEngine
    fx = Fixture("dump_blast_cadence_16x12x8_s8")
    par = fx.par(); run = fx.run_config(par)
    d = pkg("driver").Driver(run, OracleEngine)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path), overlap=True)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        d.main(outs)
    told = [w for w in rec if "overlap = True" in str(w.message)]
    assert len(told) == 1 and "no state on a device" in str(told[0].message), [str(w.message) for w in rec]
    dumpfix.compare_tree(fx, str(tmp_path))


@pytest.mark.parametrize("case", ["composite", "max_bytes", "none"])
def test_sources_without_the_route_fall_back_with_one_warning(case, tmp_path):
    grid = FakeGrid()
    kw = {}
    if case == "composite":
        grid.composite = True
    if case == "max_bytes":
        kw["overlap_max_bytes"] = grid.dump_snapshot_bytes("vtk") - 1
    tgt = FakeTarget(grid)
    outs = _outputs(tmp_path / "o", overlap=True, **kw)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        if case == "none":
            for n in range(3):
                assert not outs.overlapped_dump(None, "f.vtk", "vtk", True)
        else:
            outs.data_output(tgt, 1); tgt.step(); outs.data_output(tgt, 1)
            outs.finish()
    told = [str(w.message) for w in rec if "overlap = True" in str(w.message)]
    assert len(told) == 1, told
    assert {"composite": "aa_dump_section", "max_bytes": "overlap_max_bytes", "none": "device"}[case] in told[0]
    if case != "none":
        assert not grid.snaps
        sync_grid = FakeGrid(); st = FakeTarget(sync_grid); so = _outputs(tmp_path / "s")
        so.data_output(st, 1); st.step(); so.data_output(st, 1)
        assert so.written == outs.written and _tree(str(tmp_path / "s")) == _tree(str(tmp_path / "o"))


def test_defaults_are_off():
    o = _outputs(".")
    assert o.overlap is False and o.overlap_max_bytes == 8 << 30
    assert not o.overlapped_dump(FakeGrid(), "f.vtk", "vtk", True)
    o.poll(); o.finish()
