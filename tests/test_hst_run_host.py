"""History rows of a queued run, without a GPU (tests/test_gpu_hst_run.py runs the real thing):
  * csrc/time_step.h hst_row_due -- data_output(&Mesh, 0) for ONE history block behind a taken step, the rule k_history_dc and
    k_hst_row evaluate on the device and run_frame on the host -- built with the host compilers as C99 and as C++
    (fixtures/hst_rule_probe.c) and run over a scripted table whose expectations are derived by hand from main.c:519-524 and
    output.c:509-512 beside each row, and against outputs.run's own loop on a stand-in target;
  * outputs.run with ``hst_queued=True`` on a stand-in target that batches and returns rows: files, every block's t and num and
    the table a restart dump carries are those of the same stand-in stepping one at a time;
  * the warnings of the targets that keep today's path."""
import ctypes as C
import math
import os
import struct
import subprocess
import sys
import types
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import twodfix               # noqa: E402
from twodfix import pkg      # noqa: E402

SRC = os.path.join(HERE, "fixtures", "hst_rule_probe.c")
CSRC = os.path.join(twodfix.ROOT, "atmospheric-athena_amd", "csrc")
DECK = os.path.join(twodfix.DECKS, "athinput.blast2d")
INF, NAN = float("inf"), float("nan")

# id, time, nstep, tlim, nlim, t_next, dt_out -> (due, t_next behind it)
ROWS = [
    # output.c:509 time >= t fires, :511 t += dt once
    ("due_on_the_time", 0.5, 3, 1.0, -1, 0.5, 0.25, (1, 0.75)),
    ("due_past_the_time", 0.6, 3, 1.0, -1, 0.5, 0.25, (1, 0.75)),
    ("not_due_below_the_time", 0.4999, 3, 1.0, -1, 0.5, 0.25, (0, 0.5)),
    # a block far behind advances ONCE per firing and stays behind: 0.1 + 0.001, still below time
    ("lagging_block_advances_once", 0.6, 3, 1.0, -1, 0.1, 0.001, (1, 0.1 + 0.001)),
    # main.c:519 the loop has ended: data_output(0) is not reached, the forced output behind the loop writes the row
    ("loop_ends_at_tlim", 1.0, 3, 1.0, -1, 0.5, 0.25, (0, 0.5)),
    ("loop_ends_past_tlim", 1.5, 3, 1.0, -1, 0.5, 0.25, (0, 0.5)),
    ("loop_ends_at_nlim", 0.6, 7, 1.0, 7, 0.5, 0.25, (0, 0.5)),
    ("goes_on_below_nlim", 0.6, 6, 1.0, 7, 0.5, 0.25, (1, 0.75)),
    ("nlim_zero_ends_at_once", 0.6, 0, 1.0, 0, 0.5, 0.25, (0, 0.5)),
    # a NaN time: (time < tlim) is false, the loop ends
    ("nan_time_ends_the_loop", NAN, 3, 1.0, -1, 0.5, 0.25, (0, 0.5)),
    # a NaN next time never fires (NaN comparisons are false), as `time >= o.t` in outputs.data_output
    ("nan_next_time_never_fires", 0.6, 3, 1.0, -1, NAN, 0.25, (0, NAN)),
    # dt_out = 0: fires behind every step, the next time stays
    ("zero_spacing_fires_and_stays", 0.6, 3, 1.0, -1, 0.5, 0.0, (1, 0.5)),
    # the addition is one IEEE addition: 0.1 + 0.2 is not 0.3
    ("one_ieee_addition", 0.2, 3, 1.0, -1, 0.1, 0.2, (1, 0.1 + 0.2)),
]


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def build(tmp, lang):
    so = os.path.join(str(tmp), f"hst_rule_{lang}.so")
    cc = ["g++", "-x", "c++"] if lang == "cxx" else ["gcc", "-std=c99"]
    subprocess.check_call(cc + ["-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, SRC, "-o", so])
    L = C.CDLL(so)
    D, I, dp, ip = C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.probe_hst_row_due.restype = I
    L.probe_hst_row_due.argtypes = [D, I, D, I, D, dp]
    L.probe_hst_many.restype = D
    L.probe_hst_many.argtypes = [D, D, I, ip]
    return L


@pytest.fixture(scope="module", params=["c99", "cxx"])
def probe(request, tmp_path_factory):
    return build(tmp_path_factory.mktemp("hst_rule"), request.param)


def py_rule(time, nstep, tlim, nlim, t_next, dt_out):
    """outputs.run + OutputSet.data_output for one block behind a step: the loop condition, then `time >= o.t: o.t += o.dt`"""
    if not (time < tlim and (nlim < 0 or nstep < nlim)):
        return 0, t_next
    if time >= t_next:
        return 1, t_next + dt_out
    return 0, t_next


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_rule_table(probe, row):
    _, time, nstep, tlim, nlim, t_next, dt_out, want = row
    t = C.c_double(t_next)
    due = probe.probe_hst_row_due(time, nstep, tlim, nlim, dt_out, C.byref(t))
    assert due == want[0] and same(t.value, want[1]), ((due, t.value), want)
    py = py_rule(time, nstep, tlim, nlim, t_next, dt_out)
    assert due == py[0] and same(t.value, py[1]), ((due, t.value), py)


@pytest.mark.parametrize("t0,dt", [(0.0, 0.001), (0.3, 0.1), (1.0e-3, 1.0 / 3.0), (5.0, 1.0e-7)])
def test_next_time_after_many_firings_is_pythons(probe, t0, dt):
    """10000 firings: the same bits as `o.t += o.dt` 10000 times (no contraction, no extended precision)"""
    n = C.c_int()
    got = probe.probe_hst_many(t0, dt, 10000, C.byref(n))
    t = t0
    for _ in range(10000):
        t += dt
    assert n.value == 10000 and struct.pack("d", got) == struct.pack("d", t), (got, t)


def test_the_kernels_and_the_frame_call_that_function(probe):
    dc = open(os.path.join(CSRC, "history_dc.hip")).read()
    body = dc[dc.index("k_history_dc(DevGrid g"):dc.index("int launch_history_dc")]
    assert "hst_row_due(c.time, c.nstep, tlim" in body and "history_body(g, nscal, partial)" in body
    # history_body is k_history's body, the same text (hydro_kernels.hip is fingerprinted by bench.py and stays as it is)
    hk = open(os.path.join(CSRC, "hydro_kernels.hip")).read()
    k = hk[hk.index("\nk_history(DevGrid g"):]
    theirs = k[k.index("{\n") + 2:k.index("\n}\n") + 1]
    ours = dc[dc.index("// >>> k_history\n") + len("// >>> k_history\n"):dc.index("  // <<< k_history")]
    assert ours == theirs and "acc[5] += 0.5*M1*M1*d1" in ours
    # ... and the launch geometry is launch_history's
    geo = "unsigned nb = nblk(n, 256); if (nb > 1024) nb = 1024;"
    assert geo in hk[hk.index("int launch_history("):][:400] and geo in dc[dc.index("int launch_history_dc"):]
    run = open(os.path.join(CSRC, "run.hip")).read()
    row = run[run.index("k_hst_row(const Real *partial"):run.index("int hst_grid_buffers")]
    assert "hst_row_due(c.time, c.nstep, tlim" in row and "contract(off)" in row
    frame = run[run.index("int run_frame("):]
    assert "hst_row_due(*o.time, *o.nstep, tlim" in frame
    hdr = open(os.path.join(twodfix.ROOT, "include", "athena_amd.h")).read()
    for decl in ("int aa_run_hst_arm(aa_grid *g, double t_next, double dt_out, int nlim);",
                 "int aa_run_hst_rows(aa_grid *g, int cap, double *rows, int *nrows, double *t_next);",
                 "int  aa_mesh_run_hst_arm(aa_mesh *m, double t_next, double dt_out, int nlim);",
                 "int  aa_mesh_run_hst_rows(aa_mesh *m, int grid, int cap, double *rows, int *nrows, double *t_next);"):
        assert decl in hdr
    assert probe.probe_hst_sched_bytes() == 32      # two doubles, four ints: the kernels load it in two 16-byte reads


# ---- outputs.run on a stand-in target ---------------------------------------------------------------------------------------------
class _Target:
    """A target of outputs.run whose state is a function of the step count: dt wobbles around 1e-3, the nine sums follow nstep.
    batches = True: may_batch / advance(t_stop, nstep_stop, hst=) take whole stretches and apply the rule as restated above."""

    def __init__(self, tlim, batches, basename_dir):
        self.tlim, self.batches = tlim, batches
        self.time, self.nstep, self.dt = 0.0, 0, self._dt(0)
        self.calls, self.tables, self.rows, self._w = [], [], [], {}
        self.hst_asked = 0

    @staticmethod
    def _dt(n): return 1.0e-3 * (1.0 + 0.3 * math.sin(1.7 * n))
    def _sums(self): return np.array([1.0 + 0.01 * self.nstep * (q + 1) for q in range(9)])

    def start(self): pass

    def step(self):
        self.calls.append("step")
        self._one()

    def _one(self):
        self.nstep += 1; self.time += self.dt
        self.dt = min(self._dt(self.nstep), self.tlim - self.time) if self.time < self.tlim else self._dt(self.nstep)

    def may_batch(self): return self.batches
    def hst_route(self): return None

    def advance(self, t_stop, nstep_stop=None, hst=None):
        n, self.rows = 0, []
        t_next = hst[0] if hst is not None else None
        while self.time < t_stop and self.nstep != nstep_stop:
            self._one(); n += 1
            if hst is not None:
                due, t_next = py_rule(self.time, self.nstep, self.tlim, -1 if hst[2] is None else hst[2], t_next, hst[1])
                if due:
                    self.rows.append((self.time, self.dt, self._sums()))
        self.calls.append(("advance", t_stop, nstep_stop, hst, n))
        return n

    def _row(self, out, outputs, time, dt, sums):
        H = pkg("history")
        if out.n not in self._w:      # (as driver._Runner._history_row keeps one writer per block)
            self._w[out.n] = H.HistoryWriter(outputs.dir, outputs.basename, 0, 0, out.dat_fmt, num=out.num)
        self._w[out.n].dump(time, dt, sums, 2.0, 0)
        rel = os.path.relpath(self._w[out.n].path, outputs.dir)
        if rel not in outputs.written:
            outputs.written.append(rel)

    def write_history_rows(self, out, outputs):
        for time, dt, sums in self.rows:
            self._row(out, outputs, time, dt, sums)
        return len(self.rows)

    def write_history(self, out, outputs):
        self.hst_asked += 1
        self._row(out, outputs, self.time, self.dt, self._sums())

    def write_dump(self, out, outputs):
        with open(outputs.path(f"dump.{out.num:04d}.{out.out_fmt}"), "w") as f:
            f.write(f"{self.nstep} {self.time!r} {self.dt!r}\n")

    def write_restart(self, out, outputs):
        tab = {b: dict(v) for b, v in outputs.par.blocks.items() if b.startswith("output")}
        self.tables.append((self.nstep, tab))
        with open(outputs.path(f"dump.{out.num:04d}.rst"), "w") as f:
            f.write(repr(sorted((b, sorted(v.items())) for b, v in tab.items())) + f"\n{self.nstep} {self.time!r}\n")


BLOCKS = ["job/maxout=4", "output1/out_fmt=hst", "output2/out_fmt=bin", "output2/dt=0.004", "output3/out_fmt=hst", "output3/out=cons",
          "output3/dt=0.0055", "output4/out_fmt=rst", "output4/dt=0.006"]


def _run(tmp, batches, hst_queued, hst_dt, tlim=0.02, nlim=-1, target=_Target):
    O, A = pkg("outputs"), pkg("athinput")
    par = A.ParTable.from_file(DECK).cmdline(BLOCKS + [f"output1/dt={hst_dt!r}"])
    outs = O.OutputSet.from_par(par, 0.0, str(tmp), hst_queued=hst_queued)
    t = target(tlim, batches, str(tmp))
    O.run(t, outs, tlim, nlim)
    files = {rel: open(os.path.join(str(tmp), rel), "rb").read() for rel in sorted(set(outs.written))}
    blocks = [(o.n, o.t, o.num) for o in outs.outs] + [(outs.rst.n, outs.rst.t, outs.rst.num)]
    return t, outs, files, blocks


@pytest.mark.parametrize("nlim", [-1, 13], ids=["tlim", "nlim13"])
@pytest.mark.parametrize("hst_dt", [1.0e-5, 0.0025, 0.001, 1.0], ids=["every_step", "2.5_steps", "about_a_step", "beyond"])
def test_run_with_rows_from_the_target_writes_what_the_stepping_run_writes(hst_dt, nlim, tmp_path):
    ref, ro, rfiles, rblocks = _run(tmp_path / "step", False, False, hst_dt, nlim=nlim)
    assert all(c == "step" for c in ref.calls) and len(ref.calls) == ref.nstep
    got, go, gfiles, gblocks = _run(tmp_path / "queued", True, True, hst_dt, nlim=nlim)
    assert (got.time, got.dt, got.nstep) == (ref.time, ref.dt, ref.nstep)
    assert sorted(set(go.written)) == sorted(set(ro.written)) and gfiles == rfiles
    assert gblocks == rblocks                                  # every block's next time (the same bits) and number
    assert got.tables == ref.tables and len(ref.tables) >= 3   # what every restart dump carries: <outputN> num / time of all blocks
    adv = [c for c in got.calls if c != "step"]
    assert adv and all(c[3] is not None and c[3][1] == hst_dt and c[3][2] == (None if nlim < 0 else nlim) for c in adv)
    # the armed block is no stop time: with a row due behind every step the calls are still whole stretches between the OTHER blocks
    assert sum(c[4] for c in adv) > len(adv)
    # ... and it is the FIRST hst block only: the second one (<output3>) stays a stop time, written by write_history
    assert got.hst_asked > 0
    # the keyword off: today's calls, positional, no hst
    off, _, ofiles, oblocks = _run(tmp_path / "off", True, False, hst_dt, nlim=nlim)
    assert ofiles == rfiles and oblocks == rblocks and off.tables == ref.tables
    assert all(c == "step" or c[3] is None for c in off.calls)


def test_an_armed_block_does_not_cut_the_stretches(tmp_path):
    """one hst block of 1e-5 and nothing else: ONE advance() call to tlim with hst_queued, a single step per pass without"""
    O, A = pkg("outputs"), pkg("athinput")

    def go(d, hq):
        par = A.ParTable.from_file(DECK).cmdline(["job/maxout=1", "output1/out_fmt=hst", "output1/dt=1e-5"])
        outs = O.OutputSet.from_par(par, 0.0, str(d), hst_queued=hq)
        t = _Target(0.02, True, str(d))
        O.run(t, outs, 0.02, -1)
        return t, open(os.path.join(str(d), outs.written[0]), "rb").read()
    on, f_on = go(tmp_path / "on", True)
    off, f_off = go(tmp_path / "off", False)
    assert f_on == f_off and on.nstep == off.nstep
    assert [c for c in on.calls if c != "step"] == [("advance", 0.02, None, (on.calls[0][3][0], 1e-5, None), on.nstep)]
    # without: a first call to the block's time (one step), then every pass has the block overdue: t_stop <= time, a single step
    assert off.calls.count("step") == off.nstep - 1 and [c[4] for c in off.calls if c != "step"] == [1]


def test_targets_without_the_route_keep_todays_path_and_say_so_once(tmp_path):
    D = pkg("driver")

    class Refuses(_Target):
        def hst_route(self): return ("1-D", "a 1-D Grid keeps its whole loop in one launch")
    NoRoute = type("NoRoute", (), {k: v for k, v in _Target.__dict__.items() if k not in ("hst_route", "__dict__", "__weakref__")})      # another engine's target
    for cls, word in ((NoRoute, "no state on a device"), (Refuses, "1-D Grid")):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            t, outs, files, blocks = _run(tmp_path / word.split()[0], True, True, 0.0025, target=cls)
        said = [str(x.message) for x in w if "hst_queued" in str(x.message)]
        assert len(said) == 1 and word in said[0] and "stop time" in said[0], said
        assert all(c == "step" or c[3] is None for c in t.calls)
        ref, _, rfiles, rblocks = _run(tmp_path / ("ref" + word.split()[0]), False, False, 0.0025)
        assert files == rfiles and blocks == rblocks
    # the reasons of the drivers themselves (tests/test_gpu_hst_run.py asks the real 1-D Driver)
    kind, why = D.MeshDriver.hst_route(None)
    assert kind == "MeshDriver" and "ranks" in why
    kind, why = D.Driver.hst_route(types.SimpleNamespace(distributed=True))
    assert kind == "ranks" and "several ranks" in why
    kind, why = D.Driver.hst_route(types.SimpleNamespace(distributed=False, eng=object()))
    assert kind == "engine" and "no state on a device" in why
    kind, why = D.MeshRun.hst_route(types.SimpleNamespace(mesh=object()))
    assert kind == "engine"
    kind, why = D.MeshRun.hst_route(types.SimpleNamespace(mesh=types.SimpleNamespace(run_hst_arm=None, cuts=(0, 4), links=None)))
    assert kind == "slabs"
