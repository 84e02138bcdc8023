"""Overlapped vtk / bin dumps on an MI355X: the one-pass payload kernel k_dump_payload behind aa_dump_snapshot_begin (csrc/dump.hip),
lib.Grid.dump_snapshot / lib.Snapshot, and whole runs with OutputSet(overlap=True).

The rule everywhere is equality: a snapshot's words are those of the synchronous aa_dump_section bit for bit (and the host
restatement dumps.payload_from_block's, NaN for NaN), a run with overlap leaves the synchronous run's tree byte for byte and the same
state.  No test asserts a time.  Shapes are the smallest at which the kernel's thread mapping can go wrong: a thread owns four
consecutive zones of the flat index, so n % 4 = 2, 1, 0, rows that end inside a thread's four zones, more than one block."""
import json
import os
import re
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dumpfix                     # noqa: E402
import twodfix                     # noqa: E402
from dumpfix import Fixture, pkg    # noqa: E402

pytestmark = pytest.mark.gpu
DECKS = dumpfix.DECKS
COMBOS = [(fmt, prim) for fmt in ("vtk", "bin") for prim in (False, True)]


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def _same_words_nan(dev, host, what):
    """device words against the host restatement (file dtype): NaN where the host has NaN, else the same bits"""
    host = np.ascontiguousarray(host)
    d = _words(dev); h = host.view(np.uint32).reshape(-1)
    assert d.size == h.size, (what, d.size, h.size)
    nan = np.isnan(host.reshape(-1))
    assert np.all(np.isnan(d.view(host.dtype)[nan])), what
    bad = np.nonzero((d != h) & ~nan)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {h.size} words differ, first at {int(bad[0])}"


def _snapshot_words(g, fmt, prim):
    """every section of a snapshot of the state as it is, copied out of the page-locked buffer"""
    s = g.dump_snapshot(fmt, prim)
    s.wait()
    assert s.ready()
    out = [_words(s.section(i)).copy() for i in range(s.nsections)]
    s.release()
    return out


def _section_words(g, fmt, prim):
    return [_words(g.dump_section(fmt, prim, i)).copy() for i in range(g.dump_sections(fmt))]


def _active(g, U):
    return U[4:-4, 4:-4, 4:-4] if g.ndim == 3 else U[:, 4:-4, 4:-4]


def _check_snapshot(g, run, what):
    D = pkg("dumps")
    U = _active(g, g.download())
    for fmt, prim in COMBOS:
        snap = _snapshot_words(g, fmt, prim)
        sync = _section_words(g, fmt, prim)
        host = D.payload_from_block(U, fmt, prim, run.gamma, run.nscal)
        assert len(snap) == len(sync) == len(host) == D.nsections(D.FORMATS[fmt], run.nscal)
        n = U.shape[0] * U.shape[1] * U.shape[2]
        for i, (a, b, h) in enumerate(zip(snap, sync, host)):
            w = f"{what} {fmt} prim={prim} section {i}"
            assert a.size == D.section_floats(D.FORMATS[fmt], i, n), w
            assert np.array_equal(a, b), f"{w}: {int(np.count_nonzero(a != b))} of {a.size} words differ from aa_dump_section"
            _same_words_nan(a, h, w)


def _grid(problem, nx, strict, deck=None, integrator=None):
    aa = pkg(); lib = pkg("lib")
    ov = [f"domain1/Nx{d + 1}={nx[d]}" for d in range(len(nx))]
    args = (problem,) if integrator is None else (problem, integrator)
    run = aa.config.load(os.path.join(DECKS, "athinput." + (deck or problem)), ov, *args)
    return lib.setup_problem(aa.config.slab(run), 0, strict), run


NGHOST = 4
GHOST_MARK = 7e77                  # a dump reads active zones only: this would show


def _bare_grid(problem, nx, strict):
    """a Grid of any shape without the problem generator: its state is uploaded"""
    aa = pkg(); lib = pkg("lib"); cfg = pkg("config")
    run = aa.config.load(os.path.join(DECKS, "athinput." + problem), [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)], problem)
    gc = cfg.GridConfig(run=run, rank=0, nranks=1, Nx=tuple(run.rootNx), disp=(0, 0, 0), MinX=tuple(run.xmin), bc=tuple(run.bc),
                        lx3=-1, rx3=-1)
    return lib.Grid(gc, 0, strict), run


def _stepped_grid(problem, nx, strict, deck=None):
    """(Grid holding the problem's state after two steps, run).  A 3-D Grid thinner than the ghost zones in some direction cannot
    be stepped (config.slab refuses it, as the reference does): such a shape -- they are here for the payload kernel's thread
    mapping, n % 4 and rows that end inside a thread's four zones -- takes the leading zones of the smallest Grid that can,
    after ITS two steps."""
    if len(nx) == 2 or min(nx) >= NGHOST:
        g, run = _grid(problem, nx, strict, deck)
        g.start()
        for _ in range(2):
            g.step()
        return g, run
    big, _ = _grid(problem, tuple(max(n, NGHOST) for n in nx), strict, deck)
    big.start()
    for _ in range(2):
        big.step()
    U = big.download()[4:-4, 4:-4, 4:-4][:nx[2], :nx[1], :nx[0]]
    t, dt, nstep = big.mesh_state()
    big.close()
    g, run = _bare_grid(problem, nx, strict)
    blk = np.full((g.N[2], g.N[1], g.N[0], g.nvar), GHOST_MARK)
    blk[4:-4, 4:-4, 4:-4] = U
    g.upload(blk)
    g.set_mesh_state(t, dt, nstep)
    return g, run


# ---- 1. the payload: every section, both formats, both variable sets, both libraries ---------------------------------------------
CASES = [("blast", (5, 3, 2), None),          # n = 30: a tail of 2, rows of 5 end inside a thread's four zones
         ("blast", (7, 5, 3), None),          # n = 105: a tail of 1
         ("blast", (4, 4, 4), None),          # no tail
         ("blast", (23, 9, 7), None),         # 1449 zones: two blocks, odd everything
         ("blast", (5, 7), "blast2d"),        # 2-D Grids: ks = 0, no x3 ghost zones
         ("blast", (64, 8), "blast2d"),
         ("ifront", (16, 5, 4), None),        # with the scalar
         ("ioniz_sphere", (20, 16, 12), None)]


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("problem,nx,deck", CASES, ids=["%s_%s" % (c[2] or c[0], "x".join(map(str, c[1]))) for c in CASES])
def test_snapshot_equals_the_synchronous_sections(problem, nx, deck, strict):
    g, run = _stepped_grid(problem, nx, strict, deck)
    assert tuple(g.cfg.Nx)[:len(nx)] == tuple(nx)
    before = g.download()
    _check_snapshot(g, run, f"{deck or problem} {nx} strict={strict}")
    assert np.array_equal(g.download(), before, equal_nan=True)          # a snapshot changes no state
    g.close()


@pytest.mark.parametrize("strict", [False, True])
def test_designed_state_takes_the_tiny_number_branch(strict):
    """one zone whose E is below its kinetic energy (P < 0), one with E = NaN: P becomes TINY_NUMBER in both, by the same words"""
    D = pkg("dumps")
    g, run = _bare_grid("blast", (7, 5, 3), strict)
    U = np.full((g.N[2], g.N[1], g.N[0], g.nvar), GHOST_MARK)
    act = U[4:-4, 4:-4, 4:-4]
    act[..., 0] = 1.0 + 0.01 * np.arange(105).reshape(3, 5, 7)
    act[..., 1] = 0.3 * act[..., 0]; act[..., 2] = -0.2 * act[..., 0]; act[..., 3] = 0.1 * act[..., 0]
    act[..., 4] = 0.15 + 0.07 * act[..., 0]                             # (0.07 d is the kinetic energy of that: P = 0.1)
    act[1, 2, 3, 4] = 1e-3 * 0.5 * 0.14 * act[1, 2, 3, 0]               # far below the kinetic energy
    act[2, 4, 6, 4] = np.nan                                            # the last zone: the one the tail thread holds alone
    g.upload(U)
    _check_snapshot(g, run, f"designed state strict={strict}")
    tiny = np.float32(D.TINY_NUMBER)
    P = _snapshot_words(g, "bin", True)[4].view("<f4").reshape(3, 5, 7)
    assert P[1, 2, 3] == tiny and P[2, 4, 6] == tiny and np.count_nonzero(P == tiny) == 2
    g.close()


# ---- 2. immunity: the snapshot is the instant of begin, and the run does not notice it ---------------------------------------------
@pytest.mark.parametrize("problem,nx", [("blast", (23, 9, 7)), ("ioniz_sphere", (20, 16, 12))])
def test_snapshot_is_immune_to_the_steps_behind_it_and_they_to_it(problem, nx):
    g, run = _grid(problem, nx, False)
    twin, _ = _grid(problem, nx, False)
    for x in (g, twin):
        x.start()
        for _ in range(2):
            x.step()
    then = _section_words(g, "vtk", True)
    s = g.dump_snapshot("vtk", True)
    for x in (g, twin):
        for _ in range(3):
            x.step()
    s.wait()
    got = [_words(s.section(i)).copy() for i in range(s.nsections)]
    s.release()
    now = _section_words(g, "vtk", True)
    for i, (a, b, c) in enumerate(zip(got, then, now)):
        assert np.array_equal(a, b), f"section {i}: the snapshot is not the state at begin"
        assert not np.array_equal(a, c), f"section {i}: three steps changed nothing"
    assert g.mesh_state() == twin.mesh_state()
    assert np.array_equal(g.download(), twin.download(), equal_nan=True)
    g.close(); twin.close()


# ---- 3. a snapshot between aa_integrate_begin and aa_integrate_3d_ctu ----------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("problem,ov", [("blast", ["domain1/Nx1=70", "domain1/Nx2=23", "domain1/Nx3=37"]),
                                        ("ioniz_sphere", ["domain1/Nx1=32", "domain1/Nx2=32", "domain1/Nx3=32", "problem/rp=2.1e10"])])
def test_snapshot_between_begin_and_integrate_changes_no_bit(problem, ov, strict, monkeypatch):
    """unlike aa_dump_section the snapshot does not stage through the face-state area: the sweeps of aa_integrate_begin stay
    valid and the step is the same bit for bit.  inner_swept shows in what a SECOND aa_integrate_begin does: nothing while the
    flag stands (as many sweep scopes as the run without a dump), the sweeps again behind a synchronous dump, which clears it."""
    aa = pkg(); lib = pkg("lib")
    monkeypatch.setenv("AA_FUSED_UPDATE", "1")
    monkeypatch.setenv("AA_CORRECT_ALL", "1")
    out = {}
    for mode in ("plain", "snapshot", "section"):
        run = aa.config.load(os.path.join(DECKS, "athinput." + problem), ov, problem)
        g = lib.setup_problem(aa.config.slab(run), 0, strict)
        g.start()
        g.profile_enable(True)
        for _ in range(2):
            g.integrate_begin()
            if mode == "snapshot":
                s = g.dump_snapshot("vtk", True)
            elif mode == "section":
                for i in range(g.dump_sections("vtk")):
                    g.dump_section("vtk", True, i)
            g.integrate_begin()                            # (a no-op where inner_swept still stands)
            g.integrate_3d_ctu()
            g.bvals_mhd()
            g.new_dt()
            if mode == "snapshot":
                s.wait(); s.release()
        g.sync()
        launches = {k: v[1] for k, v in g.profile().items() if not k.startswith("dump_")}
        out[mode] = (g.download(), g.mesh_state(), launches)
        g.close()
    assert out["plain"][1] == out["snapshot"][1]
    assert np.array_equal(out["plain"][0], out["snapshot"][0], equal_nan=True)
    assert out["snapshot"][2] == out["plain"][2], (out["snapshot"][2], out["plain"][2])
    assert np.array_equal(out["plain"][0], out["section"][0], equal_nan=True)
    assert out["section"][2]["sweep_x2"] == out["plain"][2]["sweep_x2"] + 2      # (what a cleared inner_swept looks like: one more per step)


# ---- 4. slots ------------------------------------------------------------------------------------------------------------------
def test_two_slots_a_third_is_refused_and_a_released_one_is_reused():
    lib = pkg("lib")
    g, run = _grid("ioniz_sphere", (20, 16, 12), False)
    g.start(); g.step()
    want = {c: _section_words(g, *c) for c in COMBOS}
    a = g.dump_snapshot("vtk", True)
    b = g.dump_snapshot("bin", False)
    assert (a.slot, b.slot) == (0, 1)
    with pytest.raises(lib.AthenaError, match="aa_dump_snapshot_begin"):
        g.dump_snapshot("vtk", False)
    a.wait(); b.wait()
    for s, c in ((a, ("vtk", True)), (b, ("bin", False))):
        for i in range(s.nsections):
            assert np.array_equal(_words(s.section(i)), want[c][i]), (c, i)
    with pytest.raises(lib.AthenaError, match="aa_dump_snapshot_section"):
        a.section(a.nsections)
    a.release()
    c = g.dump_snapshot("bin", True)                       # the freed slot, another format
    assert c.slot == 0
    c.wait()
    for i in range(c.nsections):
        assert np.array_equal(_words(c.section(i)), want[("bin", True)][i]), i
        assert np.array_equal(_words(b.section(i)), want[("bin", False)][i]), i      # the other slot is untouched
    with pytest.raises(lib.AthenaError):
        a.section(0)                                       # a released Snapshot is dead
    b.release(); c.release()
    g.close()


def test_section_before_the_payload_is_on_the_host_is_refused_or_served():
    """never blocks, never hands out memory a copy is still writing: either the named refusal or -- the copy was quick -- the words"""
    lib = pkg("lib")
    g, run = _grid("blast", (23, 9, 7), False)
    g.start()
    want = _section_words(g, "bin", False)[0]
    s = g.dump_snapshot("bin", False)
    try:
        got = _words(s.section(0)).copy()
    except lib.AthenaError as e:
        assert "aa_dump_snapshot_section" in str(e)
        got = _words(s.wait().section(0)).copy()
    assert np.array_equal(got, want)
    s.release()
    g.close()


def test_closing_a_grid_with_a_snapshot_in_flight_returns_cleanly():
    lib = pkg("lib")
    g, run = _grid("blast", (23, 9, 7), False)
    g.start(); g.step()
    s = g.dump_snapshot("vtk", True)
    g.step()
    g.close()
    with pytest.raises(lib.AthenaError):
        s.ready()
    s.release()                                            # nothing left to free: no error
    g2, _ = _grid("blast", (23, 9, 7), False)              # and the device is fine
    g2.start(); g2.step()
    _check_snapshot(g2, run, "after a close in flight")
    g2.close()


# ---- 5. whole runs -------------------------------------------------------------------------------------------------------------
def _tree(rundir):
    return {os.path.relpath(os.path.join(dp, f), rundir): open(os.path.join(dp, f), "rb").read()
            for dp, _, fs in os.walk(rundir) for f in fs}


def _same_trees(a, b):
    ta, tb = _tree(a), _tree(b)
    assert sorted(ta) == sorted(tb) and ta, (sorted(ta), sorted(tb))
    assert not [p for p in tb if p.endswith(".part")]
    for rel in ta:
        assert ta[rel] == tb[rel], f"{rel}: the overlapped run wrote other bytes"


def test_strict_driver_with_overlap_leaves_the_reference_tree(tmp_path):
    fx = Fixture("dump_blast_cadence_16x12x8_s8")
    par = fx.par(); run = fx.run_config(par)
    d = pkg("driver").Driver(run, strict=True)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path), overlap=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # no fall-back here
        d.main(outs)
    assert d.nstep == fx.nlim
    dumpfix.compare_tree(fx, str(tmp_path))
    assert sorted(set(outs.written)) == fx.paths
    d.eng.close()


def test_shipped_output_deck_overlapped_equals_synchronous(tmp_path):
    """decks/athinput.ioniz_sphere_out (rst + vtk prim) at the fixture's 20^3, three steps, default library: the same paths, the
    same bytes in every file -- rst and hst included --, the same order of `written`, the same final state"""
    fx = Fixture("dump_ioniz_sphere_20x20x20_s3")
    res = {}
    for overlap in (False, True):
        text = re.sub(r"(?m)^maxout\s*=.*$", "maxout = 3", open(os.path.join(DECKS, "athinput.ioniz_sphere_out")).read(), count=1)
        par = pkg("athinput").ParTable.from_text(text + "\n<output3>\nout_fmt = hst\ndt = 1.0\n")
        par.cmdline([f"domain1/Nx{d}=20" for d in (1, 2, 3)] + ["time/nlim=3", "output1/dt=1.0", "output2/dt=1.0"])
        run = pkg("config").from_par(par, "ioniz_sphere")
        d = pkg("driver").Driver(run)
        rundir = str(tmp_path / ("over" if overlap else "sync"))
        outs = pkg("outputs").OutputSet.from_par(par, 0.0, rundir, overlap=overlap)
        d.main(outs)
        res[overlap] = (outs.written, d.eng.download(), d.eng.download_edgeflux(), (d.time, d.dt, d.nstep))
        d.eng.close()
    assert sorted(p for p in _tree(str(tmp_path / "sync")) if not p.endswith(".hst")) == fx.paths
    _same_trees(str(tmp_path / "sync"), str(tmp_path / "over"))
    assert res[True][0] == res[False][0]
    assert res[True][3] == res[False][3]
    assert np.array_equal(res[True][1], res[False][1], equal_nan=True) and np.array_equal(res[True][2], res[False][2])


def test_mesh_run_overlapped_equals_synchronous(tmp_path):
    """every level's Grid with its own slots (lib.Mesh on the SMR fixture's deck)"""
    lib = pkg("lib"); cfg = pkg("config")
    fx = Fixture("dump_blast_smr_16x12x8_s1")
    written = {}
    for overlap in (False, True):
        par = fx.par(); run = fx.run_config(par)
        mesh = lib.Mesh(cfg.levels(par, run), 0, True)
        tgt = pkg("driver").MeshRun(mesh, run)
        rundir = str(tmp_path / ("over" if overlap else "sync"))
        outs = pkg("outputs").OutputSet.from_par(par, 0.0, rundir, overlap=overlap)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            tgt.main(outs)
        assert mesh.nstep == fx.nlim
        written[overlap] = outs.written
        mesh.close()
    assert sorted(_tree(str(tmp_path / "sync"))) == fx.paths
    _same_trees(str(tmp_path / "sync"), str(tmp_path / "over"))
    assert written[True] == written[False]


def test_2d_run_overlapped_equals_synchronous(tmp_path):
    """decks/athinput.blast2d cut to 24 x 20 with the hst + bin + vtk + rst blocks of the 2-D output fixture"""
    fx = twodfix.fixture("g2d_out_blast_24x20")
    blocks = json.loads(str(fx["blocks"]))
    ov = [str(o) for o in fx["overrides"]] + [f"job/maxout={max(int(n) for n in blocks)}"]
    for n, kv in blocks.items():
        ov += [f"output{n}/{k}={v}" for k, v in kv.items()]
    for overlap in (False, True):
        par = pkg("athinput").ParTable.from_file(os.path.join(DECKS, "athinput.blast2d")).cmdline(ov)
        run = pkg("config").from_par(par, "blast")
        assert tuple(run.rootNx) == (24, 20, 1)
        d = pkg("driver").Driver(run, strict=True)
        d.main(pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path / ("over" if overlap else "sync")), overlap=overlap))
        d.eng.close()
    assert sorted(_tree(str(tmp_path / "sync"))) == [str(p) for p in fx["paths"]]
    _same_trees(str(tmp_path / "sync"), str(tmp_path / "over"))


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_a_grid_cut_into_slabs_refuses_by_naming_the_synchronous_call():
    aa = pkg(); lib = pkg("lib")
    run = aa.config.load(os.path.join(DECKS, "athinput.blast"), ["domain1/Nx1=24", "domain1/Nx2=16", "domain1/Nx3=32"], "blast")
    g = lib.setup_problem(aa.config.slab(run), 0, True, nslab=2)
    assert g.composite
    with pytest.raises(lib.AthenaError, match="aa_dump_section"):
        g.dump_snapshot("vtk", True)
    g.dump_section("vtk", True, 0)                         # ... which works
    g.close()


def test_max_bytes_smaller_than_the_payload_is_refused():
    lib = pkg("lib")
    g, run = _grid("blast", (23, 9, 7), False)
    n = 23 * 9 * 7
    assert g.dump_snapshot_bytes("bin") == 4 * 5 * ((n + 3) // 4 * 4)
    assert g.dump_snapshot_bytes("vtk") == 4 * (2 * ((n + 3) // 4 * 4) + (3 * n + 3) // 4 * 4)
    with pytest.raises(lib.AthenaError, match="max_bytes"):
        g.dump_snapshot("bin", False, max_bytes=g.dump_snapshot_bytes("bin") - 1)
    s = g.dump_snapshot("bin", False, max_bytes=g.dump_snapshot_bytes("bin"))      # refused before the slot was taken
    assert s.slot == 0
    s.release()
    with pytest.raises(lib.AthenaError, match="format"):
        g.dump_snapshot(7, False)
    g.close()


def test_small_overlap_max_bytes_warns_once_and_leaves_the_synchronous_tree(tmp_path):
    fx = Fixture("dump_blast_cadence_16x12x8_s8")
    par = fx.par(); run = fx.run_config(par)
    d = pkg("driver").Driver(run, strict=True)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path), overlap=True, overlap_max_bytes=1000)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        d.main(outs)
    told = [str(w.message) for w in rec if "overlap = True" in str(w.message)]
    assert len(told) == 1 and "overlap_max_bytes" in told[0], told
    dumpfix.compare_tree(fx, str(tmp_path))
    d.eng.close()
