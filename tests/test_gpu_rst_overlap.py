"""Overlapped restart dumps on an MI355X: the one-pass payload kernel k_rst_payload and the EdgeFlux copy behind
aa_rst_snapshot_begin (csrc/restart.hip), lib.Grid.rst_snapshot / lib.RstSnapshot, and whole runs with OutputSet(overlap_rst=True).

The rule everywhere is equality: a snapshot's doubles are those of the synchronous aa_rst_section_get bit for bit, a run with
overlap_rst leaves the synchronous run's tree byte for byte and the same state.  No test asserts a time.  Shapes are the smallest at
which the kernel's thread mapping can go wrong: a thread owns two consecutive doubles of the flat index, so an odd n (the one thread
that stores a single word), an odd Nx1 (pairs that straddle two rows), more than one block, 2-D Grids (ks = 0)."""
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
import restartfix                  # noqa: E402
import twodfix                     # noqa: E402
from dumpfix import Fixture, pkg    # noqa: E402
from test_gpu_restart import _own_par      # noqa: E402  (a restart fixture's deck, its cadence fit for a resumed run)

pytestmark = pytest.mark.gpu
DECKS = dumpfix.DECKS


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).reshape(-1)


def _grid(problem, nx, strict, deck=None, extra=()):
    aa = pkg(); lib = pkg("lib")
    ov = [f"domain1/Nx{d + 1}={nx[d]}" for d in range(len(nx))] + list(extra)
    run = aa.config.load(os.path.join(DECKS, "athinput." + (deck or problem)), ov, problem)
    return lib.setup_problem(aa.config.slab(run), 0, strict), run


def _stepped(problem, nx, strict, deck=None, steps=2):
    g, run = _grid(problem, nx, strict, deck)
    g.start()
    for _ in range(steps):
        g.step()
    return g, run


def _snapshot(g):
    """[(label, bits)] of a snapshot of the state as it is, copied out of the page-locked buffer"""
    s = g.rst_snapshot()
    s.wait()
    assert s.ready()
    out = [(label, _bits(a).copy()) for label, a in s.sections()]
    s.release()
    return out


def _sync_sections(g):
    return [(label, _bits(g.rst_section(i)).copy()) for i, (label, _n) in enumerate(g.rst_sections())]


def _same_sections(got, want, what):
    assert [l for l, _ in got] == [l for l, _ in want], what
    for (label, a), (_, b) in zip(got, want):
        assert a.size == b.size, (what, label, a.size, b.size)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, f"{what} {label}: {bad.size} of {a.size} doubles differ from aa_rst_section_get, first at {int(bad[0])}"


# ---- 1. the payload: every section, labels and counts, both libraries --------------------------------------------------------------
CASES = [("blast", (23, 9, 7), None),              # n = 1449 is odd: the tail thread; Nx1 odd: pairs straddle rows; two blocks
         ("blast", (16, 12, 8), None),             # even everything: three blocks, no tail
         ("blast", (24, 20), "blast2d"),           # 2-D Grids: ks = 0, no x3 ghost zones
         ("blast", (23, 9), "blast2d"),            # ... with an odd n and an odd Nx1
         ("ioniz_sphere", (20, 16, 12), None),     # the scalar; EdgeFlux filled by the short-ray path
         ("ifront", (128, 6, 5), None)]            # rays of 128 zones: the one-kernel sub-cycle leaves EdgeFlux to whoever reads it


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("problem,nx,deck", CASES, ids=["%s_%s" % (c[2] or c[0], "x".join(map(str, c[1]))) for c in CASES])
def test_snapshot_equals_the_synchronous_sections(problem, nx, deck, strict):
    g, run = _stepped(problem, nx, strict, deck)
    assert tuple(g.cfg.Nx)[:len(nx)] == tuple(nx)
    what = f"{deck or problem} {nx} strict={strict}"
    fused = bool(run.ion) and g.ion_is_fused()
    assert fused == (problem == "ifront"), what
    n = int(np.prod(nx))
    nef = int(np.prod([v + 1 for v in g.cfg.Nx]))
    labels = ["DENSITY", "1-MOMENTUM", "2-MOMENTUM", "3-MOMENTUM", "ENERGY"] + (["EDGEFLUX"] if run.ion else []) + \
             ["SCALAR %d" % i for i in range(run.nscal)]
    pad = lambda x: (x + 1) // 2 * 2      # noqa: E731
    assert g.rst_snapshot_bytes() == 8 * sum(pad(nef if l == "EDGEFLUX" else n) for l in labels), what
    g.profile_enable(True); g.profile_reset()
    snap = _snapshot(g)                    # FIRST: where the fill of EdgeFlux is still due, the snapshot has to ask for it
    g.sync()
    prof = g.profile()
    assert prof["rst_snapshot"][1] == 1 and prof.get("rst_snapshot_ef", (0.0, 0))[1] == (1 if run.ion else 0), prof
    assert prof.get("ion_finish", (0.0, 0))[1] == (1 if fused else 0), (what, prof)      # the deferred fill, done for the snapshot
    g.profile_enable(False)
    before = g.download()
    sync = _sync_sections(g)
    assert [l for l, _ in snap] == labels and [a.size for _, a in snap] == [nef if l == "EDGEFLUX" else n for l in labels], what
    _same_sections(snap, sync, what)
    # ... and against the downloaded block
    U = before[4:-4, 4:-4, 4:-4] if g.ndim == 3 else before[:, 4:-4, 4:-4]
    assert np.array_equal(dict(snap)["ENERGY"], _bits(U[..., 4])), what
    if run.ion:
        assert np.array_equal(dict(snap)["EDGEFLUX"], _bits(g.download_edgeflux())), what
        assert np.any(dict(snap)["EDGEFLUX"] != 0), what
    _same_sections(_snapshot(g), sync, what + " (again: the slot reused)")
    assert np.array_equal(_bits(g.download()), _bits(before))          # a snapshot changes no state
    g.close()


# ---- 2. immunity: the snapshot is the instant of begin, and the run does not notice it ---------------------------------------------
@pytest.mark.parametrize("problem,nx", [("blast", (23, 9, 7)), ("ioniz_sphere", (20, 16, 12)), ("ifront", (128, 6, 5))])
def test_snapshot_is_immune_to_the_steps_behind_it_and_they_to_it(problem, nx):
    g, run = _stepped(problem, nx, False)
    twin, _ = _stepped(problem, nx, False)
    s = g.rst_snapshot()
    for x in (g, twin):
        for _ in range(2):
            x.step()
    s.wait()
    got = [(label, _bits(a).copy()) for label, a in s.sections()]
    s.release()
    ref, _ = _stepped(problem, nx, False)                # the state after step 2, from a Grid that stopped there
    then = _sync_sections(ref)
    now = _sync_sections(g)
    _same_sections(got, then, f"{problem}: the snapshot is not the state at begin:")
    for (label, a), (_, c) in zip(got, now):
        if label in ("DENSITY", "1-MOMENTUM", "ENERGY"):
            assert not np.array_equal(a, c), f"{label}: two steps changed nothing"
    assert g.mesh_state() == twin.mesh_state()
    assert np.array_equal(_bits(g.download()), _bits(twin.download()))
    if run.ion:
        assert np.array_equal(_bits(g.download_edgeflux()), _bits(twin.download_edgeflux()))
    g.close(); twin.close(); ref.close()


# ---- 3. a snapshot between aa_integrate_begin and aa_integrate_3d_ctu ----------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("problem,ov", [("blast", ["domain1/Nx1=70", "domain1/Nx2=23", "domain1/Nx3=37"]),
                                        ("ioniz_sphere", ["domain1/Nx1=32", "domain1/Nx2=32", "domain1/Nx3=32", "problem/rp=2.1e10"])])
def test_snapshot_between_begin_and_integrate_changes_no_bit(problem, ov, strict, monkeypatch):
    """unlike aa_rst_section_get the snapshot does not stage through the face-state area and leaves inner_swept standing: the
    sweeps of aa_integrate_begin stay valid and the step is the same bit for bit.  inner_swept shows in what a SECOND
    aa_integrate_begin does: nothing while the flag stands (as many sweep scopes as the run without a dump), the sweeps again
    behind a synchronous rst_section, which clears it."""
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
                s = g.rst_snapshot()
            elif mode == "section":
                for i in range(len(g.rst_sections())):
                    g.rst_section(i)
            g.integrate_begin()                            # (a no-op where inner_swept still stands)
            g.integrate_3d_ctu()
            g.bvals_mhd()
            g.new_dt()
            if mode == "snapshot":
                s.wait(); s.release()
        g.sync()
        launches = {k: v[1] for k, v in g.profile().items() if not k.startswith("rst_")}      # (rst_snapshot, rst_snapshot_ef; rst_gather)
        out[mode] = (g.download(), g.mesh_state(), launches, g.profile().get("rst_snapshot", (0, 0))[1])
        g.close()
    assert out["snapshot"][3] == 2 and out["plain"][3] == 0
    assert out["plain"][1] == out["snapshot"][1]
    assert np.array_equal(_bits(out["plain"][0]), _bits(out["snapshot"][0]))
    assert out["snapshot"][2] == out["plain"][2], (out["snapshot"][2], out["plain"][2])
    assert np.array_equal(_bits(out["plain"][0]), _bits(out["section"][0]))
    assert out["section"][2]["sweep_x2"] == out["plain"][2]["sweep_x2"] + 2      # (what a cleared inner_swept looks like: one more per step)


# ---- 4. the slot ---------------------------------------------------------------------------------------------------------------
def test_one_slot_a_second_begin_is_refused_and_a_released_one_is_reused():
    lib = pkg("lib")
    g, run = _stepped("ioniz_sphere", (20, 16, 12), False, steps=1)
    assert lib.Grid.RST_SLOTS == lib.RstSnapshot.RST_SLOTS == 1
    want = _sync_sections(g)
    a = g.rst_snapshot()
    assert a.slot == 0
    with pytest.raises(lib.AthenaError, match="aa_rst_snapshot_begin.*still held"):
        g.rst_snapshot()
    a.wait()
    _same_sections([(l, _bits(x)) for l, x in a.sections()], want, "first")
    with pytest.raises(lib.AthenaError, match="aa_rst_snapshot_section"):
        a.section(a.nsections)
    g.step()
    _same_sections([(l, _bits(x)) for l, x in a.sections()], want, "held across a step")
    a.release()
    with pytest.raises(lib.AthenaError):
        a.section(0)                                       # a released snapshot is dead
    with pytest.raises(lib.AthenaError):
        a.ready()
    a.release()                                            # ... and releasing it again is nothing
    want = _sync_sections(g)
    b = g.rst_snapshot()                                   # the freed slot
    assert b.slot == 0
    _same_sections([(l, _bits(x)) for l, x in b.wait().sections()], want, "reused")
    b.release()
    g.close()


def test_section_before_the_payload_is_on_the_host_is_refused_or_served():
    """never blocks, never hands out memory a copy is still writing: either the named refusal or -- the copy was quick -- the doubles"""
    lib = pkg("lib")
    g, run = _grid("blast", (23, 9, 7), False)
    g.start()
    want = _bits(g.rst_section(0)).copy()
    s = g.rst_snapshot()
    try:
        got = _bits(s.section(0)).copy()
    except lib.AthenaError as e:
        assert "aa_rst_snapshot_section" in str(e)
        got = _bits(s.wait().section(0)).copy()
    assert np.array_equal(got, want)
    s.release()
    g.close()


def test_closing_a_grid_with_a_snapshot_in_flight_returns_cleanly():
    lib = pkg("lib")
    g, run = _stepped("ioniz_sphere", (20, 16, 12), False, steps=1)
    s = g.rst_snapshot()
    g.step()
    g.close()
    with pytest.raises(lib.AthenaError):
        s.ready()
    s.release()                                            # nothing left to free: no error
    g2, _ = _stepped("ioniz_sphere", (20, 16, 12), False, steps=1)      # and the device is fine
    _same_sections(_snapshot(g2), _sync_sections(g2), "after a close in flight")
    g2.close()


def test_a_grid_cut_into_slabs_refuses_by_naming_the_synchronous_call():
    aa = pkg(); lib = pkg("lib")
    run = aa.config.load(os.path.join(DECKS, "athinput.blast"), ["domain1/Nx1=24", "domain1/Nx2=16", "domain1/Nx3=32"], "blast")
    g = lib.setup_problem(aa.config.slab(run), 0, True, nslab=2)
    assert g.composite
    with pytest.raises(lib.AthenaError, match="aa_rst_section_get"):
        g.rst_snapshot()
    g.rst_section(0)                                       # ... which works
    g.close()


def test_max_bytes_smaller_than_the_payload_is_refused_before_the_slot_is_taken():
    lib = pkg("lib")
    g, run = _grid("blast", (23, 9, 7), False)
    n = 23 * 9 * 7
    assert g.rst_snapshot_bytes() == 8 * 5 * (n + 1)
    with pytest.raises(lib.AthenaError, match="max_bytes"):
        g.rst_snapshot(max_bytes=g.rst_snapshot_bytes() - 1)
    s = g.rst_snapshot(max_bytes=g.rst_snapshot_bytes())   # the slot is free
    assert s.slot == 0
    s.release()
    with pytest.raises(lib.AthenaError, match="format"):   # a separate entry point, not a format code of the data dumps
        g.dump_snapshot(7, False)
    g.close()


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


def test_strict_driver_with_overlap_rst_leaves_the_reference_tree(tmp_path):
    fx = Fixture("dump_blast_cadence_16x12x8_s8")
    assert any(p.endswith(".rst") for p in fx.paths)
    par = fx.par(); run = fx.run_config(par)
    d = pkg("driver").Driver(run, strict=True)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path), overlap=True, overlap_rst=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # no fall-back here
        d.main(outs)
    assert d.nstep == fx.nlim
    dumpfix.compare_tree(fx, str(tmp_path))
    assert sorted(set(outs.written)) == fx.paths
    assert d.eng.g._rst_snaps == [None]                     # (the slot given back)
    d.eng.close()


def test_shipped_output_deck_overlapped_equals_synchronous(tmp_path):
    """decks/athinput.ioniz_sphere_out (rst + vtk prim) at the fixture's 20^3, three steps, default library, overlap_rst on and off,
    with and without overlap: the same paths, the same bytes in every file, the same order of `written`, the same final state"""
    fx = Fixture("dump_ioniz_sphere_20x20x20_s3")
    res = {}
    for rst, overlap in ((False, False), (True, False), (True, True), (False, True)):
        text = re.sub(r"(?m)^maxout\s*=.*$", "maxout = 3", open(os.path.join(DECKS, "athinput.ioniz_sphere_out")).read(), count=1)
        par = pkg("athinput").ParTable.from_text(text + "\n<output3>\nout_fmt = hst\ndt = 1.0\n")
        par.cmdline([f"domain1/Nx{d}=20" for d in (1, 2, 3)] + ["time/nlim=3", "output1/dt=1.0", "output2/dt=1.0"])
        run = pkg("config").from_par(par, "ioniz_sphere")
        d = pkg("driver").Driver(run)
        rundir = str(tmp_path / f"rst{int(rst)}_ov{int(overlap)}")
        outs = pkg("outputs").OutputSet.from_par(par, 0.0, rundir, overlap=overlap, overlap_rst=rst)
        d.eng.g.profile_enable(True)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            d.main(outs)
        assert not [str(w.message) for w in rec if "True, but" in str(w.message)]      # no fall-back here
        prof = d.eng.g.profile()
        nrst = sum(1 for p in outs.written if p.endswith(".rst"))
        assert prof.get("rst_snapshot", (0.0, 0))[1] == (nrst if rst else 0), prof      # one launch per restart dump, or the
        assert (prof.get("rst_gather", (0.0, 0))[1] > 0) == (not rst), prof             # per-section gathers of today's path
        res[(rst, overlap)] = (outs.written, d.eng.download(), d.eng.download_edgeflux(), (d.time, d.dt, d.nstep), rundir)
        d.eng.close()
    base = res[(False, False)]
    assert sorted(p for p in _tree(base[4]) if not p.endswith(".hst")) == fx.paths
    assert sum(1 for p in base[0] if p.endswith(".rst")) >= 3
    for key, r in res.items():
        _same_trees(base[4], r[4])
        assert r[0] == base[0] and r[3] == base[3], key
        assert np.array_equal(_bits(r[1]), _bits(base[1])) and np.array_equal(_bits(r[2]), _bits(base[2])), key


def test_mesh_run_overlapped_equals_synchronous(tmp_path):
    """one job with the snapshot of every level, root first (lib.Mesh on the SMR fixture's deck)"""
    lib = pkg("lib"); cfg = pkg("config")
    fx = Fixture("dump_blast_smr_16x12x8_s1")
    written = {}
    for on in (False, True):
        par = fx.par(); run = fx.run_config(par)
        mesh = lib.Mesh(cfg.levels(par, run), 0, True)
        assert mesh.RST_SLOTS == 1 and mesh.rst_snapshot_bytes(1) == mesh.lev[1].rst_snapshot_bytes() > 0
        tgt = pkg("driver").MeshRun(mesh, run)
        rundir = str(tmp_path / ("over" if on else "sync"))
        outs = pkg("outputs").OutputSet.from_par(par, 0.0, rundir, overlap_rst=on)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            tgt.main(outs)
        assert mesh.nstep == fx.nlim
        written[on] = outs.written
        if on:
            s = mesh.rst_snapshot(1)                       # the per-level spelling
            _same_sections([(l, _bits(a)) for l, a in s.wait().sections()], _sync_sections(mesh.lev[1]), "Mesh.rst_snapshot(1)")
            s.release()
        mesh.close()
    assert sorted(_tree(str(tmp_path / "sync"))) == fx.paths and any(p.endswith(".rst") for p in fx.paths)
    _same_trees(str(tmp_path / "sync"), str(tmp_path / "over"))
    assert written[True] == written[False]


def test_2d_run_overlapped_equals_synchronous(tmp_path):
    """decks/athinput.blast2d cut to 24 x 20 with the hst + bin + vtk + rst blocks of the 2-D output fixture"""
    fx = twodfix.fixture("g2d_out_blast_24x20")
    blocks = json.loads(str(fx["blocks"]))
    ov = [str(o) for o in fx["overrides"]] + [f"job/maxout={max(int(n) for n in blocks)}"]
    for n, kv in blocks.items():
        ov += [f"output{n}/{k}={v}" for k, v in kv.items()]
    for on in (False, True):
        par = pkg("athinput").ParTable.from_file(os.path.join(DECKS, "athinput.blast2d")).cmdline(ov)
        run = pkg("config").from_par(par, "blast")
        assert tuple(run.rootNx) == (24, 20, 1)
        d = pkg("driver").Driver(run, strict=True)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            d.main(pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path / ("over" if on else "sync")), overlap_rst=on))
        assert not [str(w.message) for w in rec if "True, but" in str(w.message)]      # no fall-back here
        assert (getattr(d.eng.g, "_rst_snaps", None) == [None]) == on                  # ... the route was taken, the slot is back
        d.eng.close()
    paths = [str(p) for p in fx["paths"]]
    assert sorted(_tree(str(tmp_path / "sync"))) == paths and any(p.endswith(".rst") for p in paths)
    _same_trees(str(tmp_path / "sync"), str(tmp_path / "over"))


def test_small_overlap_max_bytes_warns_once_and_leaves_the_synchronous_tree(tmp_path):
    fx = Fixture("dump_blast_cadence_16x12x8_s8")
    par = fx.par(); run = fx.run_config(par)
    d = pkg("driver").Driver(run, strict=True)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path), overlap_rst=True, overlap_max_bytes=1000)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        d.main(outs)
    told = [str(w.message) for w in rec if "overlap_rst = True" in str(w.message)]
    assert len(told) == 1 and "overlap_max_bytes" in told[0], told
    dumpfix.compare_tree(fx, str(tmp_path))
    d.eng.close()


# ---- 6. resumed from a file written overlapped ---------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("name,nx", [("restart_ioniz_sphere_24x20x16_s6_s10", (24, 20, 16)), ("restart_blast_16x12x8_s3_s8", (23, 9, 7))])
def test_resumed_from_an_overlapped_file_equals_the_uninterrupted_run(name, nx, strict, tmp_path):
    """Driver.main to the fixture's end with overlap_rst; a second Driver resumed from that run's 0001.rst and continued to the same
    end: the final state, EdgeFlux, time, dt, nstep and every later file are identical bit for bit"""
    D = pkg("driver"); O = pkg("outputs")
    fx, par = _own_par(name, nx)
    run = pkg().config.from_par(par, fx.problem)
    full = str(tmp_path / "full"); res = str(tmp_path / "resumed")
    d = D.Driver(run, strict=strict)
    d.main(O.OutputSet.from_par(par, 0.0, full, overlap_rst=True))
    assert d.nstep == fx.nlim and d.eng.g._rst_snaps == [None]              # (the route was taken, the slot is back)
    base = par.gets("job", "problem_id")
    r = D.Driver.from_restart(os.path.join(full, base + ".0001.rst"), strict=strict)
    assert 0 < r.nstep < fx.nlim
    r.main(O.OutputSet.from_par(r.par, r.time, res, overlap_rst=True))
    assert (r.time, r.dt, r.nstep) == (d.time, d.dt, d.nstep)
    assert r.niter_trace == d.niter_trace[-len(r.niter_trace):]
    assert np.array_equal(_bits(r.eng.download()), _bits(d.eng.download()))
    if run.ion:
        assert np.array_equal(_bits(r.eng.download_edgeflux()), _bits(d.eng.download_edgeflux()))
    later = [p for p in restartfix.tree(full) if not p.endswith(".hst") and fx.where(p)[2] > 1]
    assert later and any(p.endswith(".rst") for p in later)
    for rel in later:
        assert open(os.path.join(res, rel), "rb").read() == open(os.path.join(full, rel), "rb").read(), rel
    d.eng.close(); r.eng.close()
