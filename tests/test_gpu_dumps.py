"""The device path of the vtk / bin data dumps (csrc/dump.hip: aa_dump_section, lib.Grid.write_dump, Driver.main) on an MI355X.

The reference is the set of files the unmodified reference executables wrote (tests/golden/dump_*.npz, see test_dumps.py), the
rule the same: byte for byte, headers included; a word that is NaN in the reference's file only has to be NaN in ours.  Where no
reference file exists for a (format, variable set) pair the checker is dumps.payload_from_block, which test_dumps.py holds against
every reference file.  Default AND strict library: the dump kernel is compiled without contraction and with IEEE division in
both, so both must give the reference's bytes."""
import importlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dumpfix                     # noqa: E402
from dumpfix import Fixture, pkg    # noqa: E402

pytestmark = pytest.mark.gpu
DECKS = dumpfix.DECKS
GHOST_MARK = 7e77                  # a dump reads active zones only: this would show


def _same_words(dev, host, what):
    """device section against its host restatement (both hold the file's words): NaN where the host has NaN, else the same bytes"""
    host = np.ascontiguousarray(host)
    db = np.ascontiguousarray(dev).view(np.uint8); hb = host.view(np.uint8)
    assert db.size == hb.size, (what, db.size, hb.size)
    nan = np.isnan(host)
    assert np.all(np.isnan(db.view(host.dtype)[nan])), what
    bad = np.nonzero((db.reshape(-1, 4) != hb.reshape(-1, 4)).any(axis=1) & ~nan)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {nan.size} words differ, first at {int(bad[0])}"


def _check_all_sections(g, U_active, gamma, nscal, what):
    D = pkg("dumps")
    for fmt in ("vtk", "bin"):
        for prim in (False, True):
            host = D.payload_from_block(U_active, fmt, prim, gamma, nscal)
            assert g.dump_sections(fmt) == len(host)
            for s, h in enumerate(host):
                _same_words(g.dump_section(fmt, prim, s), h, f"{what} {fmt} prim={prim} section {s}")


# ---- 5. every fixture state uploaded, every fixture file reproduced ---------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 100])
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("name", dumpfix.FIXTURES)
def test_device_dump_reproduces_reference_files(name, strict, chunk, tmp_path, monkeypatch):
    """chunk = 100: a bounce buffer of 100 floats per half (AA_DUMP_CHUNK_FLOATS), so that every section travels in many
    pieces of one or two rows each and pieces begin at any word -- the ragged ends of the 16-byte stores."""
    if chunk is not None:
        monkeypatch.setenv("AA_DUMP_CHUNK_FLOATS", str(chunk))
    lib = pkg("lib"); D = pkg("dumps")
    fx = Fixture(name)
    grids = {}
    checked = 0
    for rel in fx.dumps():
        rank, level, _num = fx.where(rel)
        gc = fx.grids()[(rank, level)]
        if (rank, level) not in grids:
            grids[(rank, level)] = lib.Grid(gc, 0, strict)
        g = grids[(rank, level)]
        U, time, dt = fx.state(rel)
        blk = np.full((g.N[2], g.N[1], g.N[0], g.nvar), GHOST_MARK)
        blk[4:-4, 4:-4, 4:-4, :] = U
        g.upload(blk)
        g.set_mesh_state(time, dt, 0)
        ext = rel.rsplit(".", 1)[1]
        for fmt in ("vtk", "bin"):
            for prim in (False, True):
                p = str(tmp_path / "dev")
                g.write_dump(p, fmt, prim, level=level)
                ours = open(p, "rb").read()
                if fmt == ext and prim == fx.prim_of(ext):
                    ref = fx.file(rel)                      # the reference's own file
                else:
                    q = str(tmp_path / "host")
                    D.write_dump_from_block(q, fmt, U, prim=prim, gamma=gc.run.gamma, nscal=fx.nscal, nx=gc.Nx, minx=gc.MinX,
                                            dx=tuple(gc.run.dx[d] / float(1 << level) for d in range(3)), time=time, dt=dt, level=level)
                    ref = open(q, "rb").read()
                dumpfix.compare_dump(ours, ref, gc.Nx, fx.nscal, fmt, prim, f"{name}:{rel} as {fmt} prim={prim} strict={strict}")
                checked += 1
    for g in grids.values():
        g.close()
    assert checked == 4 * len(fx.dumps())


# ---- 6. the kernel against its host restatement on states no fixture holds -------------------------------------------------
@pytest.mark.parametrize("problem,nx", [("ioniz_sphere", (20, 20, 20)), ("blast", (23, 9, 7)), ("ioniz_sphere", (50, 12, 9))])
def test_device_payload_equals_host_restatement_after_steps(problem, nx):
    aa = pkg(); lib = pkg("lib")
    run = aa.config.load(os.path.join(DECKS, "athinput." + problem), [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)], problem)
    g = lib.setup_problem(aa.config.slab(run), 0, False)
    g.start()
    for _ in range(3):
        g.step()
    U = g.download()[4:-4, 4:-4, 4:-4]
    _check_all_sections(g, U, run.gamma, run.nscal, f"{problem} {nx}")
    assert np.array_equal(g.download()[4:-4, 4:-4, 4:-4], U, equal_nan=True)          # a dump changes no state
    g.close()


# ---- 7. a Grid cut into slabs inside the library writes the same file ---------------------------------------------------------
@pytest.mark.parametrize("problem,nx,nslab", [("blast", (24, 16, 32), 2), ("ioniz_sphere", (24, 24, 25), 3)])
def test_slabs_write_the_same_file(problem, nx, nslab, tmp_path):
    aa = pkg(); lib = pkg("lib")
    files = []
    for ns in (1, nslab):
        run = aa.config.load(os.path.join(DECKS, "athinput." + problem), [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)], problem)
        g = lib.setup_problem(aa.config.slab(run), 0, True, nslab=ns)
        g.start()
        for _ in range(2):
            g.step()
        out = {}
        for fmt in ("vtk", "bin"):
            for prim in (False, True):
                p = str(tmp_path / f"s{ns}.{fmt}")
                g.write_dump(p, fmt, prim)
                out[(fmt, prim)] = open(p, "rb").read()
        files.append(out)
        g.close()
    for key in files[0]:
        a = np.frombuffer(files[0][key], dtype=np.uint8); b = np.frombuffer(files[1][key], dtype=np.uint8)
        assert a.size == b.size and a.size > 1000
        assert np.array_equal(a, b), (key, int(np.count_nonzero(a != b)))


# ---- 8. end to end: Driver.main on the strict library leaves the reference's tree ------------------------------------------------
def test_strict_driver_leaves_the_reference_tree(tmp_path):
    fx = Fixture("dump_blast_cadence_16x12x8_s8")
    par = fx.par(); run = fx.run_config(par)
    d = pkg("driver").Driver(run, strict=True)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path))
    d.main(outs)
    assert d.nstep == fx.nlim
    dumpfix.compare_tree(fx, str(tmp_path))
    d.eng.close()


def test_mesh_writes_every_level(tmp_path):
    """lib.Mesh on the SMR fixture's deck: the reference's paths (root files, lev1/Blast-lev1.NNNN.*, one rst for all levels);
    each level's dump equals the host restatement of that level's download()."""
    lib = pkg("lib"); cfg = pkg("config"); D = pkg("dumps")
    fx = Fixture("dump_blast_smr_16x12x8_s1")
    par = fx.par(); run = fx.run_config(par)
    levs = cfg.levels(par, run)
    mesh = lib.Mesh(levs, 0, True)
    tgt = pkg("driver").MeshRun(mesh, run)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path))
    tgt.main(outs)
    assert mesh.nstep == fx.nlim
    got = sorted(os.path.relpath(os.path.join(dp, f), str(tmp_path)) for dp, _, fs in os.walk(str(tmp_path)) for f in fs)
    assert got == fx.paths
    t, dt, _n = mesh.state()
    last = max(fx.where(p)[2] for p in fx.paths)
    for gc, g in zip(levs, mesh.lev):
        U = g.download()[4:-4, 4:-4, 4:-4]
        for ext in ("vtk", "bin"):
            rel = D.fname("Blast", gc.level, 0, last, ext)
            q = str(tmp_path / "host")
            D.write_dump_from_block(q, ext, U, prim=fx.prim_of(ext), gamma=run.gamma, nscal=0, nx=gc.Nx, minx=gc.MinX,
                                    dx=tuple(run.dx[d] / float(1 << gc.level) for d in range(3)), time=t, dt=dt, level=gc.level)
            dumpfix.compare_dump(open(tmp_path / rel, "rb").read(), open(q, "rb").read(), gc.Nx, 0, ext, fx.prim_of(ext), rel)
    mesh.close()


# ---- 9. a dump between aa_integrate_begin and aa_integrate_3d_ctu changes no bit of the step -----------------------------------
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("problem,ov", [("blast", ["domain1/Nx1=70", "domain1/Nx2=23", "domain1/Nx3=37"]),
                                        ("ioniz_sphere", ["domain1/Nx1=32", "domain1/Nx2=32", "domain1/Nx3=32", "problem/rp=2.1e10"])])
def test_dump_between_begin_and_integrate_changes_no_bit(problem, ov, strict, monkeypatch):
    """the dump stages through the face-state area like a download: it makes the integrator redo the sweeps of
    aa_integrate_begin (inner_swept is cleared) and must change nothing else"""
    aa = pkg(); lib = pkg("lib")
    monkeypatch.setenv("AA_FUSED_UPDATE", "1")
    monkeypatch.setenv("AA_CORRECT_ALL", "1")
    out = []
    for dump in (False, True):
        run = aa.config.load(os.path.join(DECKS, "athinput." + problem), ov, problem)
        g = lib.setup_problem(aa.config.slab(run), 0, strict)
        g.start()
        for _ in range(2):
            g.integrate_begin()
            if dump:
                for s in range(g.dump_sections("vtk")):
                    g.dump_section("vtk", True, s)
            g.integrate_3d_ctu()
            g.bvals_mhd()
            g.new_dt()
        out.append((g.download(), g.mesh_state()))
        g.close()
    assert out[0][1] == out[1][1]
    assert np.array_equal(out[0][0], out[1][0], equal_nan=True)


def test_shipped_output_deck_runs_end_to_end(tmp_path):
    """Driver.main on decks/athinput.ioniz_sphere_out (the reference's rst + vtk prim blocks), cut down to the fixture's 20^3 and
    three steps: the reference's file names and sizes; the last restart dump holds the resident state bit for bit and the last vtk
    is the host restatement of it."""
    fx = Fixture("dump_ioniz_sphere_20x20x20_s3")
    par = pkg("athinput").ParTable.from_file(os.path.join(DECKS, "athinput.ioniz_sphere_out"))
    par.cmdline([f"domain1/Nx{d}=20" for d in (1, 2, 3)] + ["time/nlim=3", "output1/dt=1.0", "output2/dt=1.0"])
    run = pkg("config").from_par(par, "ioniz_sphere")
    d = pkg("driver").Driver(run)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path))
    d.main(outs)
    got = sorted(os.listdir(tmp_path))
    assert got == fx.paths
    for rel in fx.dumps():
        assert os.path.getsize(tmp_path / rel) == len(fx.file(rel))
    U = d.eng.download()[4:-4, 4:-4, 4:-4]
    r = dumpfix.read_rst(str(tmp_path / "ioniz_sphere.0003.rst"), (20, 20, 20), 1, True)
    assert r["nstep"] == 3 and r["time"] == d.time and r["dt"] == d.dt
    assert np.array_equal(r["U"], U, equal_nan=True)
    assert np.array_equal(r["edgeflux"], d.eng.download_edgeflux())
    q = str(tmp_path / "host")
    g = d.grid
    pkg("dumps").write_dump_from_block(q, "vtk", U, prim=True, gamma=run.gamma, nscal=1, nx=g.Nx, minx=g.MinX, dx=run.dx,
                                       time=d.time, dt=d.dt)
    dumpfix.compare_dump(open(tmp_path / "ioniz_sphere.0003.vtk", "rb").read(), open(q, "rb").read(), g.Nx, 1, "vtk", True, "last vtk")
    d.eng.close()


@pytest.mark.parametrize("chunk", [None, 1500000])
def test_large_pieces_and_threaded_copy_out(chunk, monkeypatch):
    """A Grid whose sections are larger than 4 MiB: the copy from the bounce buffer to the caller's memory runs on several threads;
    with AA_DUMP_CHUNK_FLOATS = 1.5e6 the sections also travel in several 6 MB pieces of many rows each (131 x 97 x 120 zones: the
    vector section is 18 MB, rows of 131 and 393 words, so pieces start and end at odd words)."""
    if chunk is not None:
        monkeypatch.setenv("AA_DUMP_CHUNK_FLOATS", str(chunk))
    aa = pkg(); lib = pkg("lib")
    nx = (131, 97, 120)
    run = aa.config.load(os.path.join(DECKS, "athinput.blast"), [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)], "blast")
    g = lib.setup_problem(aa.config.slab(run), 0, False)
    g.start()
    g.step()
    U = g.download()[4:-4, 4:-4, 4:-4]
    _check_all_sections(g, U, run.gamma, run.nscal, f"blast {nx} chunk={chunk}")
    g.close()
