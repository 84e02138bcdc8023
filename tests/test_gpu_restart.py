"""The restart payload to and from the resident state (csrc/restart.hip: aa_rst_section_get / _put, aa_resume) and resumed runs
(Driver.from_restart, MeshRun.from_restart) on an MI355X.

Sections against download(): bit for bit, compared as uint64.  Resumed runs against the reference's resumed runs
(tests/golden/restart_*.npz, see test_restart_resume.py) and against this package's own uninterrupted runs: bit for bit."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dumpfix                                         # noqa: E402
import restartfix                                      # noqa: E402
from dumpfix import pkg                                # noqa: E402
from restartfix import RFixture                        # noqa: E402
from test_history import check_rows                    # noqa: E402

pytestmark = pytest.mark.gpu
DECKS = dumpfix.DECKS
GRIDS = [("blast", (13, 6, 5)), ("blast", (23, 9, 7)), ("ioniz_sphere", (20, 20, 20)), ("ioniz_sphere", (24, 20, 16))]
GHOST_MARK = 7e77


def _run_config(problem, nx, extra=()):
    return pkg().config.load(os.path.join(DECKS, "athinput." + problem), [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)] + list(extra), problem)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _host_sections(g, U_active, ef):
    """the sections of a Grid as slices of its downloaded block, in file order"""
    out = []
    for label, n in g.rst_sections():
        if label == "EDGEFLUX":
            a = ef
        elif label.startswith("SCALAR"):
            a = U_active[..., 5 + int(label.split()[1])]
        else:
            a = U_active[..., ["DENSITY", "1-MOMENTUM", "2-MOMENTUM", "3-MOMENTUM", "ENERGY"].index(label)]
        a = np.ascontiguousarray(a).reshape(-1)
        assert a.size == n, (label, a.size, n)
        out.append(a)
    return out


def _pattern(shape, seed):
    """doubles of every kind: ordinary values of both signs, a NaN with a payload, -0.0, a denormal, infinities"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(int(np.prod(shape))) * 10.0 ** rng.integers(-30, 30, int(np.prod(shape)))
    special = np.array([0x7ff8dead0000beef, 0x8000000000000000, 0x0000000000000123, 0x7ff0000000000000, 0xfff0000000000000,
                        0x7ff4000000001234], dtype=np.uint64).view(np.float64)
    pos = rng.choice(a.size, size=min(a.size, 4 * special.size), replace=False)
    a[pos] = np.resize(special, pos.size)
    return a.reshape(shape)


# ---- 6. rst_section against download() -----------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 100])
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("problem,nx", GRIDS)
def test_sections_equal_the_downloaded_block(problem, nx, strict, chunk, monkeypatch):
    if chunk is not None:
        monkeypatch.setenv("AA_DUMP_CHUNK_FLOATS", str(chunk))
    run = _run_config(problem, nx)
    g = pkg("lib").setup_problem(pkg().config.slab(run), 0, strict)
    g.start()
    for _ in range(2):
        g.step()
    U = g.download()
    ef = g.download_edgeflux() if run.ion else None
    secs = g.rst_sections()
    assert [s[0] for s in secs] == ["DENSITY", "1-MOMENTUM", "2-MOMENTUM", "3-MOMENTUM", "ENERGY"] + (["EDGEFLUX", "SCALAR 0"] if run.ion else [])
    if run.ion:
        assert secs[5][1] == (nx[0] + 1) * (nx[1] + 1) * (nx[2] + 1)
    for s, h in enumerate(_host_sections(g, U[4:-4, 4:-4, 4:-4], ef)):
        dev = g.rst_section(s)
        assert np.array_equal(_bits(dev), _bits(h)), (secs[s][0], int(np.count_nonzero(_bits(dev) != _bits(h))))
    assert np.array_equal(_bits(g.download()), _bits(U))                 # no state changed
    if run.ion:
        assert np.array_equal(_bits(g.download_edgeflux()), _bits(ef))
    g.close()


# ---- 7. put_rst_section: active zones only, every bit -----------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 100])
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("problem,nx", GRIDS)
def test_put_writes_active_zones_only_and_round_trips(problem, nx, strict, chunk, monkeypatch):
    if chunk is not None:
        monkeypatch.setenv("AA_DUMP_CHUNK_FLOATS", str(chunk))
    run = _run_config(problem, nx)
    g = pkg("lib").Grid(pkg().config.slab(run), 0, strict)
    blk = np.full((g.N[2], g.N[1], g.N[0], g.nvar), GHOST_MARK)
    blk[4:-4, 4:-4, 4:-4, :] = _pattern((nx[2], nx[1], nx[0], g.nvar), 1)
    g.upload(blk)
    second = [_pattern((n,), 100 + s) for s, (_label, n) in enumerate(g.rst_sections())]
    for s, a in enumerate(second):
        g.put_rst_section(s, a)
    U = g.download()
    ghost = np.ones(U.shape[:3], dtype=bool); ghost[4:-4, 4:-4, 4:-4] = False
    assert np.all(U[ghost] == GHOST_MARK)                                # no ghost zone was written
    ef = g.download_edgeflux() if run.ion else None
    for s, h in enumerate(_host_sections(g, U[4:-4, 4:-4, 4:-4], ef)):
        assert np.array_equal(_bits(h), _bits(second[s])), g.rst_sections()[s][0]
        assert np.array_equal(_bits(g.rst_section(s)), _bits(second[s])), g.rst_sections()[s][0]        # get(put(x)) == x
    g.close()


# ---- 8. a Grid cut into slabs inside the library -------------------------------------------------------------------------
@pytest.mark.parametrize("problem,nx,nslab", [("blast", (24, 16, 25), 2), ("ioniz_sphere", (24, 24, 25), 3), ("ioniz_sphere", (24, 24, 25), 2)])
def test_slabs_take_both_calls(problem, nx, nslab):
    """strict library: get gives the words of the one-slab Grid; after put (into Grids that never saw the problem generator's
    state), resume and two steps the state is the one-slab state, bit for bit"""
    lib = pkg("lib"); cfg = pkg().config
    run = _run_config(problem, nx)
    secs = {}
    for ns in (1, nslab):
        g = lib.setup_problem(cfg.slab(run), 0, True, nslab=ns)
        g.start()
        for _ in range(2):
            g.step()
        secs[ns] = ([g.rst_section(s) for s in range(len(g.rst_sections()))], g.mesh_state())
        g.close()
    assert secs[1][1] == secs[nslab][1]
    for a, b in zip(secs[1][0], secs[nslab][0]):
        assert np.array_equal(_bits(a), _bits(b))
    out = {}
    for ns in (1, nslab):
        g = lib.setup_problem(cfg.slab(run), 0, True, nslab=ns, initial=False)
        for s, a in enumerate(secs[1][0]):
            g.put_rst_section(s, a)
        g.set_mesh_state(*secs[1][1])
        g.resume()
        its = [g.step() for _ in range(2)]
        out[ns] = (g.download(), g.download_edgeflux() if run.ion else None, g.mesh_state(), its)
        g.close()
    assert out[1][2] == out[nslab][2] and out[1][3] == out[nslab][3]
    assert np.array_equal(_bits(out[1][0]), _bits(out[nslab][0]))
    if run.ion:
        assert np.array_equal(_bits(out[1][1]), _bits(out[nslab][1]))


# ---- 9. the file Driver.write_restart / MeshRun.write_restart leaves ------------------------------------------------------------
def _outputs_with_rst(par, rundir):
    par.blocks.setdefault("output1", {}).update({"out_fmt": "rst", "dt": "1e300"})
    par.blocks["job"]["maxout"] = "1"
    return pkg("outputs").OutputSet.from_par(par, 0.0, rundir)


@pytest.mark.parametrize("problem,nx", [("blast", (23, 9, 7)), ("ioniz_sphere", (20, 20, 20))])
def test_driver_restart_file_equals_the_host_writer(problem, nx, tmp_path):
    R = pkg("restart")
    par = pkg("athinput").ParTable.from_file(os.path.join(DECKS, "athinput." + problem)).cmdline([f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)])
    run = pkg().config.from_par(par, problem)
    d = pkg("driver").Driver(run)
    d.start()
    for _ in range(2):
        d.step()
    outs = _outputs_with_rst(par, str(tmp_path))
    d.write_restart(outs.rst, outs)
    ours = open(tmp_path / outs.written[-1], "rb").read()
    U = d.eng.download()[4:-4, 4:-4, 4:-4, :5 + run.nscal]
    q = str(tmp_path / "host.rst")
    R.write_rst(q, R.par_dump(outs.par), d.nstep, d.time, d.dt, U, d.eng.download_edgeflux() if run.ion else None)
    assert ours == open(q, "rb").read()
    d.eng.close()


def test_meshrun_restart_file_equals_the_host_writer(tmp_path):
    R = pkg("restart"); lib = pkg("lib"); cfg = pkg().config
    fx = dumpfix.Fixture("dump_blast_smr_16x12x8_s1")
    par = fx.par(); run = fx.run_config(par)
    mesh = lib.Mesh(cfg.levels(par, run), 0, True)
    tgt = pkg("driver").MeshRun(mesh, run)
    tgt.start()
    for _ in range(2):
        tgt.step()
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path))
    tgt.write_restart(outs.rst, outs)
    ours = open(tmp_path / outs.written[-1], "rb").read()
    q = str(tmp_path / "host.rst")
    t, dt, n = mesh.state()
    R.write_rst_levels(q, R.par_dump(outs.par), n, t, dt, [(g.download()[4:-4, 4:-4, 4:-4, :5], None) for g in mesh.lev])
    assert ours == open(q, "rb").read()
    mesh.close()


# ---- 10. resumed from the reference's seeds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["restart_blast_16x12x8_s3_s8", "restart_blast_16x12x8_s3_s11"])
def test_strict_driver_resumed_from_the_reference_seed(name, tmp_path):
    fx = RFixture(name)
    seed = fx.write_seeds(str(tmp_path / "seed"))
    d = pkg("driver").Driver.from_restart(seed, fx.resume_overrides, strict=True)
    rundir = str(tmp_path / "run")
    d.main(pkg("outputs").OutputSet.from_par(d.par, d.time, rundir))
    assert d.nstep == fx.nlim
    restartfix.compare_resumed_tree(fx, rundir, hst_rows=check_rows)
    d.eng.close()


def test_strict_mesh_resumed_from_the_reference_seed(tmp_path):
    fx = RFixture("restart_blast_smr_16x12x8_s2_s5")
    seed = fx.write_seeds(str(tmp_path / "seed"))
    m = pkg("driver").MeshRun.from_restart(seed, fx.resume_overrides, strict=True)
    assert m.restarted and m.nstep == fx.seed_nstep and len(m.mesh.lev) == 2
    rundir = str(tmp_path / "run")
    m.main(pkg("outputs").OutputSet.from_par(m.par, m.time, rundir))
    assert m.nstep == fx.nlim
    restartfix.compare_resumed_tree(fx, rundir, hst_rows=check_rows)
    m.mesh.close()


@pytest.mark.parametrize("strict,tol", [(True, 1e-9), (False, 1e-8)])
def test_sphere_resumed_from_the_reference_seed(strict, tol, tmp_path):
    """the bars of test_from_developed_reference_state: 1e-9 of each field's maximum in the strict library, 1e-8 in the default
    one; the same sub-cycle counts; dt to 1e-12"""
    fx = RFixture("restart_ioniz_sphere_24x20x16_s6_s10")
    seed = fx.write_seeds(str(tmp_path / "seed"))
    d = pkg("driver").Driver.from_restart(seed, fx.resume_overrides, strict=strict)
    rundir = str(tmp_path / "run")
    d.main(pkg("outputs").OutputSet.from_par(d.par, d.time, rundir))
    assert d.nstep == fx.nlim
    print("sub-cycles", d.niter_trace, "fixture", fx.niter)
    assert d.niter_trace == fx.niter
    restartfix.compare_resumed_tree(fx, rundir, tol=tol)
    d.eng.close()


# ---- 11. resumed equals uninterrupted, 12. resume() leaves dt alone ----------------------------------------------------------------
def _own_par(name, nx):
    fx = RFixture(name)
    fx.nx = nx
    par = fx.par()
    par.cmdline([str(o) for o in fx.z["overrides"] if str(o).startswith("domain1/x")])       # (the sphere's box)
    if fx.problem == "blast":           # the coarser Grid takes longer steps: a cadence that still fires several times after the seed
        par.cmdline(["output1/dt=0.01", "output2/dt=0.01", "output3/dt=0.005"])
    return fx, par


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("name,nx", [("restart_ioniz_sphere_24x20x16_s6_s10", (24, 20, 16)), ("restart_blast_16x12x8_s3_s8", (23, 9, 7))])
def test_resumed_equals_uninterrupted(name, nx, strict, tmp_path):
    """Driver.main to nlim; a second Driver resumed from the first one's own 0001.rst: the final state, EdgeFlux, time, dt, nstep
    and every later file are identical bit for bit -- whatever a step carries is in the file"""
    D = pkg("driver"); O = pkg("outputs")
    fx, par = _own_par(name, nx)
    run = pkg().config.from_par(par, fx.problem)
    full = str(tmp_path / "full"); res = str(tmp_path / "resumed")
    d = D.Driver(run, strict=strict)
    d.main(O.OutputSet.from_par(par, 0.0, full))
    assert d.nstep == fx.nlim
    base = par.gets("job", "problem_id")
    r = D.Driver.from_restart(os.path.join(full, base + ".0001.rst"), strict=strict)
    assert 0 < r.nstep < fx.nlim
    r.main(O.OutputSet.from_par(r.par, r.time, res))
    assert (r.time, r.dt, r.nstep) == (d.time, d.dt, d.nstep)
    assert r.niter_trace == d.niter_trace[-len(r.niter_trace):]
    assert np.array_equal(_bits(r.eng.download()), _bits(d.eng.download()))
    if run.ion:
        assert np.array_equal(_bits(r.eng.download_edgeflux()), _bits(d.eng.download_edgeflux()))
    later = [p for p in restartfix.tree(full) if p.endswith(".hst") or fx.where(p)[2] > 1]
    assert restartfix.tree(res) == later and len(later) >= 5
    for rel in later:
        a = open(os.path.join(res, rel), "rb").read(); b = open(os.path.join(full, rel), "rb").read()
        if rel.endswith(".hst"):
            rows = a.decode().splitlines()
            assert rows and b.decode().splitlines()[-len(rows):] == rows
        else:
            assert a == b, rel
    d.eng.close(); r.eng.close()


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("name,nx", [("restart_ioniz_sphere_24x20x16_s6_s10", (24, 20, 16)), ("restart_blast_16x12x8_s3_s8", (23, 9, 7))])
def test_resume_leaves_dt_alone_and_fills_the_ghost_zones(name, nx, strict, tmp_path):
    D = pkg("driver")
    fx, par = _own_par(name, nx)
    run = pkg().config.from_par(par, fx.problem)
    d = D.Driver(run, strict=strict)
    d.start()
    for _ in range(3):
        d.step()
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path))
    d.write_restart(outs.rst, outs)
    p = str(tmp_path / outs.written[-1])
    head = pkg("restart").read_head(p)
    assert head["dt"] == d.dt and head["time"] == d.time and head["nstep"] == 3
    r = D.Driver.from_restart(p, strict=strict)
    r.start()
    assert _bits(np.array([r.dt, r.eng.g.dt])).tolist() == _bits(np.array([head["dt"]] * 2)).tolist()       # the file's double, exactly
    assert (r.time, r.nstep) == (d.time, 3)
    assert np.array_equal(_bits(r.eng.download()), _bits(d.eng.download()))      # ghost zones included
    d.eng.close(); r.eng.close()
