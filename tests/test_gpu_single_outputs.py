"""The device path of the single-variable outputs (csrc/outdata.hip: aa_outdata, aa_outdata_gray; lib.Grid.outdata; Driver.main with
OutputSet.from_par(single=True)) on an MI355X.  Every comparison is byte for byte (files against the reference's,
tests/golden/single_*.npz) or bit for bit (payload, minimum, maximum and gray bytes against the numpy restatement over the
downloaded state), in the default AND the strict library: the kernels are compiled without contraction and with IEEE division in
both."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import singlefix                                              # noqa: E402
from singlefix import Fixture, pkg                            # noqa: E402

pytestmark = pytest.mark.gpu
NG = 4
EXPRS = ["d", "M1", "M2", "M3", "E", "V1", "V2", "V3", "P", "cs2"]


def _upload(d, U_active):
    """the fixture's state into the Driver's Grid, ghost zones by the boundary conditions on the device"""
    g = d.eng.g
    blk = g.new_host_block()
    sl = tuple(slice(NG, -NG) if n > 1 else slice(None) for n in blk.shape[:3])
    blk[sl + (slice(0, U_active.shape[-1]),)] = U_active
    g.upload(blk)
    g.bvals_mhd()


# ---- 1. files, byte for byte ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("name", singlefix.HYDRO)
def test_files_from_the_fixture_states(name, strict, tmp_path):
    """every output time of the fixture: its state on the device, the blocks written by Driver.write_single"""
    fx = Fixture(name)
    par = fx.par(); run = fx.run_config(par)
    d = pkg("driver").Driver(run, strict=strict)
    try:
        outs = fx.outputs(tmp_path, par)
        for num in fx.nums():
            st, d.time = fx.state(num)
            _upload(d, st["U"][..., :5])
            for o in outs.outs:
                o.num = num
                d.write_single(o, outs)
        singlefix.compare_singles(fx, tmp_path)
    finally:
        d.eng.close()


@pytest.mark.parametrize("name", singlefix.HYDRO + [singlefix.SPHERE])
def test_strict_driver_main_leaves_the_reference_files(name, tmp_path):
    """Driver.main from the problem generator over the fixture's steps: the names, the count and the bytes of every file (the
    restart dumps: their names)"""
    fx = Fixture(name)
    par = fx.par(); run = fx.run_config(par)
    d = pkg("driver").Driver(run, strict=True)
    try:
        d.main(fx.outputs(tmp_path, par))
        assert d.nstep == fx.nlim
        assert singlefix.tree(tmp_path) == fx.paths
        singlefix.compare_singles(fx, tmp_path)
    finally:
        d.eng.close()


@pytest.mark.parametrize("strict", [True, False])
def test_flux_from_the_fixture_edgeflux(strict):
    fx = Fixture(singlefix.SPHERE)
    lib = pkg("lib"); D = pkg("dumps")
    run = fx.run_config()
    g = lib.setup_problem(pkg("config").slab(run), 0, strict)
    try:
        for num in fx.nums():
            st, time = fx.state(num)
            ef = np.ascontiguousarray(st["ef"])
            g._chk(g.L.aa_upload_edgeflux(g._h, lib._dp(ef)))
            data, dmin, dmax = g.outdata("flux")
            want = ef[:-1, :-1, :-1]
            assert data.tobytes() == np.ascontiguousarray(want).tobytes()
            assert (dmin, dmax) == D.minmax(want)
            b = D.single_vtk_bytes(data, "flux", nx=run.rootNx, minx=run.xmin, dx=run.dx, raw_reduce=(0, 0, 0), time=time)
            assert b == fx.file("ioniz_sphere.%04d.flux.vtk" % num)
    finally:
        g.close()


# ---- 2. the C-ABI on a designed state -------------------------------------------------------------------------------------------------
def _designed(g, seed):
    rng = np.random.default_rng(seed)
    U = g.new_host_block()
    sh = U.shape[:3]
    U[..., 0] = rng.uniform(0.5, 2.0, sh)
    for c in (1, 2, 3):
        U[..., c] = rng.uniform(-1.0, 1.0, sh)
    U[..., 2][rng.random(sh) < 0.3] = 0.0            # zeros of either sign: the minimum / maximum keep the LAST of equals
    U[..., 2][rng.random(sh) < 0.3] = -0.0
    U[..., 4] = rng.uniform(2.0, 5.0, sh)
    U[..., 3] *= 1.0e3                               # sums whose rounding depends on the order
    if U.shape[-1] > 5:
        U[..., 5] = 0.5
    return U


def _cases(Nx):
    """(reduce, lo, hi): nothing reduced, each direction alone, each pair; ranges of one zone, of several, reaching into the ghost
    zones on either side, over the whole extent"""
    dirs = [a for a in range(3) if Nx[a] > 1]
    rngs = {a: [(0, Nx[a] - 1), (Nx[a] - 1 + NG, Nx[a] - 1 + NG), (-NG, 1), (2, min(5, Nx[a] - 1))] for a in dirs}
    out = [((0, 0, 0), (0, 0, 0), (0, 0, 0))]
    for a in dirs:
        for r in rngs[a]:
            red, lo, hi = [0, 0, 0], [0, 0, 0], [0, 0, 0]
            red[a], lo[a], hi[a] = 1, r[0], r[1]
            out.append((tuple(red), tuple(lo), tuple(hi)))
    for a in dirs:
        for b in dirs:
            if a < b:
                for ra, rb in ((rngs[a][3], rngs[b][0]), (rngs[a][1], rngs[b][2])):
                    red, lo, hi = [0, 0, 0], [0, 0, 0], [0, 0, 0]
                    red[a], lo[a], hi[a] = 1, ra[0], ra[1]
                    red[b], lo[b], hi[b] = 1, rb[0], rb[1]
                    out.append((tuple(red), tuple(lo), tuple(hi)))
    return out


@pytest.mark.parametrize("chunk", [None, "512"])
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("deck,nx", [("blast", (130, 9, 7)), ("blast2d", (130, 11, 1))])
def test_payload_minmax_and_gray_equal_numpy(deck, nx, strict, chunk, monkeypatch):
    """Nx1 = 130: two full waves and a tail of two lanes.  chunk: the payload in pieces of 256 doubles through the bounce buffer"""
    if chunk:
        monkeypatch.setenv("AA_DUMP_CHUNK_FLOATS", chunk)
    lib = pkg("lib"); cfg = pkg("config"); D = pkg("dumps")
    run = cfg.load(os.path.join(singlefix.DECKS, "athinput." + deck), [f"domain1/Nx{a + 1}={nx[a]}" for a in range(3) if nx[a] > 1], "blast")
    g = lib.Grid(cfg.slab(run), 0, strict)
    try:
        g.upload(_designed(g, 7))
        U = g.download()
        first = [NG if n > 1 else 0 for n in nx]
        for ex in EXPRS:
            V = D.expr_from_block(U, ex, run.gamma)
            for red, lo, hi in _cases(nx) if ex in ("d", "M2", "M3", "P", "cs2", "V1") else _cases(nx)[:2]:
                what = f"{ex} reduce={red} lo={lo} hi={hi}"
                data, dmin, dmax = g.outdata(ex, red, lo, hi)
                full_lo = [lo[a] if red[a] else 0 for a in range(3)]
                full_hi = [hi[a] if red[a] else nx[a] - 1 for a in range(3)]
                want = D.outdata_from_values(V, first, red, full_lo, full_hi)
                assert data.shape == want.shape, what
                assert data.tobytes() == want.tobytes(), what
                wmin, wmax = D.minmax(want)
                assert np.float64(dmin).tobytes() == np.float64(wmin).tobytes(), (what, dmin, wmin)
                assert np.float64(dmax).tobytes() == np.float64(wmax).tobytes(), (what, dmax, wmax)
                shape = pkg("outputs").payload_shape(red, nx)
                if len(shape) == 2:
                    for lo_, hi_ in ((dmin, dmax), (0.5 * (dmin + dmax), dmax), (dmin, dmin)):
                        gray = g.outdata_gray(ex, red, lo, hi, lo_, hi_)
                        assert gray.tobytes() == D.pgm_gray(want.reshape(shape), lo_, hi_).tobytes(), (what, lo_, hi_)
        assert np.array_equal(g.download(), U)                       # the calls change no state
    finally:
        g.close()


# ---- 3. refusals, the state untouched -------------------------------------------------------------------------------------------------
def _refused(g, match):
    lib = pkg("lib")
    before = g.download()
    for call in (lambda: g.outdata("d"), lambda: g.outdata_gray("d", (0, 0, 1), (0, 0, 0), (0, 0, 0), 0.0, 1.0)):
        with pytest.raises(lib.AthenaError, match=match):
            call()
    assert np.array_equal(g.download(), before, equal_nan=True)


def test_refusals(monkeypatch):
    lib = pkg("lib"); cfg = pkg("config")
    # a level of a Mesh (root and patch)
    import dumpfix
    fx = dumpfix.Fixture("dump_blast_smr_16x12x8_s1")
    par = fx.par(); run = fx.run_config(par)
    mesh = lib.Mesh(cfg.levels(par, run), 0, True)
    try:
        for g in mesh.lev:
            _refused(g, "level of a Mesh")
    finally:
        mesh.close()
    # a 1-D Grid
    run1 = cfg.load(os.path.join(singlefix.DECKS, "athinput.blast1d"), ["domain1/Nx1=24"], "blast")
    g1 = lib.setup_problem(cfg.slab(run1), 0, True)
    try:
        _refused(g1, "1-D Grid")
    finally:
        g1.close()
    # a range outside the arrays, an unknown expression, flux without a radiation plane; then a Grid cut into slabs
    run3 = cfg.load(os.path.join(singlefix.DECKS, "athinput.blast"), [f"domain1/Nx{a + 1}={n}" for a, n in enumerate((24, 20, 16))], "blast")
    g = lib.setup_problem(cfg.slab(run3), 0, True)
    try:
        before = g.download()
        for args, match in ((("d", (0, 0, 1), (0, 0, 0), (0, 0, 16 + NG)), "zones 0 .. 20 along x3"),
                            (("d", (1, 0, 0), (-NG - 1, 0, 0), (0, 0, 0)), "along x1"),
                            (("d", (0, 1, 0), (0, 3, 0), (0, 2, 0)), "along x2"),
                            ((11, (0, 0, 0), (0, 0, 0), (0, 0, 0)), "expression code 11"),
                            (("flux", (0, 0, 0), (0, 0, 0), (0, 0, 0)), "radiation plane")):
            with pytest.raises(lib.AthenaError, match=match):
                g.outdata(*args)
        with pytest.raises(lib.AthenaError, match="2-D slice"):
            g.outdata_gray("d", (0, 0, 0), (0, 0, 0), (0, 0, 0), 0.0, 1.0)
        assert np.array_equal(g.download(), before)
    finally:
        g.close()
    monkeypatch.setenv("AA_SLAB_DEVICES", "0,0")
    gs = lib.setup_problem(cfg.slab(run3), 0, True, nslab=2)
    try:
        _refused(gs, "cut into slabs")
        outs = pkg("outputs").OutputSet.from_par(Fixture("single_blast_16x12x8_s2").par(), 0.0, ".", single=True)
        d = pkg("driver").Driver.__new__(pkg("driver").Driver)
        d.nranks, d.run = 1, run3
        d.eng = type("E", (), {"g": gs})()
        assert "slabs" in d.single_route(outs)
    finally:
        gs.close()


# ---- 4. a queued stretch stops at a single-variable output time ------------------------------------------------------------------
def test_queued_run_writes_the_same_files(tmp_path, monkeypatch):
    """run_3d with four steps per read-back against the per-step loop: output times a few steps apart, inside the stretches"""
    monkeypatch.setenv("AA_CORRECT_ALL", "1")
    blocks = ["out_fmt = vtk\nout = P\nid = P\ndt = 0.011\nx3 = 0.0", "out_fmt = tab\nout = V2\nid = V2\ndt = 0.017\nx1 = 0.1\nx3 = -0.2:0.2",
              "out_fmt = pgm\nout = d\nid = d\ndt = 0.011\nx2 = 0.3"]
    text = open(os.path.join(singlefix.DECKS, "athinput.blast")).read().replace("maxout      = 0", "maxout      = 3")
    for n, body in enumerate(blocks, 1):
        text += f"\n<output{n}>\n{body}\n"
    trees = {}
    for batch in ("4", "0"):
        monkeypatch.setenv("AA_3D_BATCH", batch)
        par = pkg("athinput").ParTable.from_text(text).cmdline(["domain1/Nx1=24", "domain1/Nx2=20", "domain1/Nx3=16", "time/nlim=14"])
        run = pkg("config").from_par(par, "blast")
        d = pkg("driver").Driver(run, strict=True)
        rundir = tmp_path / batch
        try:
            assert d.eng.g.run_3d_batch() == int(batch)
            d.main(pkg("outputs").OutputSet.from_par(par, 0.0, str(rundir), single=True))
            assert d.nstep == 14
        finally:
            d.eng.close()
        trees[batch] = {rel: open(os.path.join(str(rundir), rel), "rb").read() for rel in singlefix.tree(rundir)}
    assert sorted(trees["4"]) == sorted(trees["0"]) and len(trees["4"]) > 6
    for rel, b in trees["0"].items():
        assert trees["4"][rel] == b, rel
