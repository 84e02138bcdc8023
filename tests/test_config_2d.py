"""2-D runs (Nx3 = 1) on the host side: what config / Driver accept and refuse, the geometry of the one Grid, the host
restatement of bvals_mhd the GPU test compares against, and the host writers (rst, vtk, bin, hst) against the files the reference
left for a 2-D run (tests/golden/g2d_out_blast_24x20.npz).  No GPU."""
import json
import os
import re
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dumpfix                      # noqa: E402
import twodfix                      # noqa: E402
from twodfix import pkg, fixture    # noqa: E402

DECK = os.path.join(twodfix.DECKS, "athinput.blast2d")
NG = twodfix.NG


def ParError():
    return pkg("athinput").ParError


# ---- what is accepted --------------------------------------------------------------------------------------------------------
def test_the_2d_deck_loads_and_gives_one_grid_without_x3_ghost_zones():
    cfg = pkg("config")
    run = cfg.load(DECK, None, "blast")
    assert run.rootNx == (200, 300, 1) and run.rootNx[2] == 1 and run.ndim == 2
    assert run.cour_no == 0.8 and run.nscal == 0 and not run.ion             # tst/2D-hydro/athinput.blast runs at 0.8
    assert run.dx == (1.0 / 200, 1.5 / 300, 1.0)
    g = cfg.slab(run)
    assert g.Nx == (200, 300, 1) and g.MinX == (-0.5, -0.75, -0.5) and g.disp == (0, 0, 0)
    assert g.bc[:4] == (4, 4, 4, 4) and g.lx3 == -1 and g.rx3 == -1 and g.nranks == 1 and g.level == 0
    run = cfg.load(DECK, ["domain1/Nx1=67", "domain1/Nx2=35", "domain1/bc_ix1=1", "domain1/bc_ox1=2", "domain1/x2min=-0.3"], "blast")
    g = cfg.slab(run)
    assert g.Nx == (67, 35, 1) and g.bc[:4] == (1, 2, 4, 4) and g.MinX[1] == -0.3
    p = pkg("lib").params_from_grid(g)
    assert tuple(p.Nx) == (67, 35, 1) and tuple(p.rootNx) == (67, 35, 1) and p.integrator == 0


def test_cour_no_above_one_half_is_the_2d_ctu_integrators_alone():
    cfg = pkg("config")
    for integ in ("ctu", "ctu-noh"):
        assert cfg.load(DECK, ["time/cour_no=0.8"], "blast", integ).cour_no == 0.8
    with pytest.raises(ParError(), match=r"must be <= 0\.5 with 2D VL integrator"):                    # integrate.c:55-57
        cfg.load(DECK, ["time/cour_no=0.8"], "blast", "vl")
    assert cfg.load(DECK, ["time/cour_no=0.5"], "blast", "vl").integrator == "vl"
    with pytest.raises(ParError(), match="3D integrator"):                                             # 3-D: either integrator
        cfg.load(os.path.join(twodfix.DECKS, "athinput.blast"), ["time/cour_no=0.8"], "blast", "vl")


# ---- what is refused ------------------------------------------------------------------------------------------------------------
def test_overrides_do_not_change_the_dimension_of_a_deck():
    """a 2-D run takes a deck written with Nx3 = 1 (the x3 keys, cour_no and the output blocks of a 3-D deck are not a 2-D run's)"""
    cfg = pkg("config")
    with pytest.raises(ParError(), match="3-D deck into a 2-D run"):
        cfg.load(os.path.join(twodfix.DECKS, "athinput.blast"), ["domain1/Nx3=1"], "blast")
    with pytest.raises(ParError(), match="2-D deck into a 3-D run"):
        cfg.load(DECK, ["domain1/Nx3=8", "time/cour_no=0.4"], "blast")
    run = cfg.load(os.path.join(twodfix.DECKS, "athinput.shkset2d"), ["domain1/Nx1=48", "problem/shk_dir=2"], "shkset1d")
    assert run.rootNx == (48, 8, 1) and run.ndim == 2 and run.bc[:4] == (2, 2, 2, 2)


def test_other_degenerate_shapes_are_refused_with_the_references_messages():
    cfg = pkg("config")
    with pytest.raises(ParError(), match=r"2D problem must have Nx1 and Nx2 > 1: Nx1=200, Nx2=1, Nx3=8"):   # integrate.c:83-84
        cfg.load(DECK, ["domain1/Nx2=1", "domain1/Nx3=8"], "blast")
    with pytest.raises(ParError(), match=r"1D problem must have Nx1 > 1"):                                  # :81-82
        cfg.load(DECK, ["domain1/Nx1=1"], "blast")
    with pytest.raises(ParError(), match="1-D"):
        cfg.load(DECK, ["domain1/Nx2=1"], "blast")


def test_what_no_reference_target_pins_in_2d_is_refused_on_the_host():
    cfg = pkg("config"); drv = pkg("driver")
    E = ParError()
    for deck, prob in (("athinput.ifront", "ifront"), ("athinput.ioniz_sphere", "ioniz_sphere")):      # ion radiation, scalars, gravity
        par = pkg("athinput").ParTable.from_file(os.path.join(twodfix.DECKS, deck)).cmdline(["domain1/Nx3=1"])
        with pytest.raises(E, match="ion radiation"):
            cfg.from_par(par, prob)
    with pytest.raises(E, match="fofc"):
        cfg.load(DECK, ["time/cour_no=0.4"], "blast", "vl", fofc=True)
    run = cfg.load(DECK, None, "blast")
    run.order = 3
    with pytest.raises(E, match="third-order"):
        cfg.slab(run)
    run.order = 2
    with pytest.raises(E, match="2 ranks"):                        # no x3 to cut
        cfg.slab(run, 0, 2)
    with pytest.raises(E, match="ranks"):                          # x2 cuts are a follow-up
        cfg.pencil(run, 0, 2, 1)
    with pytest.raises(E, match="slabs"):
        cfg.check_2d(run, nslab=2)
    with pytest.raises(E, match="2 ranks"):
        drv.Driver(run, engine_factory=lambda g: None, rank=0, nranks=2)
    # a refined mesh: the reference's own 2-D deck has three levels, ours stops at the root
    par = pkg("athinput").ParTable.from_file(os.path.join(twodfix.DECKS, "athinput.blast")).cmdline(
        ["domain1/Nx3=1", "job/num_domains=2", "domain2/Nx3=1", "domain2/kDisp=0"])
    run2 = cfg.from_par(par, "blast")
    with pytest.raises(E, match="mesh refinement"):
        cfg.levels(par, run2)
    with pytest.raises(E, match="mesh refinement"):
        drv.MeshDriver(par, run2)


# ---- the host restatement of bvals_mhd on a 2-D Grid ---------------------------------------------------------------------------
def test_bvals_restatement():
    rng = np.random.default_rng(3)
    blk = rng.uniform(-1, 1, size=(1, 6 + 2 * NG, 5 + 2 * NG, 5))
    act = blk[0, NG:-NG, NG:-NG]
    per = twodfix.bvals_2d(blk, (4, 4, 4, 4, 0, 0))
    assert np.array_equal(per[0], np.pad(act, ((NG, NG), (NG, NG), (0, 0)), mode="wrap"))
    out = twodfix.bvals_2d(blk, (2, 2, 2, 2, 0, 0))
    assert np.array_equal(out[0], np.pad(act, ((NG, NG), (NG, NG), (0, 0)), mode="edge"))
    ref = twodfix.bvals_2d(blk, (1, 1, 1, 1, 0, 0))
    want = np.pad(act, ((NG, NG), (NG, NG), (0, 0)), mode="symmetric")
    want[:, :NG, 1] *= -1; want[:, -NG:, 1] *= -1; want[:NG, :, 2] *= -1; want[-NG:, :, 2] *= -1
    assert np.array_equal(ref[0], want)
    # mixed: the corner takes the x2 copy of what the x1 pass left (x1 first, then x2 over every column)
    mix = twodfix.bvals_2d(blk, (1, 2, 4, 4, 0, 0))
    assert np.array_equal(mix[0, :NG, :NG], mix[0, -2 * NG:-NG, :NG]) and mix[0, 0, 0, 1] == -act[-NG, NG - 1, 1]
    assert np.array_equal(mix[0, NG:-NG, NG:-NG], act)
    none = twodfix.bvals_2d(blk, (0, 0, 4, 4, 0, 0))
    assert np.array_equal(none[0, NG:-NG, :NG], blk[0, NG:-NG, :NG])


# ---- the host writers against the reference's 2-D files -------------------------------------------------------------------------
def _out_fixture():
    fx = fixture("g2d_out_blast_24x20")
    paths = [str(p) for p in fx["paths"]]
    files = {p: fx[f"file_{i}"].tobytes() for i, p in enumerate(paths)}
    run = pkg("config").load(DECK, [str(o) for o in fx["overrides"]], "blast")
    return fx, files, run


def _rst_state(b, nx):
    """(header text, nstep, time, dt, U active [1][Nx2][Nx1][5]) of the bytes of a restart dump"""
    end = b.index(b"<par_end>\n") + len(b"<par_end>\n")
    pos = end + len(b"N_STEP\n")
    nstep = struct.unpack_from("<i", b, pos)[0]; pos += 4 + len(b"\nTIME\n")
    time = struct.unpack_from("<d", b, pos)[0]; pos += 8 + len(b"\nTIME_STEP\n")
    dt = struct.unpack_from("<d", b, pos)[0]; pos += 8
    n = nx[0] * nx[1] * nx[2]
    U = np.zeros((nx[2], nx[1], nx[0], 5))
    for c, lab in enumerate(("DENSITY", "1-MOMENTUM", "2-MOMENTUM", "3-MOMENTUM", "ENERGY")):
        tag = b"\n" + lab.encode() + b"\n"
        assert b[pos:pos + len(tag)] == tag
        pos += len(tag)
        U[..., c] = np.frombuffer(b, dtype="<f8", count=n, offset=pos).reshape(nx[2], nx[1], nx[0]); pos += 8 * n
    assert b[pos:] == b"\nUSER_DATA\n"
    return b[:end].decode(), nstep, time, dt, U


def test_host_writers_reproduce_the_references_2d_files(tmp_path):
    fx, files, run = _out_fixture()
    g = pkg("config").slab(run)
    nx = g.Nx
    rsts = sorted(p for p in files if p.endswith(".rst"))
    assert len(rsts) == 3 and sum(p.endswith((".vtk", ".bin")) for p in files) == 8 and "Blast.hst" in files
    blocks = json.loads(str(fx["blocks"]))
    hist = pkg("history")
    hst_lines = files["Blast.hst"].decode().splitlines(keepends=True)
    assert "".join(hst_lines[:3]) == hist.header(0, 0, (run.xmax[0] - run.xmin[0]) * (run.xmax[1] - run.xmin[1]), 0)
    rows_seen = 0
    for rel in rsts:
        head, nstep, time, dt, U = _rst_state(files[rel], nx)
        # rst: the whole file, under the reference's own parameter dump
        p = str(tmp_path / "x.rst")
        pkg("restart").write_rst(p, head, nstep, time, dt, U)
        assert open(p, "rb").read() == files[rel], rel
        # the dumps written at the same instant: the numbers the blocks' tables in this rst file carry, minus one
        par = pkg("athinput").ParTable.from_text(head)
        for n, ext in (("2", "bin"), ("3", "vtk")):
            num = par.geti(f"output{n}", "num") - 1
            ref = files["Blast.%04d.%s" % (num, ext)]
            prim = blocks[n].get("out", "cons") == "prim"
            q = str(tmp_path / ("x." + ext))
            pkg("dumps").write_dump_from_block(q, ext, U, prim=prim, gamma=run.gamma, nscal=0, nx=nx, minx=g.MinX, dx=run.dx,
                                               time=time, dt=dt)
            assert dumpfix.compare_dump(open(q, "rb").read(), ref, nx, 0, ext, prim, f"{rel} -> {ext}") == 0
        # hst: the row of this instant, the zones added up one by one in the reference's order (dump_history.c:157-200), so that
        # even the columns that are rounding noise (the net momenta of a symmetric run) come out the same
        dVol = 1.0 * run.dx[0] * run.dx[1] * run.dx[2]
        s = [0.0] * 8
        for z in U.reshape(-1, 5):
            d, M1, M2, M3, E = (float(v) for v in z)
            d1 = 1.0 / d
            for m, v in enumerate((dVol * d, dVol * E, dVol * M1, dVol * M2, dVol * M3,
                                   dVol * 0.5 * (M1 * M1) * d1, dVol * 0.5 * (M2 * M2) * d1, dVol * 0.5 * (M3 * M3) * d1)):
                s[m] += v
        vol = (run.xmax[0] - run.xmin[0]) * (run.xmax[1] - run.xmin[1])                     # :316-321: Nx3 = 1 does not count
        row = hist.format_row([time, dt] + [v / vol for v in s])
        assert row in hst_lines[3:], (rel, row, hst_lines)
        rows_seen += 1
        # and the vectorised sums the drivers use agree with it to rounding
        assert np.allclose(hist.sums_from_block(U, run.dx, 0)[[0, 1, 5, 6, 7]], np.array(s)[[0, 1, 5, 6, 7]], rtol=1e-13, atol=0)
    assert rows_seen == 3 and len(hst_lines) == 3 + 4


def test_vtk_header_of_a_2d_grid_counts_one_corner_plane():
    h = pkg("dumps").vtk_header((24, 20, 1), (-0.5, -0.75, -0.5), (1 / 24, 0.075, 1.0), 0.0, 0, 0, True).decode()
    assert "DIMENSIONS 25 21 1\n" in h and "CELL_DATA 480 \n" in h                     # dump_vtk.c:147-149
    h3 = pkg("dumps").vtk_header((24, 20, 2), (0, 0, 0), (1, 1, 1), 0.0, 0, 0, True).decode()
    assert "DIMENSIONS 25 21 3\n" in h3
