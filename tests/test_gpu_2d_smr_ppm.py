"""Static mesh refinement on 2-D Grids at THIRD order on an MI355X: aa_mesh_create_2d on levels that are all at order 3
(aa_set_order_2d) with CTU + H-correction, aa_mesh_step and aa_mesh_run_2d on such a Mesh, against tests/golden/g2dppmsmr_*.npz --
runs of the reference's blast_smr_ppm build on its 2-D blast deck at cour_no 0.8 (tests/golden/make_golden_2d_ppm.py).

A level reconstructs in k2d_first only; restriction, flux correction and prolongation are what they are at second order.  The strict
build agrees BIT FOR BIT on every level with time and dt; the default build is held to the bars of test_gpu_2d_smr.py (1e-11 of each
field's maximum, 1e-12 in dt)."""
import dataclasses
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import twodfix                      # noqa: E402
from twodfix import DECKS, NG, pkg  # noqa: E402

pytestmark = pytest.mark.gpu

DECK = os.path.join(DECKS, "athinput.blast2d_smr")
# three nested levels; a child on the root boundary; a child three x1 tiles wide with its outline on tile-edge faces; two Domains on a level
CASES = [("A", 6), ("B", 5), ("T", 4), ("D", 6)]
TOL_U, TOL_DT = 1e-11, 1e-12
FAR = 1.0e300


def fixture(case, n):
    return twodfix.fixture(f"g2dppmsmr_{case}_ctu_s{n}")


def levels(fx, integ="ctu", order_2d=3, extra=()):
    aa, cfg = pkg(), pkg("config")
    ov = [str(o) for o in fx["overrides"]] + list(extra)
    par = aa.athinput.ParTable.from_file(DECK).cmdline(ov)
    return cfg.levels_2d(par, cfg.load(DECK, ov, "blast", integ, order_2d=order_2d))


def make_mesh(fx, strict):
    m = pkg("lib").Mesh(levels(fx), 0, strict)
    assert [g.order for g in m.lev] == [3] * len(m.lev)
    return m


def active(U):
    return U[:, NG:-NG, NG:-NG, :]


def relerr(a, b):
    out = []
    for c in range(a.shape[-1]):
        scale = np.abs(b[..., c]).max()
        diff = float(np.abs(a[..., c] - b[..., c]).max())
        out.append(diff / scale if scale > 0 else (0.0 if diff == 0.0 else np.inf))
    return out


_runs = {}


def stepped(case, n, strict):
    """start + n calls of Mesh.step(): the whole blocks of every level at step 0 and after the steps, time, dt, dt0; run once and shared"""
    key = (case, n, strict)
    if key not in _runs:
        m = make_mesh(fixture(case, n), strict)
        try:
            m.start()
            first = [g.download() for g in m.lev]
            dt0 = m.dt
            for _ in range(n):
                m.step()
            out = dict(first=first, last=[g.download() for g in m.lev], time=m.time, dt=m.dt, dt0=dt0, nstep=m.nstep)
        finally:
            m.close()
        for a in out["first"] + out["last"]:
            a.setflags(write=False)
        _runs[key] = out
    return _runs[key]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("case,n", CASES, ids=[f"{c}{n}" for c, n in CASES])
def test_levels_vs_the_third_order_reference(case, n, strict):
    fx = fixture(case, n)
    r = stepped(case, n, strict)
    assert r["nstep"] == int(fx["nstep"]) and len(r["last"]) == int(fx["nlevels"])
    for l in range(int(fx["nlevels"])):
        assert np.array_equal(active(r["first"][l]), fx[f"U0_{l}"]), f"step 0, level {l}"
    err = [relerr(active(U), fx[f"U_{l}"]) for l, U in enumerate(r["last"])]
    e_dt0, e_dt, e_t = abs(r["dt0"] / float(fx["dt0"]) - 1), abs(r["dt"] / float(fx["dt"]) - 1), abs(r["time"] / float(fx["time"]) - 1)
    print(f"{case}{n} {'strict' if strict else 'default'}: max error / field maximum per level {[max(e) for e in err]}, "
          f"dt0 {e_dt0:.2e} dt {e_dt:.2e} time {e_t:.2e}")
    if strict:
        assert r["dt0"] == float(fx["dt0"]) and r["time"] == float(fx["time"]) and r["dt"] == float(fx["dt"])
        for l, U in enumerate(r["last"]):
            assert np.array_equal(active(U), fx[f"U_{l}"]), f"level {l}: {err[l]}"
    else:
        assert e_dt0 < TOL_DT and e_dt < TOL_DT and e_t < TOL_DT
        for l in range(len(err)):
            assert max(err[l]) < TOL_U, f"level {l}: {err[l]}"


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("case,n", CASES, ids=[f"{c}{n}" for c, n in CASES])
def test_run_2d_gives_the_bits_of_step(case, n, strict, monkeypatch):
    """one batch of n + 2 queued steps: two stand behind the stop; whole blocks of every level, ghost zones included, and the clock"""
    monkeypatch.setenv("AA_2D_BATCH", str(n + 2))
    m = make_mesh(fixture(case, n), strict)
    try:
        assert m.can_run_2d() and m.run_2d_batch() == n + 2
        m.start()
        assert m.run_2d(FAR, nstep_stop=n) == n
        got = (m.time, m.dt, m.nstep), [g.download() for g in m.lev]
    finally:
        m.close()
    r = stepped(case, n, strict)
    assert got[0] == (r["time"], r["dt"], r["nstep"])
    for l, (U, V) in enumerate(zip(got[1], r["last"])):
        assert np.array_equal(U, V), f"level {l} against step(): {relerr(U, V)}"


def test_mixed_orders_and_van_leer_levels_at_order_3_are_refused():
    lib = pkg("lib")
    fx = fixture("B", 5)
    # the root at order 3, the child at 2 -- and the other way round
    for orders in ((3, 2), (2, 3)):
        grids = [dataclasses.replace(g, run=dataclasses.replace(g.run, order_2d=o)) for g, o in zip(levels(fx), orders)]
        with pytest.raises(lib.AthenaError, match=r"\[aa_mesh_create_2d\].*share one reconstruction order"):
            lib.Mesh(grids, 0, True)
    # van Leer levels at order 3: no blast_smr_vl_ppm build (config.levels_2d says so on the host; here the library is asked)
    vl = levels(fx, "vl", 2, extra=["time/cour_no=0.4"])
    grids = [dataclasses.replace(g, run=dataclasses.replace(g.run, order_2d=3)) for g in vl]
    with pytest.raises(lib.AthenaError, match=r"\[aa_mesh_create_2d\].*van Leer level at third order"):
        lib.Mesh(grids, 0, True)
    # ... while second-order van Leer levels and third-order CTU levels make a Mesh; a level of one no longer takes the setter
    lib.Mesh(vl, 0, True).close()
    m = lib.Mesh(levels(fx), 0, True)
    try:
        with pytest.raises(lib.AthenaError, match=r"\[aa_set_order_2d\].*belongs to a Mesh"):
            m.lev[0].set_order_2d(2)
        assert m.lev[0].order == 3
    finally:
        m.close()
