"""1-D runs (Nx2 = Nx3 = 1) on the host: what config accepts and refuses (check_1d, with the reference's messages), the two 1-D
decks, the rule that overrides may not change a deck's dimension, and the coverage of the g1d_* fixtures.  No GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import onedfix                      # noqa: E402
from onedfix import pkg, fixture    # noqa: E402

SOD = os.path.join(onedfix.DECKS, "athinput.sod1d")
BLAST = os.path.join(onedfix.DECKS, "athinput.blast1d")


def ParError():
    return pkg("athinput").ParError


def test_both_decks_load_as_1d_runs():
    cfg = pkg("config")
    run = cfg.load(SOD, None, "shkset1d")
    # tst/1D-hydro/athinput.sod: 128 zones on [-0.5, 0.5], outflow, cour_no 0.8 (legal with the 1-D CTU integrator), tlim 0.25
    assert run.rootNx == (128, 1, 1) and run.ndim == 1 and run.bc[:2] == (2, 2)
    assert run.cour_no == 0.8 and run.tlim == 0.25 and run.gamma == 1.4 and run.nlim == 1000
    assert (run.xmin[0], run.xmax[0]) == (-0.5, 0.5) and run.prob["dr"] == 0.125 and run.prob["pr"] == 0.1
    gc = cfg.slab(run)
    assert gc.Nx == (128, 1, 1) and gc.bc[:2] == (2, 2) and gc.MinX[0] == -0.5 and gc.level == 0
    # a direction with one zone keeps the root's extent (init_mesh.c:331-337)
    assert run.dx == (1.0 / 128, 1.0, 1.0)
    run = cfg.load(BLAST, ["time/cour_no=0.4"], "blast", "vl")
    assert run.rootNx == (200, 1, 1) and run.ndim == 1 and run.bc[:2] == (4, 4) and run.integrator == "vl"
    for integ in ("ctu", "ctu-noh"):
        assert cfg.load(BLAST, None, "blast", integ).cour_no == 0.8


def test_check_1d_accepts_and_refuses_with_the_references_messages():
    cfg = pkg("config")
    # integrate.c:41-44: the van Leer limit; :38-39: none with CTU
    with pytest.raises(ParError(), match=r"must be <= 0.5 with 1D VL integrator"):
        cfg.load(SOD, None, "shkset1d", "vl")
    assert cfg.load(SOD, ["time/cour_no=0.5"], "shkset1d", "vl").cour_no == 0.5
    assert cfg.load(SOD, ["time/cour_no=0.95"], "shkset1d", "ctu").cour_no == 0.95
    run = cfg.load(SOD, None, "shkset1d")
    cfg.check_1d(run)
    for order in (2, 3):                      # blast_ppm / blast_vl_ppm pin the third order in 1-D
        run.order = order
        cfg.check_1d(run)
    with pytest.raises(ParError(), match="1-D"):
        cfg.check_1d(run, nranks=2)
    with pytest.raises(ParError(), match="1-D"):
        cfg.slab(run, 0, 2)
    with pytest.raises(ParError(), match="1-D"):
        cfg.check_1d(run, nslab=2)
    with pytest.raises(ParError(), match="1-D"):
        cfg.check_1d(run, mesh=True)
    with pytest.raises(ParError(), match="fofc.*1-D"):
        cfg.load(SOD, ["time/cour_no=0.4"], "shkset1d", "vl", fofc=True)
    with pytest.raises(ParError(), match=r"shk_dir = 2 on a 1-D Grid"):
        cfg.load(SOD, ["problem/shk_dir=2"], "shkset1d")
    for problem in ("ifront", "ioniz_sphere"):
        with pytest.raises(ParError(), match="1-D"):
            cfg.load(SOD, None, problem)
    with pytest.raises(ParError(), match=r"bc flag = 3 unknown"):
        cfg.load(SOD, ["domain1/bc_ox1=3"], "shkset1d")
    # the flags of the directions with one zone are never looked at (bvals_mhd.c:187-193 installs no function there)
    assert cfg.load(SOD, ["domain1/bc_ix2=7", "domain1/bc_ox3=9"], "shkset1d").bc[:2] == (2, 2)
    # the refined levels of the reference's 1-D decks stay out
    par = pkg("athinput").ParTable.from_file(SOD).cmdline(["job/num_domains=2"])
    with pytest.raises(ParError(), match="1-D"):
        cfg.levels(par, run)
    # a 3-D or 2-D run is none of check_1d's business
    cfg.check_1d(cfg.load(os.path.join(onedfix.DECKS, "athinput.blast"), None, "blast"), nranks=4, mesh=True)


def test_a_deck_keeps_its_dimension():
    cfg = pkg("config")
    with pytest.raises(ParError(), match="1-D deck into a 2-D run"):
        cfg.load(SOD, ["domain1/Nx2=8"], "shkset1d")
    with pytest.raises(ParError(), match="1-D deck into a 3-D run"):
        cfg.load(SOD, ["domain1/Nx2=8", "domain1/Nx3=8", "time/cour_no=0.4"], "shkset1d")
    with pytest.raises(ParError(), match="2-D deck into a 1-D run"):
        cfg.load(os.path.join(onedfix.DECKS, "athinput.blast2d"), ["domain1/Nx2=1"], "blast")
    with pytest.raises(ParError(), match="3-D deck into a 1-D run"):
        cfg.load(os.path.join(onedfix.DECKS, "athinput.blast"), ["domain1/Nx2=1", "domain1/Nx3=1"], "blast")
    with pytest.raises(ParError(), match="3-D deck into a 2-D run"):
        cfg.load(os.path.join(onedfix.DECKS, "athinput.blast"), ["domain1/Nx3=1"], "blast")
    # the shapes no integrator takes keep the reference's messages (integrate.c:81-84)
    with pytest.raises(ParError(), match=r"1D problem must have Nx1 > 1"):
        cfg.load(SOD, ["domain1/Nx1=1", "domain1/Nx2=8"], "shkset1d")
    with pytest.raises(ParError(), match=r"\[config\]: a Domain of a single zone \(Nx1=1, Nx2=1, Nx3=1\)"):      # (the reference has no text for it)
        cfg.load(SOD, ["domain1/Nx1=1"], "shkset1d")
    # resizing along x1 is what overrides are for
    assert cfg.load(SOD, ["domain1/Nx1=1200"], "shkset1d").rootNx == (1200, 1, 1)


def test_drivers_that_need_more_than_one_grid_refuse_a_1d_run():
    cfg = pkg("config"); D = pkg("driver"); O = pkg("outputs"); A = pkg("athinput")
    run = cfg.load(SOD, None, "shkset1d")
    with pytest.raises(ParError(), match="1-D"):
        D.Driver(run, engine_factory=lambda g: None, rank=0, nranks=2)
    with pytest.raises(ParError(), match="1-D"):
        D.MeshRun([cfg.slab(run)], run)
    par = A.ParTable.from_file(SOD)
    with pytest.raises(ParError(), match="1-D"):
        D.MeshDriver(par, run)
    with pytest.raises(ValueError, match="1-D"):
        O.OutputSet.from_par(par, 0.0, ".", rst_ngrid=(2, 1, 1))


def test_every_size_class_and_integrator_has_a_fixture():
    names = onedfix.STEP_FIXTURES
    B, R = onedfix.B, onedfix.R
    sizes = {int(fixture(n)["nx"][0]) for n in names}
    assert {4, 5, B - 1, B, B + 1, 3 * B + 2, R, R + 1} <= sizes, sorted(sizes)
    have = {(str(fixture(n)["integrator"]), int(fixture(n)["order"])) for n in names}
    assert {("ctu-noh", 2), ("ctu", 2), ("ctu", 3), ("vl", 2), ("vl", 3)} <= have, have
    shk = [fixture(n) for n in names if n.startswith("g1d_shk_")]
    assert {tuple(f["bc"][:2]) for f in shk} == {(1, 1), (2, 2), (4, 4)}
    assert {0.4, 0.8} <= {pkg("config").load(os.path.join(onedfix.DECKS, "athinput.sod1d"), [str(o) for o in f["overrides"]], "shkset1d").cour_no
                          for f in shk}
    assert all(4 <= int(f["nstep"]) <= 12 for f in shk)
    assert any("einfeldt1125" in n for n in names)
    # the same run under both CTU names, the same bits: integrate_1d_ctu.c has no H-correction
    a, b = fixture("g1d_shk_ctu_bc2_c8_248_s12"), fixture("g1d_shk_ctu-noh_bc2_c8_248_s12")
    assert (a["U"] == b["U"]).all() and float(a["dt"]) == float(b["dt"]) and float(a["time"]) == float(b["time"])
    # the full run: 87 steps to tlim, the last dt clipped there
    full = fixture("g1d_sod_full")
    assert int(full["nstep"]) == 87 == len(full["times"]) == len(full["dts"]) and float(full["times"][-1]) == 0.25 == float(full["time"])
    assert float(full["times"][-2]) + float(full["dts"][-2]) == 0.25 and float(full["dts"][-2]) < float(full["dts"][-3])
    out = fixture("g1d_out_sod_24")
    exts = {str(p).rsplit(".", 1)[1] for p in out["paths"]}
    assert exts == {"hst", "vtk", "bin", "rst"}
    total = sum(os.path.getsize(p) for p in __import__("glob").glob(os.path.join(onedfix.GOLDEN, "g1d_*.npz")))
    assert total < 512 * 1024, total


def test_fewer_zones_than_ghost_zones_are_refused():
    """bvals_mhd.c fills a side's ghost zones one after the other and one side after the other; with Nx1 < nghost a boundary
    function reads ghost zones, the order decides what it finds, and the kernels fill all eight at once"""
    cfg = pkg("config")
    for n in (2, 3):
        with pytest.raises(ParError(), match=f"1-D Grid .* of {n} zones: fewer than the 4 ghost zones"):
            cfg.load(SOD, [f"domain1/Nx1={n}"], "shkset1d")
    assert cfg.load(SOD, ["domain1/Nx1=4"], "shkset1d").rootNx == (4, 1, 1)


class _Stalled:
    """a target of outputs.run whose advance() takes no step: what Driver.advance gives when dt is not positive (aa_run_1d ends
    at once) -- the single step then goes on as the reference does, and time = NaN ends the loop"""
    restarted = False

    def __init__(self, batch):
        self.time, self.nstep, self.batch, self.calls = 0.0, 0, batch, []

    def start(self): pass
    def may_batch(self): return self.batch

    def advance(self, t_stop, nstep_stop):
        self.calls.append(("advance", t_stop, nstep_stop))
        return 0

    def step(self):
        self.calls.append("step")
        self.nstep += 1
        self.time = float("nan")


@pytest.mark.parametrize("batch", [True, False])
def test_outputs_run_does_not_spin_when_advance_takes_no_step(batch, tmp_path):
    O = pkg("outputs"); A = pkg("athinput")
    par = A.ParTable.from_file(SOD).cmdline(["job/maxout=0"])
    t = _Stalled(batch)
    O.run(t, O.OutputSet.from_par(par, 0.0, str(tmp_path)), 0.25)
    assert t.calls == ([("advance", 0.25, None)] if batch else []) + ["step"]
