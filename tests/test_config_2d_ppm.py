"""Third-order reconstruction on 2-D runs (Nx3 = 1) on the host side: the opt-in switch ``order_2d`` of config.RunConfig -- where it
is accepted, where refused, that ``order = 3`` on a 2-D run is refused as before, and that the levels of a 2-D Mesh carry it.  No GPU."""
import inspect
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import twodfix                      # noqa: E402
from twodfix import pkg             # noqa: E402

DECK = os.path.join(twodfix.DECKS, "athinput.blast2d")
DECK_SMR = os.path.join(twodfix.DECKS, "athinput.blast2d_smr")


def ParError():
    return pkg("athinput").ParError


def test_order_2d_is_off_by_default_and_accepted_with_ctu_and_van_leer():
    cfg = pkg("config")
    assert cfg.load(DECK, None, "blast").order_2d == 2
    run = cfg.load(DECK, None, "blast", order_2d=3)
    assert run.order_2d == 3 and run.order == 2 and run.integrator == "ctu" and run.cour_no == 0.8      # (CTU keeps the deck's 0.8)
    assert cfg.slab(run).run.order_2d == 3
    run = cfg.load(DECK, ["time/cour_no=0.4"], "blast", "vl", order_2d=3)
    assert run.order_2d == 3 and run.integrator == "vl"
    assert cfg.load(DECK, None, "blast", order_2d=2).order_2d == 2
    # aa_params.order stays 2: the library's switch is the setter behind aa_create
    assert pkg("lib").params_from_grid(cfg.slab(cfg.load(DECK, None, "blast", order_2d=3))).order == 2


def test_order_2d_is_refused_where_no_third_order_build_pins_it():
    cfg = pkg("config"); E = ParError()
    with pytest.raises(E, match=r"order_2d = 3 with \"ctu-noh\""):                  # no blast_noh_ppm build
        cfg.load(DECK, None, "blast", "ctu-noh", order_2d=3)
    with pytest.raises(E, match="order_2d = 4"):
        cfg.load(DECK, None, "blast", order_2d=4)
    with pytest.raises(E, match="order_2d = 3 on a 3-D run"):                         # a 3-D run takes `order`
        cfg.load(os.path.join(twodfix.DECKS, "athinput.blast"), None, "blast", order_2d=3)
    with pytest.raises(E, match="order_2d = 3 on a 1-D run"):
        cfg.load(os.path.join(twodfix.DECKS, "athinput.blast1d"), None, "blast", order_2d=3)
    with pytest.raises(E, match="must be <= 0.5 with 2D VL integrator"):              # (the van Leer limit is what it was)
        cfg.load(DECK, None, "blast", "vl", order_2d=3)
    # what stays refused on 2-D stays refused at third order
    run = cfg.load(DECK, None, "blast", order_2d=3)
    with pytest.raises(E, match="2 ranks"):
        cfg.slab(run, 0, 2)
    with pytest.raises(E, match="slabs"):
        cfg.check_2d(run, nslab=2)
    with pytest.raises(E, match="fofc"):
        cfg.load(DECK, ["time/cour_no=0.4"], "blast", "vl", fofc=True, order_2d=3)


def test_order_3_on_a_2d_run_still_raises_as_before():
    cfg = pkg("config")
    for order_2d in (2, 3):
        run = cfg.load(DECK, None, "blast", order_2d=order_2d)
        run.order = 3
        with pytest.raises(ParError(), match=r"third-order reconstruction on a 2-D Grid \(Nx3 = 1\): no reference target pins it"):
            cfg.slab(run)


def test_levels_2d_carries_order_2d_to_every_level():
    cfg = pkg("config"); A = pkg("athinput")
    par = A.ParTable.from_file(DECK_SMR)
    run = cfg.load(DECK_SMR, None, "blast", order_2d=3)
    levs = cfg.levels_2d(par, run)
    assert len(levs) > 1 and all(g.run.order_2d == 3 for g in levs)
    assert all(g.run.order_2d == 2 for g in cfg.levels_2d(par, cfg.load(DECK_SMR, None, "blast")))
    # blast_smr_ppm is CTU + H-correction: refined van Leer levels at third order have no reference build
    run_vl = cfg.load(DECK_SMR, ["time/cour_no=0.4"], "blast", "vl", order_2d=3)
    with pytest.raises(ParError(), match="third order with the van Leer integrator"):
        cfg.levels_2d(par, run_vl)
    assert len(cfg.levels_2d(par, cfg.load(DECK_SMR, ["time/cour_no=0.4"], "blast", "vl"))) == len(levs)      # (second order: as before)


def test_the_restart_entries_take_the_keyword():
    """the reference's order is a build option and is not in a restart file: from_restart takes it as a keyword"""
    D = pkg("driver")
    for cls in (D.Driver, D.MeshRun):
        assert inspect.signature(cls.from_restart).parameters["order_2d"].default == 2
    assert inspect.signature(pkg("config").load).parameters["order_2d"].default == 2
    G = pkg("lib").Grid
    assert callable(G.set_order_2d) and isinstance(G.order, property)
