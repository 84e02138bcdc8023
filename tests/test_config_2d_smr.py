"""config.levels_2d: the Domains of a 2-D refined deck (root Nx3 = 1), nested by the rules of init_mesh.c:320-499 in x1 and x2, and
the deck decks/athinput.blast2d_smr that carries the reference's three-level 2-D blast.  config.levels keeps refusing such a deck
(tests/test_config_2d.py); this is the entry point beside it."""
import os

import pytest

from twodfix import DECKS, pkg

DECK = os.path.join(DECKS, "athinput.blast2d_smr")


def levels_2d(overrides=(), integrator="ctu"):
    aa, cfg = pkg(), pkg("config")
    ov = list(overrides)
    par = aa.athinput.ParTable.from_file(DECK).cmdline(ov)
    return cfg.levels_2d(par, cfg.load(DECK, ov, "blast", integrator))


def test_the_shipped_deck_gives_the_reference_s_three_domains():
    levs = levels_2d()
    assert [g.level for g in levs] == [0, 1, 2]
    assert [g.Nx for g in levs] == [(200, 300, 1), (240, 240, 1), (320, 320, 1)]
    assert [g.disp for g in levs] == [(0, 0, 0), (80, 180, 0), (240, 440, 0)]
    # init_mesh.c:375-390: root_xmin + Disp*dx of the level; x3 is the root's
    dx1, dx2 = 1.0 / 200, 1.5 / 300
    assert levs[0].MinX == (-0.5, -0.75, -0.5)
    assert levs[1].MinX == (-0.5 + 80.0 * (dx1 / 2.0), -0.75 + 180.0 * (dx2 / 2.0), -0.5)
    assert levs[2].MinX == (-0.5 + 240.0 * (dx1 / 4.0), -0.75 + 440.0 * (dx2 / 4.0), -0.5)
    assert levs[0].bc == (4, 4, 4, 4, 0, 0)
    assert levs[1].bc[:4] == (0, 0, 0, 0) and levs[2].bc[:4] == (0, 0, 0, 0)      # inner sides: ghost zones come by prolongation


def test_a_child_on_the_root_boundary_keeps_the_root_s_flag_there():
    ov = ["job/num_domains=2", "domain1/Nx1=32", "domain1/Nx2=24", "domain2/Nx1=24", "domain2/Nx2=16", "domain2/iDisp=0", "domain2/jDisp=12",
          "domain1/bc_ix1=2", "domain1/bc_ox1=2"]
    root, child = levels_2d(ov)
    assert child.bc[:4] == (2, 0, 0, 0) and child.MinX[0] == root.MinX[0] and child.disp == (0, 12, 0)
    # two Domains on one level, deck order
    ov = ["domain1/Nx1=40", "domain1/Nx2=24", "domain2/Nx1=16", "domain2/Nx2=16", "domain2/iDisp=12", "domain2/jDisp=16",
          "domain3/level=1", "domain3/Nx1=20", "domain3/Nx2=16", "domain3/iDisp=44", "domain3/jDisp=16"]
    assert [(g.level, g.Nx[:2], g.disp[:2]) for g in levels_2d(ov)] == [(0, (40, 24), (0, 0)), (1, (16, 16), (12, 16)), (1, (20, 16), (44, 16))]


SMALL = ["job/num_domains=2", "domain1/Nx1=32", "domain1/Nx2=24", "domain2/Nx1=24", "domain2/Nx2=16", "domain2/iDisp=16", "domain2/jDisp=12"]


@pytest.mark.parametrize("extra,match", [
    ([], "touches its parent in x1"),                                    # (its own deck below: level 2 on the edge of level 1)
    (["domain2/jDisp=2"], "closer than nghost/2 to its parent in x2"),
    (["domain2/iDisp=2"], "closer than nghost/2 to its parent in x1"),
    (["domain2/Nx1=23"], "Nx1 = 23 must be divisible by 2"),
    (["domain2/jDisp=13"], "Disp2 = 13 must be divisible by 2"),
    (["domain2/kDisp=2"], "kDisp"),
    (["domain2/Nx3=2"], "in domain2 grid is 3D, but in root level it is 2D"),
])
def test_what_init_mesh_refuses(extra, match):
    athinput = pkg("athinput")
    if match.startswith("touches"):
        # a child may touch its parent's edge only where that is the root boundary: level 2 on the edge of level 1
        ov = ["domain1/Nx1=32", "domain1/Nx2=24", "domain2/Nx1=24", "domain2/Nx2=16", "domain2/iDisp=16", "domain2/jDisp=12",
              "domain3/Nx1=16", "domain3/Nx2=16", "domain3/iDisp=32", "domain3/jDisp=32"]
    else:
        ov = SMALL + extra
    with pytest.raises(athinput.ParError, match=match):
        levels_2d(ov)


def test_siblings_may_neither_overlap_nor_touch():
    athinput = pkg("athinput")
    base = ["domain1/Nx1=40", "domain1/Nx2=24", "domain2/Nx1=16", "domain2/Nx2=16", "domain2/iDisp=12", "domain2/jDisp=16",
            "domain3/level=1", "domain3/Nx1=20", "domain3/Nx2=16", "domain3/jDisp=16"]
    for idisp in (28, 20):          # touching at i = 28, overlapping
        with pytest.raises(athinput.ParError, match="overlap or touch"):
            levels_2d(base + [f"domain3/iDisp={idisp}"])
    assert len(levels_2d(base + ["domain3/iDisp=30"])) == 3


def test_what_stays_refused():
    """config.levels and a 3-D run through levels_2d; CTU without H-correction on a refined 2-D deck (no reference build)"""
    aa, cfg, athinput = pkg(), pkg("config"), pkg("athinput")
    par = aa.athinput.ParTable.from_file(DECK)
    run = cfg.load(DECK, [], "blast")
    with pytest.raises(athinput.ParError, match="mesh refinement"):
        cfg.levels(par, run)
    with pytest.raises(athinput.ParError, match="H-correction"):
        levels_2d(integrator="ctu-noh")
    with pytest.raises(athinput.ParError, match="0.5 with 2D VL"):
        levels_2d(integrator="vl")                                    # the deck's cour_no is 0.8
    assert len(levels_2d(["time/cour_no=0.4"], "vl")) == 3
    deck3 = os.path.join(DECKS, "athinput.blast")
    with pytest.raises(athinput.ParError, match="levels_2d takes a 2-D run"):
        cfg.levels_2d(aa.athinput.ParTable.from_file(deck3), cfg.load(deck3, [], "blast"))


def test_the_shipped_deck_carries_the_reference_s_keys():
    """the values of the reference's tst/2D-hydro/athinput.blast, restated here (the test reads only our deck)"""
    par = pkg("athinput").ParTable.from_file(DECK)
    want = {"job": {"problem_id": "Blast", "num_domains": "3"},
            "time": {"cour_no": "0.8", "nlim": "10000", "tlim": "1.0"},
            "domain1": {"level": "0", "Nx1": "200", "x1min": "-0.5", "x1max": "0.5", "bc_ix1": "4", "bc_ox1": "4", "Nx2": "300",
                        "x2min": "-0.75", "x2max": "0.75", "bc_ix2": "4", "bc_ox2": "4", "Nx3": "1", "x3min": "-0.5", "x3max": "0.5"},
            "domain2": {"level": "1", "Nx1": "240", "Nx2": "240", "Nx3": "1", "iDisp": "80", "jDisp": "180", "kDisp": "0"},
            "domain3": {"level": "2", "Nx1": "320", "Nx2": "320", "Nx3": "1", "iDisp": "240", "jDisp": "440", "kDisp": "0"},
            "problem": {"gamma": "1.6666666667", "pamb": "0.1", "prat": "100.0", "radius": "0.1"}}
    for blk, kv in want.items():
        for k, v in kv.items():
            assert par.gets(blk, k) == v, (blk, k)
