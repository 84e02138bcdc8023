"""TEST INFRASTRUCTURE for the 2-D tests (test_config_2d.py, test_gpu_2d.py): reads tests/golden/g2d_*.npz (written by
tests/golden/make_golden_2d.py from the reference's own executables run on decks with Nx3 = 1) and restates bvals_mhd of a 2-D
Grid on the host."""
import glob
import importlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
DECKS = os.path.join(ROOT, "atmospheric-athena_amd", "decks")
NG = 4

STEP_FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "g2d_blast_*.npz")) +
                       glob.glob(os.path.join(GOLDEN, "g2d_shk_*.npz")))
GENERATOR = {"blast2d": "blast", "shkset1d": "shkset1d"}      # the fixture's `problem` -> problem generator
DECK = {"blast2d": "athinput.blast2d", "shkset1d": "athinput.shkset2d"}      # ... -> our 2-D deck (config.load: a 2-D run takes a 2-D deck)


def pkg(name=""):
    return importlib.import_module("atmospheric-athena_amd" + ("." + name if name else ""))


_cache = {}


def fixture(name):
    """the npz as a dict, read once and shared (nobody writes into it)"""
    if name not in _cache:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        d = {k: z[k] for k in z.files}
        for a in d.values():
            a.setflags(write=False)
        _cache[name] = d
    return _cache[name]


def grid_config(fx, extra=()):
    cfg = pkg("config")
    deck = str(fx["problem"])
    run = cfg.load(os.path.join(DECKS, DECK[deck]), [str(o) for o in fx["overrides"]] + list(extra), GENERATOR[deck],
                   str(fx["integrator"]))
    return cfg.slab(run)


def host_block(gc, U_active, fill=0.0):
    """[1][N2][N1][5] with the active zones of a fixture"""
    blk = np.full((1, gc.Nx[1] + 2 * NG, gc.Nx[0] + 2 * NG, 5), fill)
    blk[0, NG:-NG, NG:-NG, :] = U_active[0]
    return blk


def bvals_2d(blk, bc):
    """bvals_mhd.c on a 2-D Grid: the x1 sides over the active rows, then the x2 sides over every column (so the corners fill),
    no x3 pass; flags 1 reflect (the normal momentum changes sign), 2 outflow, 4 periodic.  Returns a new block."""
    U = blk.copy()
    N2, N1 = U.shape[1], U.shape[2]
    is_, ie, js, je = NG, N1 - NG - 1, NG, N2 - NG - 1

    def side(axis, lo, flag):
        s, e = (is_, ie) if axis == 0 else (js, je)
        rows = slice(js, je + 1) if axis == 0 else slice(None)
        for gl in range(1, NG + 1):
            dst = s - gl if lo else e + gl
            if flag == 1:
                src = s + (gl - 1) if lo else e - (gl - 1)
            elif flag == 2:
                src = s if lo else e
            else:
                src = e - (gl - 1) if lo else s + (gl - 1)
            if axis == 0:
                U[0, rows, dst, :] = U[0, rows, src, :]
                if flag == 1:
                    U[0, rows, dst, 1] = -U[0, rows, dst, 1]
            else:
                U[0, dst, :, :] = U[0, src, :, :]
                if flag == 1:
                    U[0, dst, :, 2] = -U[0, dst, :, 2]
    for axis in (0, 1):
        for lo in (True, False):
            f = bc[2 * axis + (0 if lo else 1)]
            if f:
                side(axis, lo, f)
    return U
