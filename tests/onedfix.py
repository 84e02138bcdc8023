"""TEST INFRASTRUCTURE for the 1-D tests (test_config_1d.py, test_gpu_1d.py): reads tests/golden/g1d_*.npz (written by
tests/golden/make_golden_1d.py from the reference's own executables run on decks with Nx2 = Nx3 = 1) and restates bvals_mhd of a
1-D Grid on the host."""
import glob
import importlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
DECKS = os.path.join(ROOT, "atmospheric-athena_amd", "decks")
NG = 4
B, R = 248, 1272      # active zones per block of k1d_step, zones the resident kernel keeps (csrc/hydro1d_kernels.hip)

STEP_FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "g1d_blast_*.npz")) +
                       glob.glob(os.path.join(GOLDEN, "g1d_shk_*.npz")))
GENERATOR = {"blast1d": "blast", "sod1d": "shkset1d"}      # the fixture's `problem` -> problem generator
DECK = {"blast1d": "athinput.blast1d", "sod1d": "athinput.sod1d"}      # ... -> our 1-D deck (config.load: a 1-D run takes a 1-D deck)


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


def run_config(fx, extra=(), integrator=None):
    cfg = pkg("config")
    deck = str(fx["problem"])
    run = cfg.load(os.path.join(DECKS, DECK[deck]), [str(o) for o in fx["overrides"]] + list(extra), GENERATOR[deck],
                   integrator or str(fx["integrator"]))
    run.order = int(fx["order"])
    return run


def grid_config(fx, extra=(), integrator=None):
    return pkg("config").slab(run_config(fx, extra, integrator))


def host_block(gc, U_active, fill=0.0):
    """[1][1][N1][5] with the active zones of a fixture"""
    blk = np.full((1, 1, gc.Nx[0] + 2 * NG, 5), fill)
    blk[0, 0, NG:-NG, :] = U_active[0, 0]
    return blk


def bvals_1d(blk, bc):
    """bvals_mhd.c on a 1-D Grid: the x1 sides only; flags 1 reflect (M1 changes sign), 2 outflow, 4 periodic, 0 leaves the side
    alone.  Returns a new block."""
    U = blk.copy()
    N1 = U.shape[2]
    s, e = NG, N1 - NG - 1
    for lo in (True, False):
        flag = bc[0 if lo else 1]
        if not flag:
            continue
        for gl in range(1, NG + 1):
            dst = s - gl if lo else e + gl
            if flag == 1:
                src = s + (gl - 1) if lo else e - (gl - 1)
            elif flag == 2:
                src = s if lo else e
            else:
                src = e - (gl - 1) if lo else s + (gl - 1)
            U[0, 0, dst, :] = U[0, 0, src, :]
            if flag == 1:
                U[0, 0, dst, 1] = -U[0, 0, dst, 1]
    return U
