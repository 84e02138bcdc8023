"""Every branch of the ion step's per-zone chemistry on the GPU (csrc/ion_dev.h + ion_kernels.hip, csrc/ion_pass.hip, the
entry inside the first pass) against the oracle, on a state designed to reach them all (tests/ionmatrix.py, pinned to the
reference by tests/golden/ionmatrix_*.npz; tests/test_oracle_golden.py holds the census) and on the ifront deck with 20 rays,
whose step leaves the sub-cycle loop by dt_hydro < dt_done.  Both builds, both kernel sets.

Tolerances.  Quantities of one phase that no rate enters (floored energies, the first sweep) are held to the rtol = 1e-14 of
test_gpu_ion_pass.py.  What the rates enter (E and s after updates, later sweeps, the time-step limits, dt_hydro) is held to
twice the spread of the ORACLE's own 1-ulp twins over the same sub-cycles (twins.ion_matrix, computed in this session; ~1e-15),
with a floor of 1e-14.  A zone the temperature floor has just floored re-evaluates to T = tfloor (1 +- eps): whether it is
"cold" (no thermal update) is decided in the last bit, in the reference too; such edge zones (|T/tfloor - 1| < 1e-12 in the
oracle, at most the zones the pattern floors on entry) may take either branch."""
import importlib
import os

import numpy as np
import pytest

import ionmatrix
import orc
import twins

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL1 = 1e-14           # single-phase ion quantities (test_gpu_ion_pass.py)
PATHS = [1, 2]          # ion_path: 1 = the one-kernel sub-cycle (ion_pass.hip), 2 = tile sweep + separate update (ion_kernels.hip)


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("atmospheric-athena_amd.lib")


def _grid(aa, lib, strict, ion_path, tceil=None):
    """the designed state on the device, boundary zones set, the radiation plane in place"""
    run = aa.config.load(os.path.join(orc.DECKS, "athinput.ifront"), ionmatrix.overrides(ionmatrix.NX, tceil), "ifront")
    g = lib.Grid(aa.config.slab(run), 0, strict, ion_path=ion_path)
    assert g.ion_is_fused() == (ion_path == 1)
    U = g.new_host_block()
    U[4:-4, 4:-4, 4:-4] = ionmatrix.pattern(run)
    g.upload(U)
    g.add_radplane_3d(-1, run.prob["flux"])
    g.bvals_mhd(); g.bvals_ionrad()
    return g


class GpuFollower:
    """a device Grid behind the interface ionmatrix.follow() drives.  The two-kernel set takes its step as an argument.  The
    one-kernel set picks its step on the device (k_ion_pick2): it is handed the step as the limit the pick is cut back to --
    pick(first, limit = dt) starts from dt_done = 0, so the cut gives dt exactly -- and the updating pass then runs in its
    closing form; the sweep of the next sub-cycle is the next call's.  (The updating pass WITH the next sweep runs in the
    whole-step tests below.)"""

    def __init__(self, g): self.g = g; self.fused = g.ion_is_fused()
    def begin(self): self.g.ion_begin()

    def rates(self, dt):
        if not self.fused:
            return self.g.ion_rates()
        self.g.ion_pass(False, True); self.g.ion_pick(0, 1, True, dt)
        v = self.g.ion_fetch()
        return v[2], v[3]

    def update(self, dt):
        if not self.fused:
            return self.g.ion_update(dt)
        self.g.ion_pass(True, False); self.g.ion_pick(0, 1, False, 1e300)
        applied, hit, _, _, count, dt_hydro, neg = self.g.ion_fetch()
        assert applied == dt and hit and not neg, (applied, dt, hit, neg)        # the device's own minimum was above the step it was handed
        self.g.ion_finish()
        return count, dt_hydro

    def state(self): return self.g.download()[4:-4, 4:-4, 4:-4]
    def edgeflux(self): return self.g.download_edgeflux()

    def set_E(self, mask, E):
        U = self.g.download()
        U[4:-4, 4:-4, 4:-4, 4][mask] = E[mask]
        self.g.upload(U)


@pytest.fixture(scope="module")
def tol():
    """twice the spread of the oracle's 1-ulp twins, floor 1e-14, per quantity; (tolerances, spreads, twins' flipped edge zones)"""
    spread, nflip = twins.ion_matrix()
    return {k: max(2.0 * v, 1e-14) for k, v in spread.items()}, spread, nflip


@pytest.mark.parametrize("tceil", [None, 0])
@pytest.mark.parametrize("begin_fused", ["1", "0"])
@pytest.mark.parametrize("ion_path", PATHS)
@pytest.mark.parametrize("strict", [True, False])
def test_entry_floors(aa, lib, strict, ion_path, begin_fused, tceil, monkeypatch):
    """apply_temp_floor + apply_neutral_floor at the entry of the ion step (ionrad_3d.c:70-156), in all three places that do
    them: k_ion_begin, k_ion_begin16, and the first pass of the one-kernel sub-cycle (AA_ION_BEGIN_FUSED).  The zones whose E
    changed and the zones whose s changed are the oracle's; s is bitwise the oracle's (a copy of d, or d IONFRACFLOOR, or
    d_nlo); floored and ceiling-clamped E within 1e-14; untouched zones bit for bit.  tceil = 0: the ceiling is off."""
    monkeypatch.setenv("AA_ION_BEGIN_FUSED", begin_fused)
    tr = ionmatrix.trace(tceil)
    g = _grid(aa, lib, strict, ion_path, tceil)
    g.ion_begin()
    if ion_path == 1:
        g.ion_pass(False, True)              # (with AA_ION_BEGIN_FUSED the entry rides on this pass; without, it changes no state)
    A = g.download()[4:-4, 4:-4, 4:-4]
    U0, ref = tr["U0"], tr["entry"]
    assert np.array_equal(A[..., :4], U0[..., :4])
    chE, chs = ref[..., 4] != U0[..., 4], ref[..., 5] != U0[..., 5]
    assert np.array_equal(A[..., 4] != U0[..., 4], chE) and np.array_equal(A[..., 5] != U0[..., 5], chs)
    assert np.array_equal(A[..., 5], ref[..., 5])
    err = np.abs(A[..., 4] / ref[..., 4] - 1.0)
    hot = ionmatrix.indices()[0] == 8
    print(f"entry: {int(chE.sum())} zones' E and {int(chs.sum())} zones' s changed, {int((chE & hot).sum())} by the ceiling; "
          f"max rel err of E {err.max():.2e} (strict={strict}, ion_path={ion_path}, begin_fused={begin_fused}, tceil={tceil})")
    assert err.max() <= RTOL1
    assert (chE & hot).sum() == (0 if tceil == 0 else hot.sum()) and hot.sum() >= 32
    g.close()


@pytest.mark.parametrize("ion_path", PATHS)
@pytest.mark.parametrize("strict", [True, False])
def test_first_rates_pass(aa, lib, strict, ion_path, tol):
    """dt_chem and dt_therm of the first rates pass against the oracle's.  (That neither is set by an edge zone is asserted on
    the oracle's arrays where the trace is built.)"""
    tr = ionmatrix.trace()
    t = tr["sub"][0]
    assert all(t["census"][k] >= 32 for k in ionmatrix.CLASSES), t["census"]
    f = GpuFollower(_grid(aa, lib, strict, ion_path))
    f.begin()
    dt_chem, dt_therm = f.rates(t["dt"])
    e = (abs(dt_chem / t["dt_chem"] - 1.0), abs(dt_therm / t["dt_therm"] - 1.0))
    print(f"first rates pass: dt_chem {dt_chem:.17g} (rel err {e[0]:.2e}), dt_therm {dt_therm:.17g} (rel err {e[1]:.2e}); "
          f"twins {tol[1]['dt_chem']:.2e}, {tol[1]['dt_therm']:.2e} (strict={strict}, ion_path={ion_path})")
    assert e[0] <= tol[0]["dt_chem"] and e[1] <= tol[0]["dt_therm"]
    f.g.close()


@pytest.mark.parametrize("ion_path", PATHS)
@pytest.mark.parametrize("strict", [True, False])
def test_twelve_subcycles_phase_by_phase(aa, lib, strict, ion_path, tol):
    """Twelve sub-cycles with the oracle's steps fed to both sides; after each update E and s of every zone, EdgeFlux, the
    two time-step limits and dt_hydro within the twins' tolerance, the out-of-range count the oracle's integer, every ray
    ending in the oracle's zone."""
    tr = ionmatrix.trace()
    tols, spread, twin_flips = tol
    f = GpuFollower(_grid(aa, lib, strict, ion_path))
    worst, nflip, nedge = ionmatrix.follow(tr, f, tols, label=f"strict={strict}, ion_path={ion_path}")
    print(f"12 sub-cycles (strict={strict}, ion_path={ion_path}): GPU error / twins' spread: "
          + ", ".join(f"{k} {worst[k]:.2e} / {spread[k]:.2e}" for k in ionmatrix.QUANT)
          + f"; edge zones at most {nedge} of {tr['cap']} floored on entry, {nflip} took the other branch (twins: up to {twin_flips})")
    assert nedge <= tr["cap"]
    f.g.close()


@pytest.mark.parametrize("spec", ["1", "0"])
@pytest.mark.parametrize("ion_path", PATHS)
@pytest.mark.parametrize("strict", [True, False])
def test_step_that_leaves_by_dt_hydro(aa, lib, strict, ion_path, spec, monkeypatch):
    """ifront 16x5x4, one step(): 109 sub-cycles ended by dt_hydro < dt_done with 20 zones out of range (20 rays = MAXCELLCOUNT)
    and sign-flip damping on the way (tests/test_oracle_golden.py).  In the one-kernel path this is the stop the host learns
    of one sweep late: the sweep behind it was speculative and GridS.EdgeFlux has to come from the other buffer
    (k_ion_finish).  Sub-cycle count the golden run's, dt and time within 1e-10, fields within 1e-9 of each field's maximum,
    EdgeFlux within the same bar.  (Measured: at this stop both flux buffers hold the same values -- a k_ion_finish that read the
    wrong one passes here and is caught by the EdgeFlux comparison of the phase test above; dropping the damping from the
    one-kernel update fails here.)"""
    monkeypatch.setenv("AA_ION_SPECULATE", spec)
    gz = np.load(os.path.join(GOLD, "ifront_16x5x4_n1.npz"))
    ov = [f"domain1/Nx{d + 1}={int(gz['nx'][d])}" for d in range(3)]
    run = aa.config.load(os.path.join(orc.DECKS, "athinput.ifront"), ov, "ifront")
    g = lib.setup_problem(aa.config.slab(run), 0, strict, ion_path=ion_path)
    assert g.ion_is_fused() == (ion_path == 1)
    o = orc.make_sim("ifront", ov)
    g.start(); o.start()
    ng, no = g.step(), o.step()
    assert ng == no == 109 == int(gz["niter"][0])
    assert abs(g.dt / o.dt - 1) < 1e-10 and abs(g.time / o.time - 1) < 1e-10
    a = g.download()[4:-4, 4:-4, 4:-4]; b = o.active
    scale = np.abs(b).max(axis=(0, 1, 2))
    diff = np.abs(a - b).max(axis=(0, 1, 2))
    assert np.all(diff[scale == 0] == 0)
    err = diff[scale > 0] / scale[scale > 0]
    ef = g.download_edgeflux()
    eferr = np.abs(ef - o.edgeflux).max() / np.abs(o.edgeflux).max()
    print(f"ifront 16x5x4, dt_hydro exit: fields {err.max():.2e}, EdgeFlux {eferr:.2e} of the maximum (strict={strict}, ion_path={ion_path}, spec={spec})")
    assert err.max() < 1e-9, err
    assert np.allclose(ef, o.edgeflux, rtol=1e-9, atol=1e-9 * np.abs(o.edgeflux).max())
    g.close()


@pytest.mark.parametrize("ion_path", PATHS)
@pytest.mark.parametrize("strict", [True, False])
def test_whole_step_from_the_designed_state(aa, lib, strict, ion_path):
    """One step() from the designed state against the reference's (ionmatrix_64x7x6_n1), at the tolerance of
    test_ifront_golden_fixture: same sub-cycle count, fields within 1e-8 of each field's maximum, ion fraction within 1e-8."""
    gz = np.load(os.path.join(GOLD, "ionmatrix_64x7x6_n1.npz"))
    g = _grid(aa, lib, strict, ion_path)
    g.start()
    assert abs(g.dt / float(gz["dt0"]) - 1) < 1e-12
    assert [g.step()] == [int(x) for x in gz["niter"]]
    a = g.download()[4:-4, 4:-4, 4:-4]; b = gz["U"]
    scale = np.abs(b).max(axis=(0, 1, 2))
    err = np.abs(a - b).max(axis=(0, 1, 2)) / scale
    xg = 1.0 - a[..., 5] / a[..., 0]; xr = 1.0 - b[..., 5] / b[..., 0]
    print(f"designed state, one step: fields {err.max():.2e} of the maximum, ion fraction {np.abs(xg - xr).max():.2e} (strict={strict}, ion_path={ion_path})")
    assert err.max() < 1e-8, err
    assert np.abs(xg - xr).max() < 1e-8
    g.close()
