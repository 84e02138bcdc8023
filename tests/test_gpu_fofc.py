"""First-order flux correction of the van Leer integrator (aa_set_fofc; the reference's --enable-fofc: integrate_3d_vl.c
Steps 10 and 14, FixCell) against the reference built with FIRST_ORDER_FLUX_CORRECTION.

The fixtures (tests/golden/make_golden_fofc.py) are pairs of restart states of near-vacuum hot bubbles of prob/blast.c around
cycles in which the reference's full update left zones with a negative density and Step 14 repaired them, with the counts it
printed in every cycle:
    A  16x12x20, steps 28 -> 36: one zone in cycles 30 and 34
    B  8x8x8,    steps 36 -> 42: one zone in cycle 39
    C  16x12x20, steps 36 -> 42 of a steeper bubble: FOUR zones in cycle 39 (the scan's order matters)
No deck made Step 10 (a NaN second-order flux) or the P < 0 branch fire: both are restated from reading only.
"""
import importlib
import os

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WINDOWS = {"A": "fofc_blast_16x12x20_s28_s36", "B": "fofc_blast_8x8x8_s36_s42", "C": "fofc_blast_16x12x20_s36_s42"}
DECK = os.path.join(orc.DECKS, "athinput.blast_fofc")
_gold = {}


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("atmospheric-athena_amd.lib")


@pytest.fixture(scope="module")
def aa():
    return importlib.import_module("atmospheric-athena_amd")


def driver():
    return importlib.import_module("atmospheric-athena_amd.driver")


def gold(w):
    if w not in _gold:
        _gold[w] = dict(np.load(os.path.join(GOLD, WINDOWS[w] + ".npz")))
    return _gold[w]


def from_state_A(aa, lib, w, strict, fofc=True):
    """The Grid with the reference's state A on board, the way tests/test_gpu_parity.py::test_from_developed_reference_state loads one."""
    gz = gold(w)
    nx = tuple(int(x) for x in gz["nx"])
    ov = [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)] + [str(o) for o in gz["overrides"]]
    run = aa.config.load(DECK, ov, "blast", "vl", fofc=fofc)
    g = lib.setup_problem(aa.config.slab(run), 0, strict)
    assert g.fofc() == fofc
    U = g.new_host_block()
    U[4:-4, 4:-4, 4:-4, :] = gz["UA"][..., :5]
    g.upload(U)
    g.set_mesh_state(float(gz["timeA"]), float(gz["dtA"]), int(gz["nstepA"]))
    g.bvals_mhd()
    return g, gz


def advance(g, nsteps):
    counts = []
    for _ in range(nsteps):
        g.step()
        counts.append(g.fofc_counts())
    return counts


def field_err(out, ref):
    """per-field max-norm error relative to the field's largest value (as test_from_developed_reference_state measures it)"""
    scale = np.abs(ref).max(axis=(0, 1, 2))
    assert np.all(out[..., scale == 0] == 0)
    return (np.abs(out - ref)[..., scale > 0] / scale[scale > 0]).max(axis=(0, 1, 2))


@pytest.mark.parametrize("predict", ["0", "1"])
@pytest.mark.parametrize("w", ["A", "B", "C"])
def test_strict_build_matches_the_reference_bit_for_bit(aa, lib, w, predict, monkeypatch):
    """Strict build, both forms of the predictor: U, time and dt at step B are the reference's bits, and every step reports the
    number of zones the reference reported (0 zones with P < 0 and 0 replaced fluxes throughout, as in the reference's runs)."""
    monkeypatch.setenv("AA_VL_PREDICT", predict)
    g, gz = from_state_A(aa, lib, w, True)
    counts = advance(g, int(gz["nstepB"]) - int(gz["nstepA"]))
    out = g.download()[4:-4, 4:-4, 4:-4, :5]
    print(w, "counts", counts, "max |dU|", float(np.abs(out - gz["UB"][..., :5]).max()))
    assert [c[0] for c in counts] == [int(c[0]) for c in gz["counts"]]
    assert [c[1] for c in counts] == [int(c[1]) for c in gz["counts"]] and all(c[2] == 0 for c in counts)
    assert g.time == float(gz["timeB"]) and g.dt == float(gz["dtB"])
    assert np.array_equal(out, gz["UB"][..., :5])
    g.close()


def test_without_the_correction_the_window_ends_elsewhere(aa, lib):
    """Window A with the switch off: the zone the update left with d < 0 stays that way or the state differs from the
    reference's -- the fixture does exercise the fix."""
    g, gz = from_state_A(aa, lib, "A", True, fofc=False)
    try:
        counts = advance(g, int(gz["nstepB"]) - int(gz["nstepA"]))
    except lib.AthenaError:
        g.close()
        return                      # (a run that stops on the bad zone also ends elsewhere)
    assert all(c == (0, 0, 0) for c in counts)
    out = g.download()[4:-4, 4:-4, 4:-4, :5]
    assert (out[..., 0] < 0).any() or not np.array_equal(out, gz["UB"][..., :5])
    g.close()


# Default (contracting) build: what it was measured to differ by from the reference's state B (the worst field, relative to that
# field's largest value); asserted at ten times that for box-to-box code generation, never looser than the
# project's 1e-6.
# Measured on an MI355X (the energy is the worst field in all three): A 6.54e-10, B 1.31e-14, C 1.45e-11.
MEASURED = {"A": 6.6e-10, "B": 1.4e-14, "C": 1.5e-11}


@pytest.mark.parametrize("w", ["A", "B", "C"])
def test_default_build_same_counts_fields_within_ten_times_measured(aa, lib, w):
    g, gz = from_state_A(aa, lib, w, False)
    counts = advance(g, int(gz["nstepB"]) - int(gz["nstepA"]))
    out = g.download()[4:-4, 4:-4, 4:-4, :5]
    err = field_err(out, gz["UB"][..., :5])
    print(w, "counts", counts, "per-field error", err, "time", g.time / float(gz["timeB"]) - 1)
    assert [c[:2] for c in counts] == [tuple(int(x) for x in c) for c in gz["counts"]] and all(c[2] == 0 for c in counts)
    assert abs(g.time / float(gz["timeB"]) - 1) < 1e-10
    bound = min(1e-6, 10.0 * MEASURED[w])
    assert err.max() < bound, (err, bound)
    g.close()


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("name,prob", [("vl_blast_16x12x20_n4", "blast"), ("vl_ioniz_sphere_20x16x12_n2", "ioniz_sphere")])
def test_switch_on_changes_nothing_where_nothing_fires(aa, lib, name, prob, strict):
    """The reference's own decks never leave a zone with d < 0: with the switch on every count is zero and the state, time and dt
    are the bits of the run with the switch off (hydro, and the ion problem with gravity, pinned zones and the passive scalar)."""
    gz = np.load(os.path.join(GOLD, name + ".npz"))
    nx = tuple(int(x) for x in gz["nx"])
    ov = [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)]
    res = []
    for fofc in (False, True):
        run = aa.config.load(os.path.join(orc.DECKS, "athinput." + prob), ov, prob, "vl", fofc=fofc)
        g = lib.setup_problem(aa.config.slab(run), 0, strict)
        g.start()
        niter, counts = [], []
        for _ in range(int(gz["nstep"])):
            niter.append(g.step()); counts.append(g.fofc_counts())
        res.append((g.download(), g.time, g.dt, niter, counts))
        if run.ion:
            res[-1] += (g.download_edgeflux(),)
        g.close()
    off, on = res
    assert all(c == (0, 0, 0) for c in on[4]) and all(c == (0, 0, 0) for c in off[4])
    assert on[1] == off[1] and on[2] == off[2] and on[3] == off[3]
    assert np.array_equal(on[0], off[0], equal_nan=True)
    if len(on) > 5:
        assert np.array_equal(on[5], off[5], equal_nan=True)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_dt_behind_a_corrected_step_is_the_references(aa, lib, fused, monkeypatch):
    """Window B, strict build: the step that corrects a zone leaves the dt the reference left (new_dt of the CORRECTED state: the
    CFL maxima the update kernel took from the uncorrected one are stale and must not be used), with the maxima riding on the
    update (the default) and with new_dt's own kernel."""
    monkeypatch.setenv("AA_CFL_FUSED", fused)
    g, gz = from_state_A(aa, lib, "B", True)
    counts = advance(g, int(gz["nstepF"]) - int(gz["nstepA"]))
    assert counts[-1][0] > 0 and all(c[0] == 0 for c in counts[:-1])
    assert g.nstep == int(gz["nstepF"]) and g.time == float(gz["timeF"])
    assert g.dt == float(gz["dtF"]), (g.dt, float(gz["dtF"]))
    g.close()


def test_refused_where_no_reference_pins_it(aa, lib):
    """aa_set_fofc refuses the CTU integrator, third-order reconstruction and Grids cut into slabs; a Mesh refuses a Grid that has it on."""
    ov = ["domain1/Nx1=8", "domain1/Nx2=8", "domain1/Nx3=8"]
    run = aa.config.load(DECK, ov, "blast", "ctu")
    g = lib.setup_problem(aa.config.slab(run), 0, False)
    with pytest.raises(lib.AthenaError, match="aa_set_fofc"):
        g.set_fofc(True)
    g.set_fofc(False)
    g.close()
    run = aa.config.load(DECK, ov, "blast", "vl")
    run.order = 3
    g = lib.setup_problem(aa.config.slab(run), 0, False)
    with pytest.raises(lib.AthenaError, match="third-order"):
        g.set_fofc(True)
    g.close()
    run = aa.config.load(DECK, ov, "blast", "vl", fofc=True)
    with pytest.raises(lib.AthenaError, match="Mesh"):
        lib.Mesh([aa.config.slab(run)])


def test_driver_reports_the_references_lines(aa, lib, capsys):
    """driver.Driver with run.fofc: the counts of every step, and the reference's line when a step corrected something."""
    gz = gold("B")
    nx = tuple(int(x) for x in gz["nx"])
    ov = [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)] + [str(o) for o in gz["overrides"]]
    run = aa.config.load(DECK, ov, "blast", "vl", fofc=True)
    d = driver().Driver(run, strict=True)
    U = d.eng.g.new_host_block()
    U[4:-4, 4:-4, 4:-4, :] = gz["UA"][..., :5]
    d.eng.g.upload(U)
    d._set_state(float(gz["timeA"]), float(gz["dtA"]), int(gz["nstepA"]))
    d.eng.bvals_local()
    for _ in range(int(gz["nstepB"]) - int(gz["nstepA"])):
        d.step()
    assert [c[:2] for c in d.fofc_trace] == [tuple(int(x) for x in c) for c in gz["counts"]]
    assert capsys.readouterr().out.count("[Step14]: 1 cells had d<0; 0 cells had P<0") == 1
    assert d.time == float(gz["timeB"]) and d.dt == float(gz["dtB"])
    d.eng.close()
