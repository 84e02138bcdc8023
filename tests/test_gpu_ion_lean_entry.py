"""The lean form of the speculating first pass of an ion step (k_ion_pass<LEAN>, AA_ION_LEAN): it stores none of the entry's dense
saves, only the E / s it overwrites and one ballot word per 64-zone tile; a lean speculation the pick refutes is redone densely by
one more launch.  Nothing of this may change a bit: every comparison here is on sub-cycle counts, the dt sequence, download() and
download_edgeflux(), exact, in both builds, against AA_ION_LEAN=0 (the dense form alone) and AA_ION_SPECULATE=0.
"""
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DECKS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "atmospheric-athena_amd", "decks")
SPHERE = ("ioniz_sphere", ["domain1/Nx1=64", "domain1/Nx2=16", "domain1/Nx3=16"])
# the four legs: (AA_ION_SPECULATE, AA_ION_LEAN)
LEGS = {"nospec": ("0", "auto"), "dense": ("1", "0"), "lean": ("1", "1"), "auto": ("1", "auto")}


@pytest.fixture(scope="module")
def aa():
    return importlib.import_module("atmospheric-athena_amd")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("atmospheric-athena_amd.lib")


def _grid(aa, lib, monkeypatch, leg, problem, ov, strict, nslab=1):
    spec, lean = LEGS[leg]
    monkeypatch.setenv("AA_ION_SPECULATE", spec)
    monkeypatch.setenv("AA_ION_LEAN", lean)
    run = aa.config.load(os.path.join(DECKS, "athinput." + problem), ov, problem)
    g = lib.setup_problem(aa.config.slab(run), 0, strict, nslab=nslab)
    assert g.ion_is_fused()
    return g


def _run(aa, lib, monkeypatch, leg, problem, ov, nstep, strict, nslab=1):
    g = _grid(aa, lib, monkeypatch, leg, problem, ov, strict, nslab)
    g.start()
    its, dts = [], []
    for _ in range(nstep):
        its.append(g.step()); dts.append(g.dt)
    out = (its, dts, g.download(), g.download_edgeflux(), g.ion_lean_counts())
    g.close()
    return out


def _same(a, b, what):
    assert a[0] == b[0], f"{what}: sub-cycle counts {a[0]} / {b[0]}"
    assert a[1] == b[1], f"{what}: dt sequence"
    assert np.array_equal(a[2], b[2], equal_nan=True), f"{what}: state"
    assert np.array_equal(a[3], b[3], equal_nan=True), f"{what}: EdgeFlux"


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("problem,ov,nstep", [
    (SPHERE[0], SPHERE[1], 12),                 # many sub-cycles in the first steps, then 1 per step
    ("ifront", ["domain1/Nx1=64", "domain1/Nx2=8", "domain1/Nx3=8", "problem/flux=1e3"], 5),
    ("ifront", ["domain1/Nx1=128", "domain1/Nx2=6", "domain1/Nx3=5"], 4),
    # a row that is no multiple of 64: the tail tile's ballot has 48 idle lanes (the CPU oracle runs this deck at this size
    # with 26, 26, 11, 9 sub-cycles in its first four steps: every speculation is refuted)
    ("ifront", ["domain1/Nx1=80", "domain1/Nx2=6", "domain1/Nx3=5"], 4)])
def test_lean_entry_changes_no_bit(aa, lib, problem, ov, nstep, strict, monkeypatch):
    """AA_ION_LEAN = 0 / 1 / auto and AA_ION_SPECULATE=0 give the same counts, dt, state and EdgeFlux.  With 1 every speculating
    step is lean, so every refuted one goes through the redo launch; with auto the first confirmed step switches dense -> lean."""
    r = {leg: _run(aa, lib, monkeypatch, leg, problem, ov, nstep, strict) for leg in LEGS}
    for leg in ("dense", "lean", "auto"):
        _same(r[leg], r["nospec"], f"{leg} against AA_ION_SPECULATE=0")
    its = r["nospec"][0]
    n = {leg: r[leg][4] for leg in LEGS}
    print(f"{problem} {ov}: sub-cycles {its}; (dense, lean, redone) = {n}")
    assert n["nospec"] == (0, 0, 0)
    assert n["dense"] == (nstep, 0, 0)
    # forced: every step lean, and exactly those with more than one sub-cycle or a refuted single one were redone
    assert n["lean"][:2] == (0, nstep) and n["lean"][2] >= sum(1 for i in its if i > 1)
    # auto: lean exactly behind the steps that took one sub-cycle
    assert n["auto"][1] == sum(1 for i in its[:-1] if i == 1) and n["auto"][0] == nstep - n["auto"][1]
    if problem == "ioniz_sphere":
        assert 1 in its[:-1] and max(its) > 1
        assert n["lean"][2] >= 1 and n["lean"][2] < nstep        # the redo ran, and confirmed lean steps went without it
        assert n["auto"][0] >= 1 and n["auto"][1] >= 1           # both forms ran
    if ov[0] == "domain1/Nx1=80":
        assert min(its) > 1 and n["lean"][2] == nstep


def _ion_step_by_hand(g, limit):
    """one ion step through the phases; -> the steps applied"""
    g.ion_begin()
    g.ion_speculate(limit)
    g.ion_pass(False, True)
    g.ion_pick(0, 1, True, limit)
    dts = []
    for _ in range(400):
        g.ion_pass(True, True)
        g.ion_pick(0, 1, False, limit)
        dt, hit = g.ion_fetch()[:2]
        dts.append(dt)
        if hit:
            break
    g.ion_finish()
    return dts


@pytest.mark.parametrize("strict", [True, False])
def test_lean_step_refuted_after_confirmed_ones(aa, lib, strict, monkeypatch):
    """auto, lean -> dense: seven steps of the sphere (the last ones take one sub-cycle, so the next is lean), then three ion steps
    by hand: one whose limit is ten times the hydro step, one with a thousand times, one with the hydro step again.  At that point
    of the run the chemistry allows 112 hydro steps (CPU oracle: dt_chem 5831 against dt 52.08), so the ten-fold step still stands
    after one sub-cycle; the thousand-fold one cannot, and is the lean step that is refuted after a run of confirmed ones.
    Against the same calls under AA_ION_LEAN=0."""
    out = {}
    for leg in ("dense", "auto"):
        g = _grid(aa, lib, monkeypatch, leg, SPHERE[0], SPHERE[1], strict)
        g.start()
        its = [g.step() for _ in range(7)]
        assert its[-2:] == [1, 1], its
        res, counts = [], [g.ion_lean_counts()]
        for factor in (10.0, 1000.0, 1.0):
            dts = _ion_step_by_hand(g, factor * g.dt)
            res.append((dts, g.download(), g.download_edgeflux()))
            counts.append(g.ion_lean_counts())
        out[leg] = (its, res, counts)
        g.close()
    a, d = out["auto"], out["dense"]
    print("sub-cycles of the three steps by hand:", [len(r[0]) for r in d[1]], "counts (auto):", a[2])
    assert len(d[1][1][0]) > 1, "the thousand-fold step was meant to take more than one sub-cycle"
    assert a[0] == d[0]
    for ra, rd in zip(a[1], d[1]):
        assert ra[0] == rd[0]
        assert np.array_equal(ra[1], rd[1], equal_nan=True) and np.array_equal(ra[2], rd[2], equal_nan=True)
    c = a[2]
    assert c[1][1] == c[0][1] + 1                                       # the ten-fold step was lean ...
    assert c[1][2] == c[0][2] + (1 if len(d[1][0][0]) > 1 else 0)       # ... and redone only if it was refuted
    assert len(d[1][0][0]) > 1 or (c[2][1] == c[1][1] + 1 and c[2][2] == c[1][2] + 1)     # the thousand-fold one: lean, refuted, redone
    assert c[3][0] == c[2][0] + 1 and c[3][1:] == c[2][1:]              # ... and the step behind it was dense again
    assert d[2][3][1:] == (0, 0)


@pytest.mark.parametrize("strict", [True, False])
def test_lean_entry_on_slabs(aa, lib, strict, monkeypatch):
    """a Grid cut into two slabs inside the library, over enough steps to reach those with one sub-cycle.  Every slab would decide
    from the gathered pick, so all take the same form -- but the composite handle's launch choices are zeroed (slabs_create), its
    aa_ion_speculate therefore returns at once and a cut Grid never speculates: neither form runs there, and the knob must not
    matter.  Where speculation does run on slabs, the forms must have been used as on one Grid."""
    r = {leg: _run(aa, lib, monkeypatch, leg, SPHERE[0], SPHERE[1], 8, strict, nslab=2) for leg in ("dense", "auto", "lean")}
    _same(r["auto"], r["dense"], "two slabs, auto")
    _same(r["lean"], r["dense"], "two slabs, forced")
    its = r["dense"][0]
    assert 1 in its[:-1]
    print("two slabs: sub-cycles", its, "(dense, lean, redone):", {leg: r[leg][4] for leg in r})
    assert r["dense"][4][1:] == (0, 0)
    if sum(r["dense"][4]) > 0:           # (speculation on a cut Grid)
        assert r["auto"][4][1] == sum(1 for i in its[:-1] if i == 1) and r["lean"][4][2] >= 1
    else:
        assert r["auto"][4] == (0, 0, 0) and r["lean"][4] == (0, 0, 0)


@pytest.mark.parametrize("strict", [True, False])
def test_lean_entry_on_mesh_levels(aa, lib, strict, monkeypatch):
    """the two-level sphere of tests/test_gpu_smr.py (32^3 root; the rays are short, so the one-kernel sub-cycle is forced): the
    levels decide one by one -- the root reaches one sub-cycle per step after 17 steps while the fine level stays at ten"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smr_ioniz_sphere_2lev_s4.npz"))
    ov = [str(o) for o in g["overrides"]]
    monkeypatch.setenv("AA_ION_FUSED", "1")
    out = {}
    for leg in ("dense", "auto", "lean"):
        monkeypatch.setenv("AA_ION_SPECULATE", LEGS[leg][0]); monkeypatch.setenv("AA_ION_LEAN", LEGS[leg][1])
        par = aa.athinput.ParTable.from_file(os.path.join(DECKS, "athinput.ioniz_sphere")).cmdline(ov)
        run = aa.config.from_par(par, "ioniz_sphere")
        m = lib.Mesh(aa.config.levels(par, run), 0, strict)
        try:
            assert all(lev.ion_is_fused() for lev in m.lev)
            m.start()
            niter = [m.step() for _ in range(20)]
            out[leg] = (niter, m.dt, [lev.download() for lev in m.lev], [lev.download_edgeflux() for lev in m.lev],
                        [lev.ion_lean_counts() for lev in m.lev])
        finally:
            m.close()
    d = out["dense"]
    for leg in ("auto", "lean"):
        a = out[leg]
        assert a[0] == d[0] and a[1] == d[1], leg
        for l in range(2):
            assert np.array_equal(a[2][l], d[2][l], equal_nan=True), (leg, l)
            assert np.array_equal(a[3][l], d[3][l], equal_nan=True), (leg, l)
    print("sub-cycles per step and level:", d[0], "counts:", {leg: out[leg][4] for leg in out})
    assert [n[0] for n in d[0][-2:]] == [1, 1] and min(n[1] for n in d[0]) > 1
    assert out["auto"][4][0][1] >= 1 and out["auto"][4][1][1] == 0       # root lean, fine level never
    assert all(c[2] >= 1 for c in out["lean"][4])                        # forced: both levels redone at least once
