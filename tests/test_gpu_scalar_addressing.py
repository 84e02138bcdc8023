"""The marching hydro kernels address every field as scalar base + one 32-bit zone offset + immediate (csrc/hydro_kernels.hip, field
accessors; k_correct_all, k_x1_edge_flux, k_flux2_update, k_sweep_march, k_eta_edges and their entries on the device clock).

Offsets.  aa_test_zone_offsets stores and loads through those accessors at byte offsets 0, 2^31 - 8, 2^31 and 2^32 - 8 of a 4 GiB
field, also with a scalar stride on the base: a sign-extended offset or a dropped high bit puts a word where the host's hipMemcpy
does not find it.  (The smallest Grid that could show either has 2.7e8 zones.)

Bits.  Only addresses are formed differently, so the fused chain (AA_CORRECT_ALL=1 AA_FUSED_UPDATE=1) must still give the unfused
chain's bits in the strict build, and stay within the 1e-12 of each field's maximum that tests/test_gpu_fused_update.py allows the
default build for its fused multiply-adds.  The Grid is 65 x 5 x 6: two x1 tiles (lanes 0 and 63 take halo and edge flux from
k_x1_edge_flux), two row tiles of k_correct_all and a partly filled update tile, and with AA_CA_KC=2 AA_FU_KC=2 three chunks with
provider planes.  With and without a passive scalar and a static potential, both reconstructions, padded and dense rows
(AA_PITCH_ALIGN=0: other sJ and sK); the same Grid through aa_run_3d (the entries on the device clock) and as level 0 of a two-level
Mesh (the entry that keeps flux planes, which RestrictCorrect reads back).

Run-to-run.  One case three times in one process: equal bits."""
import importlib
import os

import numpy as np
import pytest

import hydromatrix as hm
import orc

pytestmark = pytest.mark.gpu

NX = (65, 5, 6)
NSTEP = 2
FAR = 1.0e300
FUSED = {"AA_CORRECT_ALL": "1", "AA_FUSED_UPDATE": "1", "AA_CA_KC": "2", "AA_FU_KC": "2"}
UNFUSED = {"AA_CORRECT_ALL": "0", "AA_FUSED_UPDATE": "0"}


def pkg(sub=None):
    return importlib.import_module("atmospheric-athena_amd" + ("." + sub if sub else ""))


def set_knobs(monkeypatch, knobs, dense):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("AA_PITCH_ALIGN", "0" if dense else "1")


# ---- offsets --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [0, 16, 4160 * 8, 1 << 30])       # (not 8: 2^31 - 8 + 8 is the third lane's own word)
def test_accessors_reach_the_ends_of_the_32_bit_offset(stride):
    lib = pkg("lib")
    L = lib.load(False)
    stored = np.full((2, 4), -1.0)
    loaded = np.full((3, 4), -1.0)
    rc = L.aa_test_zone_offsets(stride, lib._dp(stored), lib._dp(loaded))
    assert rc == 0, L.aa_last_error().decode()
    lanes = np.arange(4.0)
    print("stored", stored.tolist(), "loaded", loaded.tolist())
    # the host finds every word where base + offset (+ stride) is in 64-bit arithmetic; with stride 0 the second store overwrote the first
    assert np.array_equal(stored[1], 2000.0 + lanes)
    assert np.array_equal(stored[0], (2000.0 if stride == 0 else 1000.0) + lanes)
    # and the accessors load the same words back: from the base, from the base moved by the stride, through the immediate
    assert np.array_equal(loaded[0], stored[0]) and np.array_equal(loaded[1], stored[1]) and np.array_equal(loaded[2], stored[0])


# ---- bits -----------------------------------------------------------------------------------------------------------------------
def make(nscal, grav, order, strict):
    """blast deck (periodic), 65 x 5 x 6, the state and the potential smooth patterns of the zone indices (tests/test_gpu_3d_run.py
    `sphere`: the potential as tables at zone centres and lower faces) -> a started Grid"""
    aa, lib = pkg(), pkg("lib")
    run = aa.config.load(os.path.join(orc.DECKS, "athinput.blast"), hm.overrides(NX), "blast", "ctu")
    run.order = order
    run.nscal = nscal
    g = lib.Grid(aa.config.slab(run), 0, strict)
    assert g.nvar == 5 + nscal
    k, j, i = (a.astype(np.float64) for a in np.meshgrid(np.arange(g.N[2]), np.arange(g.N[1]), np.arange(g.N[0]), indexing="ij"))
    if grav:
        def phi(x, y, z):
            return np.ascontiguousarray(0.02 * (x + 0.5 * y - 0.25 * z) + 0.05 * np.sin(0.3 * x) * np.cos(0.2 * y + 0.1 * z))
        tabs = [phi(i, j, k), phi(i - 0.5, j, k), phi(i, j - 0.5, k), phi(i, j, k - 0.5)]
        g._chk(g.L.aa_set_static_grav_tables(g._h, *[lib._dp(t) for t in tabs]))
    d = 1.0 + 0.3 * np.sin(0.37 * i + 0.21 * j) * np.cos(0.29 * k)
    v = [0.2 * np.sin(0.2 * i + 0.3 * j + 0.4 * k), 0.15 * np.cos(0.25 * i - 0.2 * k), 0.1 * np.sin(0.3 * j + 0.15 * k)]
    p = 1.0 + 0.2 * np.cos(0.23 * i + 0.19 * j - 0.27 * k)
    U = g.new_host_block()
    U[..., 0] = d
    for a in range(3):
        U[..., 1 + a] = d * v[a]
    U[..., 4] = p / (run.gamma - 1.0) + 0.5 * d * (v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    if nscal:
        U[..., 5] = d * (0.5 + 0.4 * np.cos(0.31 * i - 0.17 * k))
    g.upload(U)
    g.start()
    return g


def stepped(nscal, grav, order, strict, run3d=False):
    g = make(nscal, grav, order, strict)
    try:
        if run3d:
            assert g.can_run_3d()
            # (the strict build has no k_correct_all_dc with scalar and potential together: run_3d steps such a Grid by aa_step)
            assert g.run_3d_batch() > 0 or (strict and nscal and grav)
            assert g.run_3d(FAR, nstep_stop=NSTEP) == NSTEP
        else:
            for _ in range(NSTEP):
                g.step()
        return g.download(), (g.time, g.dt, g.nstep)
    finally:
        g.close()


_ref = {}


def unfused(key, monkeypatch):
    """the chain of separate kernels on the same input: run once per case and shared, never written to"""
    if key not in _ref:
        nscal, grav, order, dense, strict = key
        set_knobs(monkeypatch, UNFUSED, dense)
        U, st = stepped(nscal, grav, order, strict)
        assert np.isfinite(U).all()
        U.setflags(write=False)
        _ref[key] = (U, st)
    return _ref[key]


def hold(U, st, ref, strict, label):
    Ur, str_ = ref
    worst = 0.0
    for c in range(Ur.shape[-1]):
        scale = np.abs(Ur[..., c]).max()
        worst = max(worst, float(np.abs(U[..., c] - Ur[..., c]).max() / scale) if scale > 0 else float(np.abs(U[..., c]).max()))
    print(f"{label}: max |fused - unfused| over each field's maximum {worst:.3e}; (time, dt, nstep) {st} / {str_}")
    if strict:
        assert st == str_
        assert np.array_equal(U, Ur), (label, np.argwhere((U != Ur).any(axis=-1))[:4].tolist())
    else:
        assert st[2] == str_[2]
        assert worst <= 1e-12, (label, worst)       # fused multiply-adds only (tests/test_gpu_fused_update.py)


CASES = [(nscal, grav, order, dense) for nscal in (0, 1) for grav in (False, True) for order in (2, 3) for dense in (False, True)]


def case_id(c):
    return f"ns{c[0]}-{'grav' if c[1] else 'nograv'}-ord{c[2]}-{'dense' if c[3] else 'padded'}"


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fused_chain_gives_the_unfused_chains_bits(case, strict, monkeypatch):
    nscal, grav, order, dense = case
    ref = unfused(case + (strict,), monkeypatch)
    set_knobs(monkeypatch, FUSED, dense)
    U, st = stepped(nscal, grav, order, strict)
    hold(U, st, ref, strict, f"step {case_id(case)}")


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("case", [c for c in CASES if c[2] == 2], ids=case_id)
def test_queued_entries_give_the_unfused_chains_bits(case, strict, monkeypatch):
    """aa_run_3d: k_sweep_march_dc, k_x1_edge_flux_dc, k_correct_all_dc, k_flux2_update_dc"""
    nscal, grav, order, dense = case
    ref = unfused(case + (strict,), monkeypatch)
    set_knobs(monkeypatch, FUSED, dense)
    U, st = stepped(nscal, grav, order, strict, run3d=True)
    hold(U, st, ref, strict, f"run_3d {case_id(case)}")


def mesh_stepped(strict, nscal):
    """the Grid as level 0 of a two-level Mesh on the blast deck: a child of 16 x 2 x 4 fine zones round the blast, two root zones
    from the root's sides along x2 and x3 (the nearest init_mesh allows): kept flux planes in all three directions"""
    aa, lib = pkg(), pkg("lib")
    deck = os.path.join(orc.DECKS, "athinput.blast")
    ov = hm.smr_overrides((NX, [(1, (16, 2, 4), (56, 4, 4))]))
    par = aa.athinput.ParTable.from_file(deck).cmdline(ov)
    run = aa.config.load(deck, ov, "blast", "ctu")
    m = lib.Mesh(aa.config.levels(par, run), 0, strict)
    try:
        m.start()
        for _ in range(NSTEP):
            m.step()
        return [g.download() for g in m.lev], (m.time, m.dt, m.nstep)
    finally:
        m.close()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("dense", [False, True], ids=["padded", "dense"])
def test_level_of_a_mesh_gives_the_unfused_chains_bits(dense, strict, monkeypatch):
    """k_flux2_update<KEEP>: the second-pass fluxes on the child's outline are stored through the accessors and read back by
    RestrictCorrect"""
    set_knobs(monkeypatch, UNFUSED, dense)
    Ur, str_ = mesh_stepped(strict, 0)
    set_knobs(monkeypatch, FUSED, dense)
    U, st = mesh_stepped(strict, 0)
    assert len(U) == 2
    for l in range(2):
        assert np.isfinite(Ur[l]).all()
        hold(U[l], st, (Ur[l], str_), strict, f"mesh level {l} {'dense' if dense else 'padded'}")


# ---- run to run -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_three_runs_in_one_process_give_equal_bits(strict, monkeypatch):
    set_knobs(monkeypatch, FUSED, False)
    runs = [stepped(1, True, 2, strict) for _ in range(3)]
    for U, st in runs[1:]:
        assert st == runs[0][1] and np.array_equal(U, runs[0][0])
