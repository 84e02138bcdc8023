"""The fused kernels of the CTU chain (csrc/hydro_kernels.hip) against the unfused chain and the CPU oracle:
k_flux2_update (AA_FUSED_UPDATE: second-pass fluxes + update) and k_correct_all (AA_CORRECT_ALL: the
correct passes of the three directions, per cell).

Strict build: the fused kernel evaluates the same expressions in the same order per zone, so both
chains must agree BIT FOR BIT with each other and with the oracle, on sizes that are not multiples
of the block tile (63 x 7 zones x chunk) and with gravity + a passive scalar (ioniz_sphere)."""
import importlib
import os

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECKS = os.path.join(ROOT, "atmospheric-athena_amd", "decks")


def run_gpu(problem, ov, strict, fused, nstep, monkeypatch, order=2):
    """fused: False = separate kernels; True = k_flux2_update; "all" = k_correct_all + k_flux2_update; "all+x3" = the
    same with the x3 first pass inside k_correct_all (AA_X3_FUSED; the library's default since round 3, forced either way here)"""
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    monkeypatch.setenv("AA_FUSED_UPDATE", "1" if fused else "0")
    monkeypatch.setenv("AA_CORRECT_ALL", "1" if fused in ("all", "all+x3") else "0")
    monkeypatch.setenv("AA_X3_FUSED", "1" if fused == "all+x3" else "0")
    run = aa.config.load(os.path.join(DECKS, "athinput." + problem), ov, problem)
    run.order = order
    g = lib.setup_problem(aa.config.slab(run), 0, strict)
    g.start()
    its = [g.step() for _ in range(nstep)]
    U = g.download()
    st = g.mesh_state()
    g.close()
    return U, its, st


CASES = [("blast", ["domain1/Nx1=70", "domain1/Nx2=23", "domain1/Nx3=37"], 3),
         ("blast", ["domain1/Nx1=128", "domain1/Nx2=8", "domain1/Nx3=4"], 2),
         ("ioniz_sphere", ["domain1/Nx1=32", "domain1/Nx2=32", "domain1/Nx3=32", "problem/rp=2.1e10"], 2),
         ("ifront", ["domain1/Nx1=66", "domain1/Nx2=9", "domain1/Nx3=15"], 2)]


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mode", [True, "all", "all+x3"])
@pytest.mark.parametrize("problem,ov,nstep", CASES)
def test_fused_equals_unfused_bitwise_strict(problem, ov, nstep, mode, order, monkeypatch):
    a, ia, sa = run_gpu(problem, ov, True, False, nstep, monkeypatch, order)
    b, ib, sb = run_gpu(problem, ov, True, mode, nstep, monkeypatch, order)
    assert ia == ib and sa == sb
    assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("mode", [True, "all", "all+x3"])
@pytest.mark.parametrize("problem,ov,nstep", CASES[:2])
def test_fused_vs_oracle_bitwise(problem, ov, nstep, mode, monkeypatch):
    U, its, st = run_gpu(problem, ov, True, mode, nstep, monkeypatch)
    o = orc.make_sim(problem, ov)
    o.start()
    for _ in range(nstep):
        o.step()
    assert np.array_equal(U[4:-4, 4:-4, 4:-4, :5], o.active[..., :5])


@pytest.mark.parametrize("mode", [True, "all", "all+x3"])
@pytest.mark.parametrize("problem,ov,nstep", CASES)
def test_fused_fast_build_within_rounding(problem, ov, nstep, mode, monkeypatch):
    a, ia, sa = run_gpu(problem, ov, False, False, nstep, monkeypatch)
    b, ib, sb = run_gpu(problem, ov, False, mode, nstep, monkeypatch)
    assert ia == ib
    for c in range(a.shape[-1]):
        scale = np.nanmax(np.abs(a[..., c]))
        if scale == 0:
            assert np.all(b[..., c] == 0)
        else:
            assert np.nanmax(np.abs(a[..., c] - b[..., c])) <= 1e-12 * scale     # fused multiply-adds only


@pytest.mark.parametrize("problem,n,nstep", [("ioniz_sphere", 48, 10), ("ifront", 32, 8), ("blast", 40, 10)])
def test_every_fused_kernel_on_against_every_one_off_strict(problem, n, nstep, monkeypatch):
    """Big-Grid defaults (k_correct_all, k_flux2_update, rates inside the ray sweep) forced on at a small
    size, against the chain with none of them, over enough steps for the radiation to sub-cycle a few dozen
    times: same sub-cycle counts, time, dt, state and EdgeFlux, bit for bit."""
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    out = []
    for on in ("0", "1"):
        for k in ("AA_FUSED_UPDATE", "AA_CORRECT_ALL", "AA_FUSED_RATES", "AA_X3_FUSED"):
            monkeypatch.setenv(k, on)
        run = aa.config.load(os.path.join(DECKS, "athinput." + problem), [f"domain1/Nx{d}={n}" for d in (1, 2, 3)], problem)
        g = lib.setup_problem(aa.config.slab(run), 0, True)
        g.start()
        its = [g.step() for _ in range(nstep)]
        out.append((g.download(), g.download_edgeflux() if run.ion else np.zeros(1), its, g.mesh_state()))
        g.close()
    a, b = out
    assert a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


@pytest.mark.parametrize("x3", ["0", "1"])
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("problem,ov", [(c[0], c[1]) for c in CASES])
def test_integrate_begin_changes_no_bit(problem, ov, strict, x3, monkeypatch):
    """aa_integrate_begin (the first-pass x1 / x2 sweeps of the planes ks..ke, for a driver that has the x3 halo in
    flight) followed by aa_integrate_3d_ctu against aa_integrate_3d_ctu alone: every pencil of those sweeps is on
    its own, so the split must not change a bit in either build."""
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    monkeypatch.setenv("AA_FUSED_UPDATE", "1")
    monkeypatch.setenv("AA_CORRECT_ALL", "1")
    monkeypatch.setenv("AA_X3_FUSED", x3)
    out = []
    for split in (False, True):
        run = aa.config.load(os.path.join(DECKS, "athinput." + problem), ov, problem)
        g = lib.setup_problem(aa.config.slab(run), 0, strict)
        g.start()
        for _ in range(2):
            if split:
                g.integrate_begin()
            g.integrate_3d_ctu()
            g.bvals_mhd()
            g.new_dt()
        out.append((g.download(), g.mesh_state()))
        g.close()
    assert out[0][1] == out[1][1]
    assert np.array_equal(out[0][0], out[1][0], equal_nan=True)


@pytest.mark.parametrize("integrator", ["ctu", "vl"])
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("problem,ov,nstep", [(c[0], c[1], 4) for c in CASES])
def test_new_dt_maxima_from_the_update_kernel(problem, ov, nstep, strict, integrator, monkeypatch):
    """AA_CFL_FUSED: k_flux2_update leaves max(|v_d| + a) of the zones it has just updated behind (pinned zones excepted,
    which k_pinned_cfl adds after Userwork has overwritten them: ioniz_sphere's core), new_dt reads that instead of sweeping
    the Grid with k_cfl.  MAX of the same non-negative doubles: the dt sequence and the state are the same, bit for bit, in
    BOTH builds (cfl_zone is compiled without multiply-add contraction everywhere: ADVICE r02).  The van Leer integrator's
    k_update does the same (block maxima to a scratch array, folded by k_cfl_fold)."""
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    monkeypatch.setenv("AA_FUSED_UPDATE", "1")
    out = []
    for on in ("0", "2"):                       # 2: also in the strict build (which keeps k_cfl by default)
        monkeypatch.setenv("AA_CFL_FUSED", on)
        run = aa.config.load(os.path.join(DECKS, "athinput." + problem), ov, problem, integrator)
        g = lib.setup_problem(aa.config.slab(run), 0, strict)
        g.start()
        its, dts = [], []
        for _ in range(nstep):
            its.append(g.step()); dts.append(g.dt)
        out.append((g.download(), its, dts))
        g.close()
    assert out[0][1] == out[1][1]
    assert out[0][2] == out[1][2]
    assert np.array_equal(out[0][0], out[1][0], equal_nan=True)


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("problem,nx1", [("blast", 46), ("blast", 47), ("blast", 48), ("ioniz_sphere", 110), ("ioniz_sphere", 111),
                                         ("ifront", 130), ("blast", 520), ("ioniz_sphere", 1039)])
def test_x1_first_pass_inside_correct_all_at_the_tile_edges(problem, nx1, order, monkeypatch):
    """Round 4: with the x3 first pass on board k_correct_all also does the x1 first pass (hydro_kernels.hip k_correct_all<X3F>): the right state
    of a zone's upper face comes from the lane above, the flux of the face between two 64-zone tiles (zone is - 16 + 64 b) from
    k_x1_edge_flux.  Sizes that put the last face the kernel needs (ie + 2) exactly on such an edge (Nx1 = 47, 111), one zone
    before it (46, 110) and one behind (48), three tiles (130), nine (520) and seventeen with the last face on an edge (1039): bit for bit the chain of separate kernels, strict build, both
    reconstructions; AA_X3_FUSED=0 runs the same kernel WITHOUT either first pass on board."""
    ov = [f"domain1/Nx1={nx1}", "domain1/Nx2=9", "domain1/Nx3=11"]
    if problem == "ioniz_sphere":
        ov.append("problem/rp=2.1e10")
    a, ia, sa = run_gpu(problem, ov, True, False, 2, monkeypatch, order)
    b, ib, sb = run_gpu(problem, ov, True, "all+x3", 2, monkeypatch, order)
    c, ic, sc = run_gpu(problem, ov, True, "all", 2, monkeypatch, order)
    monkeypatch.setenv("AA_EDGE_OVERLAP", "1")          # k_x1_edge_flux on a side stream beside the x2 sweep (api.hip; off by default)
    d, id_, sd = run_gpu(problem, ov, True, "all+x3", 2, monkeypatch, order)
    assert ia == ib == ic == id_ and sa == sb == sc == sd
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True) and np.array_equal(a, d, equal_nan=True)
