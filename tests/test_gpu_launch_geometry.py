"""Launch geometry at the values the big Grids take, forced on small Grids.

The library picks planes per block, march chunk lengths, block caps and zone order by Grid size (csrc/grid.h LaunchCfg,
read once per Grid in aa_create).  The oracle tests run on Grids of up to about 128^3, where the heuristics never choose what a
512^3 step runs: k_correct_all with 64 planes per block, k_flux2_update and k_vl_predict with 32, k_sweep_march with 32 faces per
thread, k_ion_pass with 16 rays per wave, k_update in strips.  Each test here forces one of those choices on a deck whose shape
puts a chunk, strip or ray boundary where it matters, and compares with

  (a) the CPU oracle (tests/orc.py), and
  (b) the same build at the geometry the size picks (module-scoped cache: one short GPU run per knob value).

Strict build (-ffp-contract=off): bit for bit against (b) for every knob value; against the oracle bit for bit on hydro-only decks,
within the tolerances of test_gpu_parity's ion tests on the ion decks.  Default build: bit for bit against (b) where the knob does
not move a chunk boundary (ion block cap, zone order, row pitch, mailbox spin, fused ion begin: the same compiled code does the
same arithmetic per zone); where it does, within the bound of test_slabs_inside_the_library_equal_one_grid (1e-13 blast / ifront,
1e-8 sphere: a chunk's peeled first iteration may be contracted differently)."""
import contextlib
import importlib
import math
import os

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECKS = os.path.join(ROOT, "atmospheric-athena_amd", "decks")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BUILDS = pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])


@contextlib.contextmanager
def environ(knobs):
    """set the AA_* knobs for the Grids created inside (aa_create reads them), restore afterwards"""
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update({k: str(v) for k, v in knobs.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def overrides(nx, extra=()):
    return [f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)] + list(extra)


def gpu_run(problem, nx, nstep, strict, knobs, integrator="ctu", order=2, extra=()):
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    with environ(knobs):
        run = aa.config.load(os.path.join(DECKS, "athinput." + problem), overrides(nx, extra), problem, integrator)
        run.order = order
        g = lib.setup_problem(aa.config.slab(run), 0, strict)
    try:
        g.start()
        its, dts = [], []
        for _ in range(nstep):
            its.append(g.step()); dts.append(g.dt)
        return {"U": g.download(), "its": its, "dts": dts, "state": g.mesh_state(), "syncs": g.host_syncs(),
                "ef": g.download_edgeflux() if run.ion else None, "nv": 5 + run.nscal}
    finally:
        g.close()


@pytest.fixture(scope="module")
def ref():
    """(b): the same deck at the geometry the size picks (only the knobs that select the kernel chain set), once per module"""
    cache = {}

    def get(problem, nx, nstep, strict, knobs=(), integrator="ctu", order=2, extra=()):
        key = (problem, nx, nstep, strict, tuple(sorted(dict(knobs).items())), integrator, order, tuple(extra))
        if key not in cache:
            cache[key] = gpu_run(problem, nx, nstep, strict, dict(knobs), integrator, order, extra)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def oracle():
    """(a): the CPU oracle, once per deck and module"""
    cache = {}

    def get(problem, nx, nstep, integrator="ctu", order=2, extra=()):
        key = (problem, nx, nstep, integrator, order, tuple(extra))
        if key not in cache:
            o = orc.make_sim(problem, overrides(nx, extra), integrator=integrator, order=order)
            o.start()
            its, dts = [], []
            for _ in range(nstep):
                its.append(o.step()); dts.append(o.dt)
            cache[key] = {"U": o.active.copy(), "its": its, "dts": dts, "time": o.time, "ef": o.edgeflux.copy()}
        return cache[key]
    return get


def relerr(a, b):
    """max |a-b| / max|b| per variable"""
    out = []
    for c in range(a.shape[-1]):
        scale = np.nanmax(np.abs(b[..., c]))
        out.append(0.0 if scale == 0 else float(np.nanmax(np.abs(a[..., c] - b[..., c])) / scale))
    return out


def assert_same_bits(a, b):
    assert a["its"] == b["its"] and a["dts"] == b["dts"] and a["state"] == b["state"]
    assert np.array_equal(a["U"], b["U"], equal_nan=True), relerr(a["U"], b["U"])
    if a["ef"] is not None:
        assert np.array_equal(a["ef"], b["ef"], equal_nan=True)


def assert_close(a, b, tol):
    assert a["its"] == b["its"]
    assert all(abs(x / y - 1) <= tol for x, y in zip(a["dts"], b["dts"])), (a["dts"], b["dts"])
    assert np.array_equal(np.isnan(a["U"]), np.isnan(b["U"]))
    err = relerr(a["U"], b["U"])
    assert max(err) <= tol, err
    if a["ef"] is not None:
        assert max(relerr(a["ef"][..., None], b["ef"][..., None])) <= tol


def assert_vs_oracle(r, o, problem, strict):
    """hydro-only decks in the strict build: bit for bit; the ion decks: test_ifront_vs_oracle / test_ioniz_sphere_vs_oracle"""
    nv = r["nv"]
    U = r["U"][4:-4, 4:-4, 4:-4, :nv]
    assert r["its"] == o["its"], (r["its"], o["its"])
    if problem == "blast":
        if strict:
            assert np.array_equal(U, o["U"][..., :nv]) and r["dts"] == o["dts"]
        else:
            assert max(relerr(U, o["U"][..., :nv])) < 1e-11
        return
    tol = 1e-9 if problem == "ifront" else 1e-8
    assert all(abs(x / y - 1) < 1e-9 for x, y in zip(r["dts"], o["dts"]))
    assert np.array_equal(np.isnan(U), np.isnan(o["U"][..., :nv]))
    err = relerr(U, o["U"][..., :nv])
    assert max(err) < tol, err
    assert np.allclose(r["ef"], o["ef"], rtol=tol, atol=tol * np.abs(o["ef"]).max())


def chunk_tol(problem):
    return 1e-8 if problem == "ioniz_sphere" else 1e-13


# ---- 1. k_correct_all: planes per block -------------------------------------------------------------------------------
# Nx1 = 70: two x1 tiles of 64 (an x1 edge face inside the Grid); Nx2 = 9.  The zones s-1 .. e+1 along x3 are Nx3 + 2 planes:
# Nx3 = 62 -> exactly one chunk of 64 (the 512^3 chunk length), 63 -> 64 + a one-plane tail, 70 -> 64 + 8.  Odd kc (1, 3, 7)
# are the only way to start chunks on odd planes (the PARK3 slot alternation pk = (k & 1) ? 12 : 0 starts on an even plane for
# every power of two).
CA_DECKS = [("blast", (70, 9, 62), 2, 2), ("blast", (70, 9, 63), 2, 3), ("blast", (70, 9, 70), 2, 2),
            ("blast", (70, 9, 62), 2, 3), ("blast", (70, 9, 63), 2, 2), ("blast", (70, 9, 70), 2, 3),
            ("ioniz_sphere", (70, 9, 63), 2, 2),      # 6 variables + gravity (PARK2): the instantiation the headline step runs
            ("ifront", (66, 9, 15), 3, 2)]            # scalar, no gravity
CA_EXTRA = {"ioniz_sphere": ("problem/rp=2.1e10",)}
CA_IDS = [f"{p}-{n[0]}x{n[1]}x{n[2]}-o{o}" for p, n, _, o in CA_DECKS]


@BUILDS
@pytest.mark.parametrize("kc", [1, 2, 3, 7, 64])
@pytest.mark.parametrize("x3f", ["1", "0"])
@pytest.mark.parametrize("deck", CA_DECKS, ids=CA_IDS)
def test_correct_all_planes_per_block(deck, x3f, kc, strict, ref, oracle):
    """AA_CA_KC: k_correct_all (47 % of the 512^3 step, 64 planes per block there; 8 on the Grids of the oracle tests) with
    1, 2, 3, 7 and 64 planes per block, with and without the x3 first pass on board (AA_X3_FUSED)."""
    problem, nx, nstep, order = deck
    extra = CA_EXTRA.get(problem, ())
    chain = {"AA_CORRECT_ALL": "1", "AA_X3_FUSED": x3f}
    r = gpu_run(problem, nx, nstep, strict, dict(chain, AA_CA_KC=kc), order=order, extra=extra)
    b = ref(problem, nx, nstep, strict, chain, order=order, extra=extra)
    if strict:
        assert_same_bits(r, b)
    else:
        assert_close(r, b, chunk_tol(problem))
    if strict or problem != "blast":
        assert_vs_oracle(r, oracle(problem, nx, nstep, order=order, extra=extra), problem, strict)


# ---- 2. k_flux2_update: planes per block -------------------------------------------------------------------------------
FU_DECKS = [CA_DECKS[0], CA_DECKS[1], CA_DECKS[2], CA_DECKS[6], CA_DECKS[7]]


@BUILDS
@pytest.mark.parametrize("kc", [1, 2, 3, 7, 32])
@pytest.mark.parametrize("deck", FU_DECKS, ids=[CA_IDS[i] for i in (0, 1, 2, 6, 7)])
def test_flux2_update_planes_per_block(deck, kc, strict, ref, oracle):
    """AA_FU_KC: k_flux2_update (32 planes per block at 512^3, 4 on the oracle tests' Grids) with 1, 2, 3, 7 and 32, behind
    k_correct_all with its x3 first pass (the headline chain).  Every chunk boundary is a kept x3 face the two blocks either
    side of it must not both write (round 4's two-writer race sat on such a boundary).  Nx3 = 62 / 63 / 70 leave 30, 31 and 6
    planes in the last chunk of 32."""
    problem, nx, nstep, order = deck
    extra = CA_EXTRA.get(problem, ())
    chain = {"AA_CORRECT_ALL": "1", "AA_X3_FUSED": "1", "AA_FUSED_UPDATE": "1"}
    r = gpu_run(problem, nx, nstep, strict, dict(chain, AA_FU_KC=kc), order=order, extra=extra)
    b = ref(problem, nx, nstep, strict, chain, order=order, extra=extra)
    if strict:
        assert_same_bits(r, b)
        assert_vs_oracle(r, oracle(problem, nx, nstep, order=order, extra=extra), problem, strict)
    else:
        assert_close(r, b, chunk_tol(problem))


# ---- 3. march chunks (k_sweep_march, k_slopes_march) and k_vl_predict -------------------------------------------------------
# Nx2 = 37: 40 x2 interfaces per column (32 + 8; 7: five chunks and a 5-face tail), 44 slope cells; Nx3 = 29: 33 x3 interfaces,
# 36 zones for k_vl_predict (32 + 4).  At 512^3 both take 32 (516 faces: 16 x 32 + 4); here the size picks 4 or 8.
MARCH_NX = (20, 37, 29)


@BUILDS
@pytest.mark.parametrize("chunk", [4, 7, 32])
@pytest.mark.parametrize("integrator,order", [("ctu", 2), ("ctu", 3), ("vl", 2), ("vl", 3)])
def test_march_chunk_lengths(integrator, order, chunk, strict, ref, oracle):
    """AA_SW_CHUNK: interfaces per thread of the x2 / x3 first-pass marches (k_sweep_march, in the headline chain for x2) and
    cells per thread of k_slopes_march (third order); AA_VP_KC: planes per block of k_vl_predict (forced on with AA_VL_PREDICT,
    which 512^3 VL runs pick by size)."""
    knobs = {"AA_VL_PREDICT": "1"} if integrator == "vl" else {}
    r = gpu_run("blast", MARCH_NX, 3, strict, dict(knobs, AA_SW_CHUNK=chunk, AA_VP_KC=chunk), integrator, order)
    b = ref("blast", MARCH_NX, 3, strict, knobs, integrator, order)
    if strict:
        assert_same_bits(r, b)
    else:
        assert_close(r, b, 1e-13)
    assert_vs_oracle(r, oracle("blast", MARCH_NX, 3, integrator, order), "blast", strict)


@pytest.mark.parametrize("knob,value", [("AA_SW_CHUNK", -1), ("AA_SW_CHUNK", 4097), ("AA_VP_KC", -2), ("AA_VP_KC", 100000)])
def test_march_chunk_knobs_refuse_what_no_kernel_takes(knob, value):
    """grid.h LaunchCfg: AA_SW_CHUNK and AA_VP_KC take 0 (by size) or 1 .. 4096; aa_create refuses anything else, loudly."""
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    with pytest.raises(lib.AthenaError, match=knob):
        gpu_run("blast", (8, 8, 8), 1, False, {knob: value})
    gpu_run("blast", (8, 8, 8), 1, False, {knob: 4096})


# ---- 4. the ion step at production block counts ---------------------------------------------------------------------------
# k_ion_pass runs at most AA_ION_PASS_BLOCKS blocks of 4 waves, a wave per ray; beyond that every wave loops over rays,
# prefetching the next ray's first tile and resetting carry / cut / dead at its start.  512^3 has 16 rays per wave; a cap of
# 1, 2, 3, 5 blocks gives 4 .. 16 here.
ION_DECKS = [("ifront", (64, 9, 7), 3),            # 63 rays: not a multiple of the 4 waves of a block
             ("ifront", (130, 6, 5), 3),           # three 64-zone tiles per ray: the prefetch crosses from a ray's third tile
             ("ioniz_sphere", (64, 16, 16), 12)]   # 80, 13, 12, 11, 10 sub-cycles, then 1 per step: both kinds of speculated step


@BUILDS
@pytest.mark.parametrize("cap", [1, 2, 3, 5])
@pytest.mark.parametrize("deck", ION_DECKS, ids=lambda d: f"{d[0]}-{d[1][0]}x{d[1][1]}x{d[1][2]}")
def test_ion_pass_with_several_rays_per_wave(deck, cap, strict, ref, oracle):
    """AA_ION_PASS_BLOCKS: the one-kernel sub-cycle with several rays per wave.  Same sub-cycle counts, time, dt, state and
    EdgeFlux as the default cap, bit for bit in both builds: a ray's arithmetic does not depend on which wave carries it."""
    problem, nx, nstep = deck
    r = gpu_run(problem, nx, nstep, strict, {"AA_ION_PASS_BLOCKS": cap, "AA_ION_FUSED": "1"})
    b = ref(problem, nx, nstep, strict, {"AA_ION_FUSED": "1"})
    assert_same_bits(r, b)
    if problem == "ioniz_sphere":
        assert 1 in r["its"] and max(r["its"]) > 1
    if problem == "ifront":     # (the sphere's 12 steps sit beyond the 1- and 2-step horizon of the oracle tolerances)
        assert_vs_oracle(r, oracle(problem, nx, nstep), problem, strict)


# ---- 5. zone order of the unfused stencil kernels ---------------------------------------------------------------------------
@BUILDS
@pytest.mark.parametrize("strip,xcd", [(s, x) for s in (0, 1, 5, 7) for x in (0, 1)])
@pytest.mark.parametrize("nx2", [17, 23])
@pytest.mark.parametrize("integrator", ["ctu", "vl"])
def test_zone_order_of_the_unfused_kernels(integrator, nx2, strip, xcd, strict, ref, oracle):
    """AA_STRIP / AA_XCD: k_flux2 + k_update (AA_FUSED_UPDATE=0) and the van Leer k_update walk the zones in strips of x2 rows,
    which only Grids with more than 64 x2 zones take by default (VL at 512^3).  Nx2 = 17 and 23 leave last strips of 2 / 3
    rows (strip 5) and 3 / 2 rows (strip 7).  Only the order changes: the same bits in both builds."""
    nx = (20, nx2, 10)
    knobs = {"AA_FUSED_UPDATE": "0"}
    r = gpu_run("blast", nx, 2, strict, dict(knobs, AA_STRIP=strip, AA_XCD=xcd), integrator)
    assert_same_bits(r, ref("blast", nx, 2, strict, knobs, integrator))
    if strict:
        assert_vs_oracle(r, oracle("blast", nx, 2, integrator), "blast", strict)


# ---- 6. dense rows ----------------------------------------------------------------------------------------------------------
@BUILDS
@pytest.mark.parametrize("nx1", [24, 56, 37, 70])
@pytest.mark.parametrize("chain", ["ctu-big", "vl", "ppm", "ifront"])
def test_dense_rows(chain, nx1, strict, ref):
    """AA_PITCH_ALIGN=0: rows of N1 doubles instead of a multiple of 16 shifted by 12.  Nx1 = 24 and 56 make N1 a multiple of 16
    with field offset 0, so march_shift takes its "aligned" branch on dense rows; 37 and 70 do not.  The big-Grid CTU kernels
    (k_correct_all, k_flux2_update), VL, PPM and the one-kernel ion sub-cycle.  Addresses only: the same bits in both builds."""
    problem, integ, order, knobs = {
        "ctu-big": ("blast", "ctu", 2, {"AA_CORRECT_ALL": "1", "AA_X3_FUSED": "1", "AA_FUSED_UPDATE": "1"}),
        "vl": ("blast", "vl", 2, {"AA_VL_PREDICT": "1"}),
        "ppm": ("blast", "ctu", 3, {}),
        "ifront": ("ifront", "ctu", 2, {"AA_ION_FUSED": "1"})}[chain]
    nx = (nx1, 11, 9)
    r = gpu_run(problem, nx, 2, strict, dict(knobs, AA_PITCH_ALIGN=0), integ, order)
    assert_same_bits(r, ref(problem, nx, 2, strict, knobs, integ, order))


# ---- 7. the read-back fallback and the unfused ion begin -----------------------------------------------------------------------
@BUILDS
@pytest.mark.parametrize("knob", ["AA_MAILBOX_SPIN_US", "AA_ION_BEGIN_FUSED"])
@pytest.mark.parametrize("deck", [("ioniz_sphere", (64, 16, 16), 12), ("blast", (24, 20, 16), 3)], ids=["sphere", "blast"])
def test_read_back_fallback_and_unfused_ion_begin(deck, knob, strict, ref):
    """AA_MAILBOX_SPIN_US=0: every scalar read-back gives up polling at once and takes the hipStreamSynchronize + stamp check
    that a read-back behind a long kernel takes at 512^3.  AA_ION_BEGIN_FUSED=0: the ion step's begin as a launch of its own.
    Same bits in both builds, and the same number of host read-backs (aa_host_syncs)."""
    problem, nx, nstep = deck
    r = gpu_run(problem, nx, nstep, strict, {knob: 0})
    b = ref(problem, nx, nstep, strict)
    assert_same_bits(r, b)
    assert r["syncs"] == b["syncs"] and r["syncs"] > 0


# ---- 8. aa_history above its grid-stride threshold -----------------------------------------------------------------------------
@BUILDS
@pytest.mark.parametrize("nx", [(64, 64, 64), (64, 64, 65), (80, 64, 56)])
def test_history_sums_on_grid_stride_grids(nx, strict):
    """k_history runs at most 1024 blocks of 256 threads: from 262 144 zones (64^3, exactly one zone per thread) on, every thread
    loops.  Against exactly rounded host sums (math.fsum) of the downloaded active zones, weighted as history.sums_from_block:
    mass, energy, kinetic energies and scalar to 1e-13; the net momenta, which cancel, to a bound from sum |M| * n * eps."""
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    run = aa.config.load(os.path.join(DECKS, "athinput.blast"), overrides(nx), "blast")
    g = lib.setup_problem(aa.config.slab(run), 0, strict)
    try:
        g.start()
        for _ in range(2):
            g.step()
        h = g.history()
        U = g.download()[4:-4, 4:-4, 4:-4, :]
    finally:
        g.close()
    dvol = run.dx[0] * run.dx[1] * run.dx[2]
    d, M = U[..., 0], [U[..., 1], U[..., 2], U[..., 3]]
    exact = [math.fsum(d.ravel()), math.fsum(U[..., 4].ravel())] + [math.fsum(m.ravel()) for m in M]
    exact += [math.fsum((0.5 * m * m * (1.0 / d)).ravel()) for m in M]
    exact += [math.fsum(U[..., 5].ravel()) if run.nscal else 0.0]
    exact = dvol * np.array(exact)
    for c in (0, 1, 5, 6, 7, 8):
        if exact[c] == 0:
            assert h[c] == 0
        else:
            assert abs(h[c] / exact[c] - 1) <= 1e-13, (c, h[c], exact[c])
    n = d.size
    for c, m in zip((2, 3, 4), M):
        bound = dvol * math.fsum(np.abs(m).ravel()) * n * np.finfo(float).eps
        assert abs(h[c] - exact[c]) <= bound, (c, h[c], exact[c], bound)


# ---- 9. host-block coherence ----------------------------------------------------------------------------------------------
def _sphere(nslab, strict):
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    run = aa.config.load(os.path.join(DECKS, "athinput.ioniz_sphere"), overrides((24, 20, 16)), "ioniz_sphere")
    with environ({"AA_SLAB_DEVICES": "0,0"}):       # (both slabs on one device, whatever the box has)
        return lib.setup_problem(aa.config.slab(run), 0, strict, nslab=nslab)


def _core(g):
    """the pinned zones of ioniz_sphere (the planet's core) as indices of the host block's zones, as setup_problem pins them"""
    import ctypes as C
    H = importlib.import_module("atmospheric-athena_amd.lib").host()
    n = H.aa_ioniz_sphere_pinned(C.byref(g.params), None, None)
    assert n > 0
    idx = np.zeros(n, dtype=np.int64); val = np.zeros((n, 6))
    H.aa_ioniz_sphere_pinned(C.byref(g.params), idx.ctypes.data_as(C.POINTER(C.c_longlong)), val.ctypes.data_as(C.POINTER(C.c_double)))
    return idx


COHERENCE_CALLS = ["apply_pinned_cells", "integrate_3d_ctu", "integrate_3d_vl", "ion_radtransfer_3d"]


@BUILDS
@pytest.mark.parametrize("nslab", [1, 2])
@pytest.mark.parametrize("call", COHERENCE_CALLS)
def test_ghost_zone_download_after_a_call_that_writes_active_zones(call, nslab, strict):
    """include/athena_amd.h: after any call that wrote active zones, aa_download_ghost_zones moves the whole block.  For each
    such call: download -> change the zones it writes in the host block -> upload -> call -> download_ghost_zones(H); H must
    then equal a full download.  aa_apply_pinned_cells on ioniz_sphere's core used to leave the caller's stale pinned zones."""
    g = _sphere(nslab, strict)
    try:
        g.start()
        H = g.download()
        if call == "apply_pinned_cells":
            H.reshape(-1, H.shape[-1])[_core(g), :5] *= 1.5
        else:
            H[4:-4, 4:-4, 4:-4, 0] *= 1.0 + 1e-3
        g.upload(H)
        getattr(g, call)()
        g.download_ghost_zones(H)
        full = g.download()
        diff = np.argwhere((H != full) & ~(np.isnan(H) & np.isnan(full)))
        assert diff.size == 0, f"{call}: {len(diff)} words of the host block differ from a full download, first (k,j,i,var) {diff[0].tolist()}"
    finally:
        g.close()


def test_ghost_zone_download_after_restrict_correct_of_the_parent_level():
    """aa_mesh_restrict_correct_pair writes the parent level's active zones: its ghost-zone download must move the whole block."""
    aa = importlib.import_module("atmospheric-athena_amd")
    lib = importlib.import_module("atmospheric-athena_amd.lib")
    gz = np.load(os.path.join(GOLD, "smr_blast_3lev_s6.npz"))
    par = aa.athinput.ParTable.from_file(orc.deck_for("blast", gz)).cmdline([str(o) for o in gz["overrides"]])
    m = lib.Mesh(aa.config.levels(par, aa.config.from_par(par, "blast")), 0, True)
    try:
        m.start()
        m.step()
        P = m.lev[0]
        H = P.download()
        H[4:-4, 4:-4, 4:-4, 0] *= 1.0 + 1e-3
        P.upload(H)
        m.restrict_correct_pair(0)
        P.download_ghost_zones(H)
        assert np.array_equal(H, P.download())
    finally:
        m.close()
