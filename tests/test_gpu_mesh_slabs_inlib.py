"""Static mesh refinement on in-library slabs: ONE process, every level cut at the same root x3 planes, one slab stack per
device (aa_create_cut + aa_mesh_create on composite handles; csrc/slabs.hip, csrc/smr.hip, csrc/mesh_cuts.h), rehearsed with
every slab on cuda:0.  lib.Mesh(levels, nslab=N, cuts=...) against lib.Mesh(levels) after start() and a few steps.

Strict build: every level's whole block (active zones and the ghost zones of the Grid's own boundaries), EdgeFlux, time, dt and
the sub-cycle counts per level and step bit for bit -- the operands of every zone are the same and the reductions are MIN / MAX /
integer sums.  Default build: equal sub-cycle counts; U, dt and EdgeFlux within the bars test_gpu_slabs_inlib.py uses for N
slabs against one (1e-13 of a field's maximum, 1e-8 for ioniz_sphere: the peeled first iteration of a marching chunk contracts
differently, and where chunks start depends on the slab).  History sums: 1e-13 (1e-8 for ioniz_sphere in the default build) of
the sum of the absolute values of a column's terms, because the summation order differs -- for the columns of one sign (mass,
energies, scalar) that is rtol 1e-13 of the sum itself; the net momenta of these symmetric problems cancel to ~1e-17 of their
terms (ioniz_sphere: x3 momentum 7.0 against 192 between the two summation orders, terms of 1e13), where a bar relative to the
net sum would measure nothing."""
import ctypes as C
import functools
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
DECKS = os.path.join(ROOT, "atmospheric-athena_amd", "decks")
GOLD = os.path.join(HERE, "golden")


def dom(n, nx, disp=None):
    o = [f"domain{n}/Nx{d + 1}={nx[d]}" for d in range(3)]
    if disp:
        o += [f"domain{n}/{k}Disp={disp[d]}" for d, k in enumerate("ijk")]
    return o


# (problem, overrides, cuts, steps, slabs): the list of test_gpu_smr_slabs.py, whose cuts are known to satisfy mesh_slabs, and 7
CASES = {
    1: ("blast", ["job/num_domains=3"] + dom(1, (16, 24, 16)) + dom(2, (12, 16, 20), (8, 20, 6)) + dom(3, (12, 8, 16), (20, 48, 16)), None, 4, 2),
    2: ("blast", ["job/num_domains=2"] + dom(1, (12, 12, 16)) + dom(2, (12, 12, 16), (6, 6, 8)), (0, 4, 16), 3, 2),
    3: ("ifront", ["job/num_domains=2"] + dom(1, (16, 8, 16)) + dom(2, (16, 8, 16), (8, 4, 8)), None, 3, 2),
    4: ("ioniz_sphere", ["job/num_domains=2"] + dom(1, (32, 32, 32)) + dom(2, (32, 28, 24), (16, 18, 20)) + ["problem/rp=2.1e10"], None, 3, 2),
    5: ("ifront", ["job/num_domains=2"] + dom(1, (64, 8, 16)) + dom(2, (64, 8, 16), (32, 4, 8)), None, 3, 2),
    6: ("ifront", ["job/num_domains=2"] + dom(1, (64, 8, 24)) + dom(2, (64, 8, 8), (32, 4, 4)), (0, 12, 24), 3, 2),
    7: ("blast", ["job/num_domains=2"] + dom(1, (16, 16, 24)) + dom(2, (16, 16, 24), (8, 8, 12)), (0, 8, 16, 24), 3, 3),
}


def pkg(name=None):
    return importlib.import_module("atmospheric-athena_amd" + ("." + name if name else ""))


def levels_of(case, integrator="ctu", order=2):
    problem, ov, _cuts, _n, _ns = CASES[case]
    aa = pkg()
    par = aa.athinput.ParTable.from_file(os.path.join(DECKS, "athinput." + problem)).cmdline(ov)
    run = aa.config.from_par(par, problem)
    run.integrator, run.order = integrator, order
    return par, run, aa.config.levels(par, run)


def run_mesh(case, strict, cut, integrator="ctu", order=2):
    problem, _ov, cuts, nsteps, nslab = CASES[case]
    _par, run, levels = levels_of(case, integrator, order)
    m = pkg("lib").Mesh(levels, 0, strict, **(dict(nslab=nslab, cuts=cuts) if cut else {}))
    try:
        m.start()
        trace = [(m.time, m.dt)]
        its = []
        for _ in range(nsteps):
            its.append(m.step()); trace.append((m.time, m.dt))
        hscale = []
        for l, g in enumerate(m.lev):       # the sum of the absolute values of every history column's terms
            h = np.abs(g.history())
            dvol = float(np.prod(run.dx)) / 8.0 ** l
            h[2:5] = np.nansum(np.abs(g.download()[4:-4, 4:-4, 4:-4, 1:4]), axis=(0, 1, 2)) * dvol
            hscale.append(h)
        out = {"U": [g.download() for g in m.lev], "its": its, "trace": trace, "hist": [g.history() for g in m.lev], "hscale": hscale,
               "ef": [g.download_edgeflux() for g in m.lev] if run.ion else None, "counts": m.halo_counts(), "cuts": m.cuts}
    finally:
        m.close()
    return out


@functools.lru_cache(maxsize=None)
def one_mesh(case, strict, integrator="ctu", order=2):
    """the undivided Mesh: computed once per case and build, shared by the tests below"""
    return run_mesh(case, strict, False, integrator, order)


def same(many, one, case, strict):
    problem = CASES[case][0]
    assert many["its"] == one["its"], "radiation sub-cycle counts per level and step"
    if problem == "ioniz_sphere":
        assert min(min(it) for it in one["its"]) > 1, "both levels must sub-cycle more than once"
    tol = 1e-8 if problem == "ioniz_sphere" else 1e-13
    worst = {"U": 0.0, "ef": 0.0, "dt": 0.0, "hist": 0.0}
    for (t1, d1), (t2, d2) in zip(one["trace"], many["trace"]):
        worst["dt"] = max(worst["dt"], abs(d2 / d1 - 1), abs(t2 - t1) / max(abs(t1), 1e-300) if t1 else abs(t2))
    for l, (a, b) in enumerate(zip(many["U"], one["U"])):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        scale = np.nanmax(np.abs(b), axis=(0, 1, 2)); scale[scale == 0] = 1
        worst["U"] = max(worst["U"], float(np.nanmax(np.nanmax(np.abs(a - b), axis=(0, 1, 2)) / scale)))
        if one["ef"] is not None:
            e = np.abs(many["ef"][l] - one["ef"][l]).max() / max(np.abs(one["ef"][l]).max(), 1e-300)
            worst["ef"] = max(worst["ef"], float(e))
        h1, h2, hs = one["hist"][l], many["hist"][l], one["hscale"][l]
        nz = hs != 0
        if nz.any():
            worst["hist"] = max(worst["hist"], float(np.nanmax(np.abs(h2[nz] - h1[nz]) / hs[nz])))
    print(f"case {case} strict={strict} cuts={many['cuts']}: max differences {worst}")
    if strict:
        assert many["trace"] == one["trace"], "time and dt of every step"
        for l, (a, b) in enumerate(zip(many["U"], one["U"])):
            assert np.array_equal(a, b, equal_nan=True), f"level {l}: {np.nanmax(np.abs(a - b), axis=(0, 1, 2))}"
        if one["ef"] is not None:
            for l in range(len(one["ef"])):
                assert np.array_equal(many["ef"][l], one["ef"][l]), f"EdgeFlux of level {l}"
    else:
        assert worst["dt"] < tol and worst["U"] < tol
        if one["ef"] is not None:
            for l in range(len(one["ef"])):
                assert np.allclose(many["ef"][l], one["ef"][l], rtol=1e-12 if tol < 1e-12 else tol, atol=1e-12 * np.abs(one["ef"][l]).max())
    assert worst["hist"] < (1e-13 if strict or problem != "ioniz_sphere" else 1e-8)
    for l in range(len(one["hist"])):
        assert np.array_equal(np.isnan(many["hist"][l]), np.isnan(one["hist"][l]))


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("strict", [True, False])
def test_cut_mesh_equals_one_mesh(case, strict):
    same(run_mesh(case, strict, True), one_mesh(case, strict), case, strict)


@pytest.mark.parametrize("integrator,order", [("vl", 2), ("ctu", 3)])
@pytest.mark.parametrize("strict", [True, False])
def test_level_that_starts_on_a_cut_with_van_leer_and_third_order(integrator, order, strict):
    same(run_mesh(2, strict, True, integrator, order), one_mesh(2, strict, integrator, order), 2, strict)


@pytest.mark.parametrize("case,env", [(2, "AA_SLAB_NO_PEER"), (5, "AA_SLAB_NO_PEER"), (5, "AA_SLAB_WORDS_STAGED")])
def test_staged_routes_leave_the_same_results(case, env, monkeypatch, capfd):
    """where peer access is refused (forced here) the halo of every level, the all-level exchange and the flux correction across
    a cut travel through pinned host memory, and so do the sub-cycle's words: the library says so, the bits are the same"""
    one = one_mesh(case, True)
    capfd.readouterr()
    monkeypatch.setenv(env, "1")
    many = run_mesh(case, True, True)
    err = capfd.readouterr().err
    if env == "AA_SLAB_NO_PEER":
        assert "the x3 halo of the slabs travels through pinned host memory" in err
    else:
        assert "reduction words of the slabs travel through pinned host memory" in err and "x3 halo" not in err
    same(many, one, case, True)


@pytest.mark.parametrize("case", [1, 4])
@pytest.mark.parametrize("strict", [True, False])
def test_per_level_and_batched_exchange_leave_the_same_bits(case, strict, monkeypatch):
    """the all-level exchange (one pack launch per slab, one copy per neighbour, one unpack launch per slab) against one exchange
    per level through the levels' own kernels (AA_MESH_HALO_BATCH=0): the same copies of the same doubles, in both builds"""
    nsteps, nslab = CASES[case][3], CASES[case][4]
    batched = run_mesh(case, strict, True)
    monkeypatch.setenv("AA_MESH_HALO_BATCH", "0")
    per_level = run_mesh(case, strict, True)
    assert per_level["counts"] == (0, 0, 0)
    exchanges = 1 + nsteps * (2 if CASES[case][0] != "blast" else 1)      # start, the end of every step, behind every radiation step
    launches, copies, n = batched["counts"]
    assert n == exchanges and launches == 2 * nslab * exchanges and nslab <= copies // exchanges <= 2 * nslab
    assert batched["its"] == per_level["its"] and batched["trace"] == per_level["trace"]
    for a, b in zip(batched["U"], per_level["U"]):
        assert np.array_equal(a, b, equal_nan=True)
    if batched["ef"] is not None:
        for a, b in zip(batched["ef"], per_level["ef"]):
            assert np.array_equal(a, b)


def test_one_read_back_per_root_sub_cycle():
    """the assertion test_gpu_slabs_inlib.py makes for a single-level composite, on the root of a cut Mesh"""
    _par, _run, levels = levels_of(5)
    m = pkg("lib").Mesh(levels, 0, True, nslab=2)
    try:
        m.start(); m.step()
        n = m.lev[0].host_syncs()
        its = m.ion_radtransfer_3d(0)
        assert its >= 1 and m.lev[0].host_syncs() - n == its
    finally:
        m.close()


def _mesh_create(L, grids, levels):
    n = len(grids)
    hs = (C.c_void_p * n)(*[g._h for g in grids])
    disp = (C.c_int * (3 * n))(*[g.disp[d] if g.level else 0 for g in levels for d in range(3)])
    h = C.c_void_p()
    rc = L.aa_mesh_create(n, hs, disp, C.byref(h))
    return rc, h, L.aa_last_error().decode()


def test_refusals_by_name():
    import torch
    lib = pkg("lib")
    _par, _run, levels = levels_of(2)
    dev = torch.cuda.current_device()

    def usable(grids):
        assert torch.cuda.current_device() == dev
        for g in grids:
            assert np.isfinite(g.download()).all()
            g.close()
        assert torch.cuda.current_device() == dev

    # mixed plain / composite levels
    grids = [lib.setup_problem(levels[0], 0, True, cuts=(0, 8, 16)), lib.setup_problem(levels[1], 0, True)]
    rc, _h, msg = _mesh_create(grids[0].L, grids, levels)
    assert rc != 0 and "levels[1] is a plain Grid but levels[0] is cut into slabs" in msg
    usable(grids)
    # different cuts
    grids = [lib.setup_problem(levels[0], 0, True, cuts=(0, 8, 16)), lib.setup_problem(levels[1], 0, True, cuts=(0, 4, 16))]
    rc, _h, msg = _mesh_create(grids[0].L, grids, levels)
    assert rc != 0 and "different cuts" in msg
    usable(grids)
    # a root cut by plain aa_create is not a level of a cut Mesh, and plain aa_create keeps refusing a refined level
    grids = [lib.setup_problem(levels[0], 0, True, nslab=2)]
    with pytest.raises(lib.AthenaError, match="only the root level can be cut into slabs.*aa_create_cut"):
        lib.setup_problem(levels[1], 0, True, nslab=2)
    usable(grids)
    # a piece thinner than nghost: level 1 lies over root planes 4 .. 12, the cut at 5 leaves it 2 planes on slab 0
    with pytest.raises(lib.AthenaError, match="level 1 on slab 0 is 2 planes thin.*plane 5"):
        lib.Mesh(levels, 0, True, cuts=(0, 5, 16))
    assert torch.cuda.current_device() == dev
    # two Domains on a level (the overrides of tests/golden/smr_blast_2dom_s6)
    aa = pkg()
    ov = [str(o) for o in np.load(os.path.join(GOLD, "smr_blast_2dom_s6.npz"))["overrides"]]
    par = aa.athinput.ParTable.from_file(os.path.join(DECKS, "athinput.blast")).cmdline(ov)
    with pytest.raises(lib.AthenaError, match="several Domains on a level"):
        lib.Mesh(aa.config.levels(par, aa.config.from_par(par, "blast")), 0, True, cuts=(0, 7, 16))
    assert torch.cuda.current_device() == dev
    # aa_mesh_set_stream, as aa_set_stream on a composite; the Mesh goes on working
    m = lib.Mesh(levels, 0, True, cuts=(0, 4, 16))
    try:
        m.start()
        with pytest.raises(lib.AthenaError, match="slabs' own streams"):
            m.set_stream(0)
        m.step()
        assert m.nstep == 1 and torch.cuda.current_device() == dev
        assert all(np.isfinite(g.download()).all() for g in m.lev)
    finally:
        m.close()
    assert torch.cuda.current_device() == dev


def _hst_rows(path):
    return np.loadtxt(path, comments="#", ndmin=2)


def test_meshrun_outputs_and_resume_on_two_slabs(tmp_path):
    """MeshRun with nslab = 2 on case 1 with hst + vtk prim + bin + rst blocks: the vtk / bin / rst files byte for byte those of
    nslab = 1 (strict build), the hst rows within the history bar; MeshRun.from_restart(<a file of the nslab = 1 run>, nslab = 2)
    continued to the same step equals the uninterrupted nslab = 1 run bit for bit."""
    import meshfix
    from restartfix import tree
    D = pkg("driver"); O = pkg("outputs"); cfg = pkg("config")
    problem, ov, _cuts, nsteps, _ns = CASES[1]
    blocks = {"1": {"out_fmt": "hst", "dt": "1e-9"}, "2": {"out_fmt": "vtk", "out": "prim", "dt": "1e-9"},
              "3": {"out_fmt": "bin", "dt": "1e-9"}, "4": {"out_fmt": "rst", "dt": "1e-9"}}
    final = {}
    for nslab in (1, 2):
        par = meshfix.deck_par(problem, list(ov) + [f"time/nlim={nsteps}"], blocks)      # (a run advances the table's output numbers)
        run = cfg.from_par(par, problem)
        rundir = str(tmp_path / f"n{nslab}")
        m = D.MeshRun(cfg.levels(par, run), run, nslab=nslab, strict=True)
        try:
            m.main(O.OutputSet.from_par(par, 0.0, rundir))
            assert m.nstep == nsteps
            final[nslab] = [g.download() for g in m.mesh.lev]
        finally:
            m.mesh.close()
    one, two = str(tmp_path / "n1"), str(tmp_path / "n2")
    files = sorted(tree(one))
    assert files == sorted(tree(two))
    kinds = {e: [p for p in files if p.endswith("." + e)] for e in ("vtk", "bin", "rst", "hst")}
    assert len(kinds["vtk"]) >= 3 * (nsteps + 1) and len(kinds["bin"]) == len(kinds["vtk"]) and len(kinds["rst"]) >= nsteps + 1 and len(kinds["hst"]) == 3
    for p in kinds["vtk"] + kinds["bin"] + kinds["rst"]:
        assert open(os.path.join(one, p), "rb").read() == open(os.path.join(two, p), "rb").read(), p
    for p in kinds["hst"]:
        a, b = _hst_rows(os.path.join(one, p)), _hst_rows(os.path.join(two, p))
        assert a.shape == b.shape and a.shape[0] >= nsteps and np.allclose(b, a, rtol=1e-13, atol=1e-13 * np.abs(a).max())
    for l in range(3):
        assert np.array_equal(final[2][l], final[1][l])
    # resumed on two slabs from the second restart file of the one-slab run
    seed = os.path.join(one, kinds["rst"][2])
    r = D.MeshRun.from_restart(seed, [f"time/nlim={nsteps}"], problem, strict=True, nslab=2)
    try:
        assert r.restarted and 0 < r.nstep < nsteps and r.mesh.nslab == 2
        r.main(O.OutputSet.from_par(r.par, r.time, str(tmp_path / "resumed")))
        assert r.nstep == nsteps
        for l, g in enumerate(r.mesh.lev):
            assert np.array_equal(g.download()[4:-4, 4:-4, 4:-4], final[1][l][4:-4, 4:-4, 4:-4]), f"level {l}"
    finally:
        r.mesh.close()


# ---- the reference's own --enable-smr main() on the shim with AA_NGPU=2 ------------------------------------------------------------
def _dropin(exe, problem, over, nlim, nxs, ion, env=None, expect_failure=False):
    import shutil
    import subprocess
    import tempfile
    from make_golden import read_rst_levels
    from test_gpu_dropin import REFBIN
    tmp = tempfile.mkdtemp(prefix="dropin_cut_")
    try:
        deck = os.path.join(tmp, "athinput")
        text = open(os.path.join(DECKS, "athinput." + problem)).read()
        text = text.replace("maxout      = 0", "maxout      = 1") + "\n<output1>\nout_fmt = rst\ndt = 1e300\n"
        open(deck, "w").write(text)
        envp = dict(os.environ); envp.update(env or {})
        pr = subprocess.run([os.path.join(REFBIN, exe), "-i", deck, "-d", os.path.join(tmp, "run"), f"time/nlim={nlim}"] + over,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=tmp, env=envp, timeout=600)
        if expect_failure:
            return pr.returncode, pr.stdout + pr.stderr
        assert pr.returncode == 0, pr.stdout[-1500:] + pr.stderr[-1500:]
        rsts = sorted(f for f in os.listdir(os.path.join(tmp, "run")) if f.endswith(".rst"))
        return (read_rst_levels(os.path.join(tmp, "run", rsts[0]), nxs, 1 if ion else 0, ion),
                read_rst_levels(os.path.join(tmp, "run", rsts[-1]), nxs, 1 if ion else 0, ion), pr.stderr)
    finally:
        shutil.rmtree(tmp)


def _need_dropin(exe):
    """the executables under oracle/_ref are build products (make -C oracle ref links the reference's own objects on
    host/athena_shim.c); skipped as the existing drop-in tests are when they are missing -- or were linked from a shim that
    does not create cut levels yet (it would run AA_NGPU on one device and say nothing about this one)"""
    from test_gpu_dropin import REFBIN
    path = os.path.join(REFBIN, exe)
    if not os.path.exists(path):
        pytest.skip("oracle/_ref SMR drop-in executables not built (make -C oracle ref)")
    if b"aa_create_cut" not in open(path, "rb").read():
        pytest.skip(f"oracle/_ref/{exe} was linked from an older host/athena_shim.c (no aa_create_cut in it): make -C oracle ref")


def _fixture(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    over = [str(o) for o in g["overrides"]]
    nlev = int(g["nlevels"])
    nxs = [tuple(int(next(o for o in over if o.startswith(f"domain{n}/Nx{d}=")).split("=")[1]) for d in (1, 2, 3)) for n in range(1, nlev + 1)]
    return over, int(g["nstep"]), nlev, nxs


@pytest.mark.parametrize("fixture,cfg", [("smr_blast_3lev_s6", "blast_smr"), ("smr_blast_3lev_edge_s8", "blast_smr"),
                                         ("smr_ioniz_sphere_2lev_s4", "ioniz_sphere_smr")])
def test_reference_smr_driver_with_two_slabs(fixture, cfg):
    """`AA_NGPU=2 athena_<cfg>_amd`: the shim creates every Domain's Grid through aa_create_cut (the root's equal division: pieces
    of 10 + 10 / 16 and 12 + 12 planes on the refined levels of these fixtures).  Against the all-CPU reference executable the
    initial dump is equal on every level and the last one within the 1e-8 of test_reference_smr_driver_on_gpu_library; against
    the same executable without AA_NGPU 1e-13 (blast) / 1e-8 (ioniz_sphere) of a field's maximum, dt likewise."""
    _need_dropin(f"athena_{cfg}_amd")
    over, nlim, nlev, nxs = _fixture(fixture)
    problem = "blast" if "blast" in cfg else "ioniz_sphere"
    ion = problem != "blast"
    nv = 6 if ion else 5
    ref0, ref, _ = _dropin(f"athena_{cfg}", problem, over, nlim, nxs, ion)
    one0, one, err1 = _dropin(f"athena_{cfg}_amd", problem, over, nlim, nxs, ion)
    two0, two, err2 = _dropin(f"athena_{cfg}_amd", problem, over, nlim, nxs, ion, {"AA_NGPU": "2"})
    assert "(level 1) on HIP device" in err1 and "in 2 slabs" not in err1
    assert "(level 1) in 2 slabs along x3" in err2 and "(level 0) in 2 slabs along x3" in err2
    assert two["nstep"] == one["nstep"] == ref["nstep"] == nlim
    assert abs(two["time"] / ref["time"] - 1) < 1e-9 and abs(two["dt"] / ref["dt"] - 1) < 1e-9
    tol = 1e-8 if ion else 1e-13
    assert abs(two["dt"] / one["dt"] - 1) < tol
    for l in range(nlev):
        assert np.array_equal(two0["levels"][l][0][..., :nv], ref0["levels"][l][0][..., :nv]), f"initial dump, level {l}"
        for other, bar in ((ref, 1e-8), (one, tol)):
            a, b = two["levels"][l][0][..., :nv], other["levels"][l][0][..., :nv]
            scale = np.abs(b).max(axis=(0, 1, 2)); scale[scale == 0] = 1
            e = (np.abs(a - b).max(axis=(0, 1, 2)) / scale).max()
            print(f"{fixture} level {l}: {e:.3e} (bar {bar})")
            assert e < bar, (l, e, bar)


def test_reference_smr_driver_refuses_two_domains_on_a_level_with_two_slabs():
    _need_dropin("athena_blast_smr_amd")
    over, nlim, _nlev, nxs = _fixture("smr_blast_2dom_s6")
    rc, text = _dropin("athena_blast_smr_amd", "blast", over, nlim, nxs, False, {"AA_NGPU": "2", "AA_SLAB_CUTS": "0,7,16"}, expect_failure=True)
    assert rc != 0 and "several Domains on a level" in text
