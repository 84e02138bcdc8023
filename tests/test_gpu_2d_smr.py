"""Static mesh refinement on 2-D Grids (Nx3 = 1) on the GPU: aa_mesh_create_2d and the k2d_* coupling kernels of csrc/smr.hip, the
flux-keeping instantiation of k2d_step (csrc/hydro2d_kernels.hip), against tests/golden/g2dsmr_*.npz -- runs of the reference's
own SMR builds (CTU + H-correction at cour_no 0.8, van Leer at 0.4) on its 2-D blast deck (tests/golden/make_golden_2d_smr.py).

Restriction, flux correction and prolongation are sums and products in the reference's order, so the strict build must agree BIT
FOR BIT on every level; the default build is held to the bars of a stand-alone 2-D Grid (tests/test_gpu_2d.py): 1e-11 of each
field's maximum, 1e-12 in dt."""
import math
import os

import numpy as np
import pytest

import twodfix
from twodfix import DECKS, GOLDEN, NG, pkg

pytestmark = pytest.mark.gpu

DECK = os.path.join(DECKS, "athinput.blast2d_smr")
CASES = [("A", 8), ("A", 1), ("B", 8), ("C", 6), ("D", 8), ("E", 6)]
PERIODIC = [("A", 8), ("C", 6), ("D", 8), ("E", 6)]
TOL_U, TOL_DT = 1e-11, 1e-12          # the project's bars for 2-D Grids in the default build


def fixture(case, integ, n):
    return twodfix.fixture(f"g2dsmr_{case}_{integ}_s{n}")


def make_mesh(fx, strict, integ=None, extra=()):
    aa, cfg, lib = pkg(), pkg("config"), pkg("lib")
    ov = [str(o) for o in fx["overrides"]] + list(extra)
    par = aa.athinput.ParTable.from_file(DECK).cmdline(ov)
    run = cfg.load(DECK, ov, "blast", integ or str(fx["integrator"]))
    return lib.Mesh(cfg.levels_2d(par, run), 0, strict)


_runs = {}


def run_case(case, integ, n, strict, fresh=False):
    """start + n steps of a fixture's Mesh -> the whole blocks of every level at step 0 and after the steps, time, dt, dt0; run once
    per process and shared (nobody writes into the arrays)"""
    key = (case, integ, n, strict)
    if fresh or key not in _runs:
        fx = fixture(case, integ, n)
        m = make_mesh(fx, strict)
        try:
            m.start()
            first = [g.download() for g in m.lev]
            dt0 = m.dt
            for _ in range(n):
                m.step()
            out = dict(first=first, last=[g.download() for g in m.lev], time=m.time, dt=m.dt, dt0=dt0, nstep=m.nstep)
        finally:
            m.close()
        for a in out["first"] + out["last"]:
            a.setflags(write=False)
        if fresh:
            return out
        _runs[key] = out
    return _runs[key]


def active(U):
    return U[:, NG:-NG, NG:-NG, :]


def relerr(a, b):
    out = []
    for c in range(a.shape[-1]):
        scale = np.abs(b[..., c]).max()
        out.append(float(np.abs(a[..., c] - b[..., c]).max()) if scale == 0 else float(np.abs(a[..., c] - b[..., c]).max() / scale))
    return out


# ---- 1. the cases of the fixtures, both integrators, both builds ---------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("integ", ["ctu", "vl"])
@pytest.mark.parametrize("case,n", CASES, ids=[f"{c}{n}" for c, n in CASES])
def test_levels_vs_reference(case, n, integ, strict):
    """Every level is filled by our problem generator; after aa_mesh_start it holds the reference's step-0 state bit for bit in
    both builds (the generator is host code, restriction is (a + b) + (c + d) times 0.25: nothing to contract) -- that isolates
    restriction.  After the steps: strict bit for bit with time and dt; default within the 2-D bars.  A1 is one step: one flux
    correction."""
    fx = fixture(case, integ, n)
    r = run_case(case, integ, n, strict)
    assert r["nstep"] == int(fx["nstep"]) and len(r["last"]) == int(fx["nlevels"])
    for l in range(int(fx["nlevels"])):
        assert np.array_equal(active(r["first"][l]), fx[f"U0_{l}"]), f"step 0, level {l}: {relerr(active(r['first'][l]), fx[f'U0_{l}'])}"
    err = [relerr(active(U), fx[f"U_{l}"]) for l, U in enumerate(r["last"])]
    e_dt0, e_dt, e_t = abs(r["dt0"] / float(fx["dt0"]) - 1), abs(r["dt"] / float(fx["dt"]) - 1), abs(r["time"] / float(fx["time"]) - 1)
    print(f"{case}{n} {integ} {'strict' if strict else 'default'}: max error / field maximum per level {[max(e) for e in err]}, "
          f"dt0 {e_dt0:.2e} dt {e_dt:.2e} time {e_t:.2e}")
    if strict:
        assert r["dt0"] == float(fx["dt0"]) and r["time"] == float(fx["time"]) and r["dt"] == float(fx["dt"])
        for l, U in enumerate(r["last"]):
            assert np.array_equal(active(U), fx[f"U_{l}"]), f"level {l}: {err[l]}"
    else:
        assert e_dt0 < TOL_DT and e_dt < TOL_DT and e_t < TOL_DT
        for l in range(len(err)):
            assert max(err[l]) < TOL_U, f"level {l}: {err[l]}"


# ---- 2. prolongation alone -----------------------------------------------------------------------------------------------------
COEF = {0: (1.0, 0.3, -0.2), 1: (0.4, -0.25, 0.15), 2: (-0.3, 0.2, 0.35), 3: (0.2, 0.1, -0.3), 4: (1.5, 0.45, 0.25)}   # a + b x + c y


def linear_state(g):
    """d, M1, M2, M3 linear in x and y, and the INTERNAL energy linear -- ProCon interpolates that, not E (smr.c:3209-3241) --
    with E = e_int + |M|^2 / 2d on top.  Whole block, ghost zones included."""
    p, N = g.params, g.N
    dx = [(p.xmax[d] - p.xmin[d]) / p.rootNx[d] / 2 ** g.cfg.level for d in range(2)]
    x = p.MinX[0] + (np.arange(N[0]) - NG + 0.5) * dx[0]
    y = p.MinX[1] + (np.arange(N[1]) - NG + 0.5) * dx[1]
    X, Y = np.meshgrid(x, y)
    U = g.new_host_block()
    f = {v: a + b * X + c * Y for v, (a, b, c) in COEF.items()}
    for v in range(4):
        U[0, :, :, v] = f[v]
    U[0, :, :, 4] = f[4] + 0.5 * (f[1] ** 2 + f[2] ** 2 + f[3] ** 2) / f[0]
    return U


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_prolongation_of_a_linear_state(case, strict):
    """aa_mesh_prolongate alone on levels that hold a state linear in x and y: mcd_slope of a linear field is its slope, so every
    ghost zone of a child on a side with a fine/coarse boundary, corners included, equals the function at its centre -- d, M1, M2,
    M3 the linear one, E the linear internal energy plus the kinetic energy of the prolonged d and M -- to 1e-14 of the field's
    maximum (a handful of roundings of O(1) numbers).  Ghost zones that belong to no such side (case B: the child's x1 side on
    the root boundary, over its active rows) keep what they held."""
    fx = fixture(case, "ctu", 8)
    m = make_mesh(fx, strict)
    SENTINEL = -777.0
    try:
        want = []
        for g in m.lev:
            U = linear_state(g)
            want.append(U.copy())
            if g.cfg.level > 0:
                act = active(U).copy()
                U[...] = SENTINEL
                U[:, NG:-NG, NG:-NG, :] = act
            g.upload(U)
        m.Prolongate()
        checked = kept = 0
        for g, W in zip(m.lev[1:], want[1:]):
            U = g.download()
            N2, N1 = U.shape[1], U.shape[2]
            irefine = 2 ** g.cfg.level
            prol = [g.cfg.disp[0] != 0, (g.cfg.disp[0] + g.cfg.Nx[0]) // irefine != g.cfg.run.rootNx[0],
                    g.cfg.disp[1] != 0, (g.cfg.disp[1] + g.cfg.Nx[1]) // irefine != g.cfg.run.rootNx[1]]
            assert [b == 0 for b in g.cfg.bc[:4]] == prol
            region = np.zeros((N2, N1), dtype=bool)
            if prol[0]: region[:, :NG] = True
            if prol[1]: region[:, -NG:] = True
            if prol[2]: region[:NG, :] = True
            if prol[3]: region[-NG:, :] = True
            ghost = np.ones((N2, N1), dtype=bool); ghost[NG:-NG, NG:-NG] = False
            assert np.array_equal(active(U), active(W))
            for v in range(5):
                scale = np.abs(W[0, :, :, v]).max()
                err = np.abs(U[0, :, :, v] - W[0, :, :, v])[region].max() / scale
                assert err < 1e-14, (g.cfg.level, v, err)
            rest = ghost & ~region
            assert np.all(U[0][rest] == SENTINEL)
            checked += int(region.sum()); kept += int(rest.sum())
        assert checked > 0 and (kept > 0) == (case == "B")
    finally:
        m.close()


# ---- 3. conservation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("integ", ["ctu", "vl"])
@pytest.mark.parametrize("case,n", PERIODIC, ids=[f"{c}{n}" for c, n in PERIODIC])
def test_root_conserves(case, n, integ, strict):
    """After RestrictCorrect the root holds the composite solution: on the periodic cases the sums over its active zones of d, M1,
    M2 and E after the steps are those at step 0 to 1e-13 of sum |q| (worst-case linear accumulation of about 8 roundings per
    zone and step; the reference's own drift on these cases is below one ulp of the total).  Without the flux correction the
    drift is many orders larger."""
    r = run_case(case, integ, n, strict)
    a, b = active(r["first"][0]), active(r["last"][0])
    for v in (0, 1, 2, 4):
        s0, s1 = math.fsum(a[..., v].ravel()), math.fsum(b[..., v].ravel())
        scale = math.fsum(np.abs(a[..., v]).ravel()) or math.fsum(np.abs(b[..., v]).ravel())
        print(f"{case}{n} {integ} field {v}: drift {abs(s1 - s0):.3e} of {scale:.3e}")
        assert abs(s1 - s0) <= 1e-13 * scale, (v, s0, s1, scale)


# ---- 4., 5. the same bits twice, and with the other launch schedule -------------------------------------------------------------
def same_bits(a, b):
    assert (a["time"], a["dt"], a["dt0"]) == (b["time"], b["dt"], b["dt0"])
    for x, y in zip(a["first"] + a["last"], b["first"] + b["last"]):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("integ", ["ctu", "vl"])
def test_same_bits_twice_in_one_process(integ):
    same_bits(run_case("A", integ, 8, False), run_case("A", integ, 8, False, fresh=True))


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("case,n,integ", [("A", 8, "ctu"), ("D", 8, "ctu"), ("E", 6, "vl")])
def test_launch_schedule_changes_no_bit(case, n, integ, strict, monkeypatch):
    """AA_SMR_ONE_LAUNCH=0 (one launch per side of a flux correction / prolongation) and AA_MESH_OVERLAP=0 (the levels integrate one
    after the other on one stream): every level's whole block, ghost zones and corners included, is the default schedule's."""
    base = run_case(case, integ, n, strict)
    for knobs in (("AA_SMR_ONE_LAUNCH",), ("AA_MESH_OVERLAP",), ("AA_SMR_ONE_LAUNCH", "AA_MESH_OVERLAP")):
        for k in ("AA_SMR_ONE_LAUNCH", "AA_MESH_OVERLAP"):
            monkeypatch.delenv(k, raising=False)
        for k in knobs:
            monkeypatch.setenv(k, "0")
        same_bits(base, run_case(case, integ, n, strict, fresh=True))


# ---- 8. what aa_mesh_create_2d refuses ------------------------------------------------------------------------------------------
def test_refusals_say_why():
    import ctypes as C
    aa, cfg, lib = pkg(), pkg("config"), pkg("lib")
    fx = fixture("A", "ctu", 8)
    ov = [str(o) for o in fx["overrides"]]
    par = aa.athinput.ParTable.from_file(DECK).cmdline(ov)
    L = lib.load(False)

    def levels(integ="ctu"):
        return cfg.levels_2d(par, cfg.load(DECK, ov + (["time/cour_no=0.4"] if integ == "vl" else []), "blast", integ))

    def create(grids, disp=None, fn=None):
        """-> the error message of aa_mesh_create_2d on these Grids (None: it succeeded)"""
        hs = (C.c_void_p * len(grids))(*[g._h for g in grids])
        flat = disp if disp is not None else [g.cfg.disp[d] if g.cfg.level else 0 for g in grids for d in range(3)]
        h = C.c_void_p()
        rc = (fn or L.aa_mesh_create_2d)(len(grids), hs, (C.c_int * len(flat))(*flat), C.byref(h))
        if rc == 0:
            L.aa_mesh_destroy(h)
            return None
        assert h.value is None
        return L.aa_last_error().decode()

    gs = [lib.Grid(g, 0, False) for g in levels()]
    vl = [lib.Grid(g, 0, False) for g in levels("vl")]
    run3 = cfg.load(os.path.join(DECKS, "athinput.blast"), ["domain1/Nx1=16", "domain1/Nx2=16", "domain1/Nx3=16"], "blast")
    g3 = lib.Grid(cfg.slab(run3), 0, False)
    noh = []
    try:
        assert create(gs) is None
        msg = create([g3])
        assert "3-D" in msg and "aa_mesh_create" in msg, msg
        msg = create([gs[0], vl[1], gs[2]])
        assert "integrator" in msg, msg
        # integrator = 2: config refuses a refined deck with it, so the Grids are made by hand
        for g in levels():
            q = lib.Grid.__new__(lib.Grid)
            q.cfg, q.L, q.nvar, q._keep, q._h = g, L, 5, [], None
            q.params = lib.params_from_grid(g); q.params.integrator = 2
            h = C.c_void_p()
            assert L.aa_create(C.byref(q.params), C.byref(h)) == 0
            q._h = h; noh.append(q)
        msg = create(noh)
        assert "integrator = 2" in msg and "H-correction" in msg, msg
        disp = [g.cfg.disp[d] if g.cfg.level else 0 for g in gs for d in range(3)]
        bad = list(disp); bad[3 * 1 + 2] = 2
        msg = create(gs, bad)
        assert "kDisp" in msg, msg
        # level 2 (16 x 16 at 40, 32) moved to the lower x1 edge of level 1 (origin 16, 12 -> 32 in zones of level 2)
        bad = list(disp); bad[3 * 2] = 32
        msg = create(gs, bad)
        assert "touches its parent in x1" in msg, msg
        bad = list(disp); bad[3 * 2] = 34
        msg = create(gs, bad)
        assert "closer than nghost/2" in msg, msg
        # ... and the 3-D constructor keeps refusing 2-D Grids, the Grids stay usable afterwards
        msg = create(gs, fn=L.aa_mesh_create)
        assert "2-D" in msg, msg
        assert create(gs) is None
        with pytest.raises(lib.AthenaError, match="ion radiation"):
            m = lib.Mesh(levels(), 0, False)
            try:
                m.ionradRestrictCorrect()
            finally:
                m.close()
    finally:
        for g in gs + vl + noh + [g3]:
            g.close()


# ---- 6. MeshRun.main with <outputN> blocks -------------------------------------------------------------------------------------
def _payload(b):
    return b[b.index(b"<par_end>\n") + len(b"<par_end>\n"):]


def test_meshrun_main_writes_the_reference_s_tree(tmp_path):
    """Case A with hst + bin (cons) + vtk (prim) + rst blocks to a short tlim, by the criteria tests/test_gpu_2d.py applies to a single
    2-D Grid: vtk and bin byte for byte (headers included), rst: everything behind the parameter dump byte for byte -- all three
    levels, root first -- and every block's num / time in it, .hst of every level: the header and every column as printed except
    the net momenta, held to 1e-9 of the mass (the order in which the zones are added up)."""
    import json
    import dumpfix
    fx = twodfix.fixture("g2dsmr_out_A")
    paths = [str(p) for p in fx["paths"]]
    files = {p: fx[f"file_{i}"].tobytes() for i, p in enumerate(paths)}
    cfg, D, O, A, lib = pkg("config"), pkg("driver"), pkg("outputs"), pkg("athinput"), pkg("lib")
    blocks = json.loads(str(fx["blocks"]))
    ov = [str(o) for o in fx["overrides"]] + [f"job/maxout={max(int(n) for n in blocks)}"]
    for n, kv in blocks.items():
        ov += [f"output{n}/{k}={v}" for k, v in kv.items()]
    par = A.ParTable.from_file(DECK).cmdline(ov)
    run = cfg.load(DECK, ov, "blast", "ctu")
    m = D.MeshRun(lib.Mesh(cfg.levels_2d(par, run), 0, True), run)
    try:
        full = str(tmp_path / "full")
        m.main(O.OutputSet.from_par(par, 0.0, full))
        got = sorted(os.path.relpath(os.path.join(dp, f), full) for dp, _, fs in os.walk(full) for f in fs)
        assert got == paths, (got, paths)
        nxs = [tuple(int(v) for v in nx) for nx in fx["nxs"]]
        for rel in paths:
            ours = open(os.path.join(full, rel), "rb").read(); ref = files[rel]
            ext = rel.rsplit(".", 1)[1]
            lev = int(rel[3]) if rel.startswith("lev") else 0
            if ext in ("vtk", "bin"):
                n = {"bin": "2", "vtk": "3"}[ext]
                assert dumpfix.compare_dump(ours, ref, nxs[lev], 0, ext, blocks[n].get("out", "cons") == "prim", rel) == 0
            elif ext == "rst":
                assert _payload(ours) == _payload(ref), rel
                po = A.ParTable.from_text(ours[:ours.index(b"<par_end>")].decode())
                pr = A.ParTable.from_text(ref[:ref.index(b"<par_end>")].decode(errors="replace"))
                for n in blocks:
                    assert po.geti(f"output{n}", "num") == pr.geti(f"output{n}", "num"), (rel, n)
                    assert po.getd(f"output{n}", "time") == pr.getd(f"output{n}", "time"), (rel, n)
                assert po.getd("time", "time") == pr.getd("time", "time") and po.geti("time", "nstep") == pr.geti("time", "nstep")
            else:
                lo, lr = ours.decode().splitlines(), ref.decode().splitlines()
                assert lo[:3] == lr[:3] and len(lo) == len(lr) > 4, (rel, lo[:3], lr[:3])
                for a, b in zip(lo[3:], lr[3:]):
                    ca, cb = a.split(), b.split()
                    assert ca[:4] == cb[:4] and ca[7:] == cb[7:], (rel, a, b)
                    assert all(abs(float(x) - float(y)) <= 1e-9 * float(cb[2]) for x, y in zip(ca[4:7], cb[4:7])), (rel, a, b)
    finally:
        m.mesh.close()


# ---- 7. restart ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("integ", ["ctu", "vl"])
def test_resume_from_the_reference_s_dump(integ, strict, tmp_path):
    """MeshRun.from_restart on the reference's dump of case A after 4 steps (it picks levels_2d by the file's table) arrives where
    the reference arrives with -r at step 8: strict bit for bit, time and dt included; default within the 2-D bars."""
    D = pkg("driver")
    fx = twodfix.fixture(f"g2dsmr_restart_A_{integ}")
    seed = str(tmp_path / "seed.rst")
    with open(seed, "wb") as f:
        f.write(fx["seed"].tobytes())
    r = D.MeshRun.from_restart(seed, [], "blast", integ, strict=strict)
    try:
        assert r.restarted and r.nstep == 4 and [g.cfg.Nx for g in r.mesh.lev] == [tuple(int(v) for v in nx) for nx in fx["nxs"]]
        r.start()
        while r.nstep < int(fx["nstep"]):
            r.step()
        err = [relerr(active(g.download()), fx[f"U_{l}"]) for l, g in enumerate(r.mesh.lev)]
        print(f"resumed {integ} {'strict' if strict else 'default'}: {[max(e) for e in err]}")
        if strict:
            assert r.time == float(fx["time"]) and r.dt == float(fx["dt"])
            for l, g in enumerate(r.mesh.lev):
                assert np.array_equal(active(g.download()), fx[f"U_{l}"]), (l, err[l])
        else:
            assert abs(r.time / float(fx["time"]) - 1) < TOL_DT and abs(r.dt / float(fx["dt"]) - 1) < TOL_DT
            assert max(max(e) for e in err) < TOL_U, err
    finally:
        r.mesh.close()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("integ", ["ctu", "vl"])
def test_own_run_resumed_from_its_own_dump(integ, strict, tmp_path):
    """case A: 4 steps, a restart dump (one file, all levels, root first), resumed for 4 more: the uninterrupted run bit for bit,
    ghost zones included, in both builds"""
    cfg, D, O, A, lib = pkg("config"), pkg("driver"), pkg("outputs"), pkg("athinput"), pkg("lib")
    fx = fixture("A", integ, 8)
    ov = [str(o) for o in fx["overrides"]] + ["job/maxout=1", "output1/out_fmt=rst", "output1/dt=1e300", "time/nlim=4"]
    par = A.ParTable.from_file(DECK).cmdline(ov)
    run = cfg.load(DECK, ov, "blast", integ)
    m = D.MeshRun(lib.Mesh(cfg.levels_2d(par, run), 0, strict), run)
    try:
        m.main(O.OutputSet.from_par(par, 0.0, str(tmp_path)))
        assert m.nstep == 4
    finally:
        m.mesh.close()
    r = D.MeshRun.from_restart(str(tmp_path / "Blast.0001.rst"), ["time/nlim=8"], "blast", integ, strict=strict)
    try:
        assert r.nstep == 4
        r.start()
        while r.nstep < 8:
            r.step()
        full = run_case("A", integ, 8, strict)
        assert (r.time, r.dt) == (full["time"], full["dt"])
        for g, U in zip(r.mesh.lev, full["last"]):
            assert np.array_equal(g.download(), U)
    finally:
        r.mesh.close()


# ---- 9. the reference's deck at its own size -----------------------------------------------------------------------------------
def test_the_shipped_deck_at_full_size_vs_the_reference_executable(tmp_path):
    """decks/athinput.blast2d_smr (200 x 300, 240^2, 320^2; cour_no 0.8) for 3 steps with MeshRun against the reference's SMR
    executable run in place on the same deck: strict build, bit for bit on all three levels."""
    import subprocess
    exe = os.path.join(twodfix.ROOT, "oracle", "_ref", "athena_blast_smr")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/athena_blast_smr not built (make -C oracle -f Makefile.ref blast_smr)")
    cfg, D, A, R, lib = pkg("config"), pkg("driver"), pkg("athinput"), pkg("restart"), pkg("lib")
    rundir = str(tmp_path / "ref")
    subprocess.run([exe, "-i", DECK, "-d", rundir, "job/maxout=1", "output1/out_fmt=rst", "output1/dt=1e300", "time/nlim=3"],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=str(tmp_path), timeout=120)
    par = A.ParTable.from_file(DECK)
    run = cfg.load(DECK, [], "blast", "ctu")
    grids = cfg.levels_2d(par, run)
    nxs = [g.Nx for g in grids]
    ref = R.scan_rst(os.path.join(rundir, "Blast.0001.rst"), nxs, 0, False)
    m = D.MeshRun(lib.Mesh(grids, 0, True), run)
    try:
        m.start()
        for _ in range(3):
            m.step()
        assert (m.nstep, m.time, m.dt) == (ref["nstep"], ref["time"], ref["dt"])
        for l, g in enumerate(m.mesh.lev):
            U, _ = R.read_state(ref, l, nxs[l], 0)
            assert np.array_equal(active(g.download()), U), (l, relerr(active(g.download()), U))
    finally:
        m.mesh.close()
