"""ctypes binding of the CPU oracle (oracle/liborc.so).  TEST INFRASTRUCTURE ONLY: nothing
under atmospheric-athena_amd/ may import this module."""
from __future__ import annotations

import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
DECKS = os.path.join(ROOT, "atmospheric-athena_amd", "decks")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class OrcParams(C.Structure):
    _fields_ = [
        ("Nx", C.c_int * 3), ("rootNx", C.c_int * 3),
        ("xmin", C.c_double * 3), ("xmax", C.c_double * 3), ("MinX", C.c_double * 3),
        ("bc", C.c_int * 6), ("nscal", C.c_int), ("ion", C.c_int),
        ("gamma", C.c_double), ("cour_no", C.c_double), ("tlim", C.c_double),
        ("sigma_ph", C.c_double), ("m_H", C.c_double), ("mu", C.c_double), ("e_gamma", C.c_double),
        ("alpha_C", C.c_double), ("k_B", C.c_double), ("time_unit", C.c_double),
        ("max_de_iter", C.c_double), ("max_de_therm_iter", C.c_double), ("max_dx_iter", C.c_double),
        ("max_de_step", C.c_double), ("max_de_therm_step", C.c_double), ("max_dx_step", C.c_double),
        ("tfloor", C.c_double), ("tceil", C.c_double),
        ("maxiter", C.c_int), ("pot", C.c_int),
        ("pot_GM", C.c_double), ("pot_Rsoft", C.c_double),
        ("userwork", C.c_int),
        ("uw_K", C.c_double), ("uw_Cp", C.c_double), ("uw_rho0", C.c_double), ("uw_rreset2", C.c_double),
        ("integrator", C.c_int), ("order", C.c_int),
    ]


_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ORACLE_DIR, "liborc.so")
        src = os.path.join(ORACLE_DIR, "athena_oracle.c")
        if (not os.path.exists(so)) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["make", "-C", ORACLE_DIR, "liborc.so"], stdout=subprocess.DEVNULL)
        L = C.CDLL(so)
        P = C.c_void_p
        D = C.c_double
        dp = C.POINTER(C.c_double)
        L.orc_create.restype = P; L.orc_create.argtypes = [C.POINTER(OrcParams)]
        L.orc_destroy.argtypes = [P]
        L.orc_U.restype = dp; L.orc_U.argtypes = [P]
        L.orc_edgeflux.restype = dp; L.orc_edgeflux.argtypes = [P]
        L.orc_dims.argtypes = [P, C.POINTER(C.c_int)]
        for f in ("orc_get_time", "orc_get_dt", "orc_new_dt_local", "orc_ion_dt_hydro"):
            getattr(L, f).restype = D; getattr(L, f).argtypes = [P]
        L.orc_get_nstep.restype = C.c_int; L.orc_get_nstep.argtypes = [P]
        L.orc_set_time.argtypes = [P, D]; L.orc_set_dt.argtypes = [P, D]; L.orc_set_nstep.argtypes = [P, C.c_int]
        L.orc_problem_ifront.argtypes = [P, D, D, D]
        L.orc_problem_ioniz_sphere.argtypes = [P, D, D, D, D, D, D]
        L.orc_problem_blast.argtypes = [P, D, D, D, D, D]
        L.orc_problem_shkset1d.argtypes = [P, dp, dp, C.c_int]
        L.orc_add_radplane.argtypes = [P, C.c_int, D]
        L.orc_set_cooling.argtypes = [P, C.c_int]; L.orc_set_cooling.restype = None
        for f in ("orc_start", "orc_bvals", "orc_bvals_ionrad", "orc_new_dt", "orc_integrate",
                  "orc_userwork", "orc_ion_begin"):
            getattr(L, f).argtypes = [P]; getattr(L, f).restype = None
        L.orc_bvals_side.argtypes = [P, C.c_int, C.c_int]; L.orc_bvals_side.restype = None
        L.orc_ion_radtransfer.restype = C.c_int; L.orc_ion_radtransfer.argtypes = [P]
        L.orc_step.restype = C.c_int; L.orc_step.argtypes = [P]
        L.orc_ion_rates.argtypes = [P, dp, dp]
        L.orc_ion_update.argtypes = [P, D]
        ip = C.POINTER(C.c_int)
        L.orc_ion_zone_rates.argtypes = [P, dp, dp, dp, ip, ip]; L.orc_ion_zone_rates.restype = None
        L.orc_ion_check_range_count.restype = C.c_long; L.orc_ion_check_range_count.argtypes = [P]
        L.orc_mesh_create.restype = P; L.orc_mesh_create.argtypes = [C.c_int, C.POINTER(OrcParams), C.POINTER(C.c_int)]
        L.orc_mesh_destroy.argtypes = [P]
        L.orc_mesh_level.restype = P; L.orc_mesh_level.argtypes = [P, C.c_int]
        L.orc_mesh_start.argtypes = [P]; L.orc_mesh_start.restype = None
        L.orc_mesh_step.argtypes = [P, C.POINTER(C.c_int)]; L.orc_mesh_step.restype = None
        L.orc_mesh_time.restype = D; L.orc_mesh_time.argtypes = [P]
        L.orc_mesh_dt.restype = D; L.orc_mesh_dt.argtypes = [P]
        L.orc_mesh_nstep.restype = C.c_int; L.orc_mesh_nstep.argtypes = [P]
        L.orc_mesh_create_tree.restype = P; L.orc_mesh_create_tree.argtypes = [C.c_int, C.POINTER(OrcParams), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.orc_mesh_create_local.restype = P; L.orc_mesh_create_local.argtypes = [C.c_int, C.POINTER(OrcParams), C.POINTER(C.c_int)]
        for f in ("orc_mesh_restrict_correct", "orc_mesh_ion_restrict_correct", "orc_mesh_prolongate"):
            getattr(L, f).argtypes = [P]; getattr(L, f).restype = None
        L.orc_mesh_restrict_correct_pair.argtypes = [P, C.c_int]; L.orc_mesh_restrict_correct_pair.restype = None
        L.orc_mesh_ionflux_prolong.argtypes = [P, C.c_int]; L.orc_mesh_ionflux_prolong.restype = None
        L.orc_cfl_max_v.argtypes = [P, dp]; L.orc_cfl_max_v.restype = None
        L.orc_flux_x3_export.argtypes = [P, C.c_int, dp]; L.orc_flux_x3_export.restype = None
        L.orc_flux_x3_apply.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp]; L.orc_flux_x3_apply.restype = None
        L.orc_cons_to_prim.argtypes = [C.c_int, C.c_int, D, dp, dp]
        L.orc_cfast.argtypes = [C.c_int, C.c_int, D, dp, dp]
        L.orc_fluxes.argtypes = [C.c_int, C.c_int, D, dp, dp, dp, dp]
        L.orc_lr_states.argtypes = [C.c_int, C.c_int, D, dp, D, D, C.c_int, C.c_int, dp, dp]
        L.orc_lr_states_ppm.argtypes = [C.c_int, C.c_int, D, dp, D, D, C.c_int, C.c_int, dp, dp]
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def params_from_grid(g) -> OrcParams:
    """g: atmospheric-athena_amd.config.GridConfig"""
    r = g.run
    p = OrcParams()
    for d in range(3):
        p.Nx[d] = g.Nx[d]; p.rootNx[d] = r.rootNx[d]
        p.xmin[d] = r.xmin[d]; p.xmax[d] = r.xmax[d]; p.MinX[d] = g.MinX[d]
    for b in range(6):
        p.bc[b] = g.bc[b]
    p.nscal = r.nscal; p.ion = 1 if r.ion else 0
    p.gamma = r.gamma; p.cour_no = r.cour_no; p.tlim = r.tlim
    p.integrator = {"ctu": 0, "vl": 1, "ctu-noh": 2}[getattr(r, "integrator", "ctu")]
    p.order = getattr(r, "order", 2)
    if r.ionp:
        for k, v in r.ionp.items():
            setattr(p, k, v)
        p.maxiter = r.maxiter
    return p


class Sim:
    """One oracle Grid.  `U` is a live numpy view [N3][N2][N1][6] (d,M1,M2,M3,E,s0)."""

    def __init__(self, grid, handle=None):
        self.grid = grid
        self.L = lib()
        self.params = params_from_grid(grid)
        self.owned = handle is None        # levels of a Mesh belong to the Mesh
        self.h = self.L.orc_create(C.byref(self.params)) if handle is None else handle
        n = (C.c_int * 3)()
        self.L.orc_dims(self.h, n)
        self.N = (n[0], n[1], n[2])
        self.U = np.ctypeslib.as_array(self.L.orc_U(self.h), shape=(n[2], n[1], n[0], 6))
        nx = grid.Nx
        self.edgeflux = np.ctypeslib.as_array(self.L.orc_edgeflux(self.h),
                                              shape=(nx[2] + 1, nx[1] + 1, nx[0] + 1))

    def __del__(self):
        try:
            if self.owned:
                self.L.orc_destroy(self.h)
        except Exception:
            pass

    def problem(self):
        r = self.grid.run; pr = r.prob
        if r.problem == "ifront":
            self.L.orc_problem_ifront(self.h, pr["n_H"], pr["cs"], pr["flux"])
        elif r.problem == "ioniz_sphere":
            self.L.orc_problem_ioniz_sphere(self.h, pr["n_H"], pr["cs"], pr["flux"],
                                            pr.get("rp", 1.2e10), pr.get("mp", 1.0e30), pr.get("np", 6.0e8))
        elif r.problem == "blast":
            self.L.orc_problem_blast(self.h, pr["radius"], pr["pamb"], pr.get("damb", 1.0),
                                     pr.get("drat", 1.0), pr["prat"])
        elif r.problem == "shkset1d":
            wl = np.array([pr["dl"], pr["pl"], pr["v1l"], pr["v2l"], pr["v3l"]])
            wr = np.array([pr["dr"], pr["pr"], pr["v1r"], pr["v2r"], pr["v3r"]])
            self.L.orc_problem_shkset1d(self.h, _dp(wl), _dp(wr), int(pr["shk_dir"]))
        else:
            raise ValueError(r.problem)
        return self

    @property
    def active(self):
        g = 4
        return self.U[g:-g, g:-g, g:-g, :]

    time = property(lambda s: s.L.orc_get_time(s.h), lambda s, v: s.L.orc_set_time(s.h, v))
    dt = property(lambda s: s.L.orc_get_dt(s.h), lambda s, v: s.L.orc_set_dt(s.h, v))
    nstep = property(lambda s: s.L.orc_get_nstep(s.h), lambda s, v: s.L.orc_set_nstep(s.h, v))

    def add_radplane(self, dir, flux): self.L.orc_add_radplane(self.h, int(dir), float(flux))
    def set_cooling(self, kind=1): self.L.orc_set_cooling(self.h, int(kind))     # CoolingFunc = KoyInut (CTU only)
    def start(self): self.L.orc_start(self.h); return self
    def step(self): return self.L.orc_step(self.h)
    def bvals(self): self.L.orc_bvals(self.h)
    def bvals_side(self, d, side): self.L.orc_bvals_side(self.h, int(d), int(side))
    def bvals_ionrad(self): self.L.orc_bvals_ionrad(self.h)
    def new_dt(self): self.L.orc_new_dt(self.h)
    def new_dt_local(self): return self.L.orc_new_dt_local(self.h)
    def integrate(self): self.L.orc_integrate(self.h)
    def userwork(self): self.L.orc_userwork(self.h)
    def ion_radtransfer(self): return self.L.orc_ion_radtransfer(self.h)
    def ion_begin(self): self.L.orc_ion_begin(self.h)

    def ion_rates(self):
        a = C.c_double(); b = C.c_double()
        self.L.orc_ion_rates(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def ion_update(self, dt): self.L.orc_ion_update(self.h, dt)

    def ion_zone_rates(self):
        """-> (ph_rate, nHdot, edot, last_sign, sign_count) of the last ion_rates, copies over the active zones [k][j][i]"""
        nx = self.grid.Nx; shp = (nx[2], nx[1], nx[0])
        ph = np.zeros(shp); nHdot = np.zeros(shp); edot = np.zeros(shp)
        ls = np.zeros(shp, dtype=np.intc); sc = np.zeros(shp, dtype=np.intc)
        ip = C.POINTER(C.c_int)
        self.L.orc_ion_zone_rates(self.h, _dp(ph), _dp(nHdot), _dp(edot), ls.ctypes.data_as(ip), sc.ctypes.data_as(ip))
        return ph, nHdot, edot, ls, sc

    def cfl_max_v(self):
        v = np.zeros(3); self.L.orc_cfl_max_v(self.h, _dp(v)); return list(v)

    def flux_x3_export(self, side):
        buf = np.zeros((self.grid.Nx[1] // 2, self.grid.Nx[0] // 2, 6))
        self.L.orc_flux_x3_export(self.h, side, _dp(buf)); return buf

    def flux_x3_apply(self, side, i0, j0, n1, n2, buf):
        buf = np.ascontiguousarray(buf, dtype=np.float64)
        self.L.orc_flux_x3_apply(self.h, side, i0, j0, n1, n2, _dp(buf))

    def ion_check_range_count(self): return self.L.orc_ion_check_range_count(self.h)
    def ion_dt_hydro(self): return self.L.orc_ion_dt_hydro(self.h)


def make_sim(problem, overrides=None, rank=0, nranks=1, integrator="ctu", order=2, nscal=None):
    """nscal: the number of passive scalars where it is not the problem's own (a hydro-only NSCALARS = 1 configuration on the blast deck)"""
    aa = importlib.import_module("atmospheric-athena_amd")
    run = aa.config.load(os.path.join(DECKS, "athinput." + problem), overrides, problem)
    run.integrator = integrator
    run.order = order
    if nscal is not None:
        run.nscal = nscal
    return Sim(aa.config.slab(run, rank, nranks)).problem()


def rayplane_pattern(nx, n_H, m_H, cs, gamma):
    """Initial state of tests/fixtures/rayplane_dir.c on the active zones [k][j][i][6]: gas at rest, neutral, density by a
    fixed integer pattern of the zone indices."""
    k, j, i = np.meshgrid(np.arange(nx[2]), np.arange(nx[1]), np.arange(nx[0]), indexing="ij")
    rho = n_H * m_H * (0.02 + 0.09 * ((7 * i + 3 * j + 5 * k) % 11).astype(np.float64))
    U = np.zeros(rho.shape + (6,))
    U[..., 0] = rho; U[..., 4] = rho * cs * cs / (gamma - 1.0); U[..., 5] = rho
    return U


def make_rayplane_sim(nx, raydir):
    """The oracle set up like the reference built on tests/fixtures/rayplane_dir.c: ifront deck, the pattern state, a
    radiation plane with rays along +x1 (raydir -1) or +x2 (-2)."""
    s = make_sim("ifront", [f"domain1/Nx{d + 1}={int(nx[d])}" for d in range(3)])
    r = s.grid.run
    s.active[...] = rayplane_pattern(nx, r.prob["n_H"], r.ionp["m_H"], r.prob["cs"], r.gamma)
    s.add_radplane(raydir, r.prob["flux"])
    return s


def cool_pattern(nx, n0, T0, v0, gamma):
    """Initial state of tests/fixtures/cool_pattern.c on the active zones [k][j][i][6]: diffuse gas in cgs units, number
    density, temperature and velocity by fixed integer patterns of the zone indices (the same expressions, operation by
    operation)."""
    mbar = 1.37 * 1.6733e-24; kb = 1.380658e-16
    c, b, a = np.meshgrid(np.arange(nx[2]), np.arange(nx[1]), np.arange(nx[0]), indexing="ij")
    n = n0 * (0.5 + 0.25 * ((7 * a + 3 * b + 5 * c) % 11).astype(np.float64))
    T = T0 * (0.06 + 0.4 * ((5 * a + 7 * b + 3 * c) % 7).astype(np.float64))
    rho = n * mbar
    v1 = v0 * (((3 * a + 5 * b + 7 * c) % 5).astype(np.float64) - 2.0)
    v2 = v0 * (((a + 2 * b + 3 * c) % 7).astype(np.float64) - 3.0)
    v3 = v0 * (((2 * a + b + 4 * c) % 3).astype(np.float64) - 1.0)
    U = np.zeros(rho.shape + (6,))
    U[..., 0] = rho; U[..., 1] = rho * v1; U[..., 2] = rho * v2; U[..., 3] = rho * v3
    U[..., 4] = n * kb * T / (gamma - 1.0) + 0.5 * rho * (v1 * v1 + v2 * v2 + v3 * v3)
    return U


def coolpat_setup(g):
    """(deck overrides, n0, T0, v0, cool) of a coolpat_* golden fixture"""
    kv = dict(str(o).split("=") for o in g["overrides"])
    ov = [f"domain1/Nx{d + 1}={int(g['nx'][d])}" for d in range(3)]
    ov += [f"{k}={v}" for k, v in kv.items() if "/" in k and k != "problem/cool"]
    return ov, float(kv["n0"]), float(kv["T0"]), float(kv["v0"]), int(kv["problem/cool"])


def make_coolpat_sim(g):
    """The oracle set up like the reference built on tests/fixtures/cool_pattern.c: blast deck (hydro, no scalar), the
    pattern state, CoolingFunc = KoyInut where the fixture had it."""
    ov, n0, T0, v0, cool = coolpat_setup(g)
    s = make_sim("blast", ov)
    s.active[...] = cool_pattern(g["nx"], n0, T0, v0, s.grid.run.gamma)
    s.set_cooling(cool)
    return s


class Mesh:
    """Nested static-mesh-refinement levels (one Domain per level) on the oracle."""

    def __init__(self, grids, links=None):
        """links: config.LinkConfig list for one rank's stack of slabs; None = the whole Mesh."""
        self.L = lib()
        n = len(grids)
        pa = (OrcParams * n)(*[params_from_grid(g) for g in grids])
        if links is None:
            da = (C.c_int * (3 * n))(*[g.disp[d] if g.level else 0 for g in grids for d in range(3)])
            la = (C.c_int * n)(*[g.level for g in grids])
            self.h = self.L.orc_mesh_create_tree(n, pa, la, da)       # grids: level by level, deck order inside a level
        else:
            flat = [v for L_ in links for v in (*L_.cs, *L_.n, *L_.prol, *L_.corr, *L_.cdisp)]
            self.h = self.L.orc_mesh_create_local(n, pa, (C.c_int * max(1, len(flat)))(*flat))
        if not self.h:
            raise ValueError("orc_mesh_create failed (levels not nested?)")
        self.lev = [Sim(g, handle=self.L.orc_mesh_level(self.h, l)) for l, g in enumerate(grids)]

    def __del__(self):
        try:
            self.lev = []
            self.L.orc_mesh_destroy(self.h)
        except Exception:
            pass

    def problem(self):
        for s in self.lev:
            s.problem()
        return self

    def start(self):
        self.L.orc_mesh_start(self.h); return self

    def restrict_correct_pair(self, l): self.L.orc_mesh_restrict_correct_pair(self.h, l)
    def ion_restrict_correct(self): self.L.orc_mesh_ion_restrict_correct(self.h)
    def prolongate(self): self.L.orc_mesh_prolongate(self.h)
    def ionflux_prolong(self, l): self.L.orc_mesh_ionflux_prolong(self.h, l)

    def step(self):
        it = (C.c_int * len(self.lev))()
        self.L.orc_mesh_step(self.h, it)
        return list(it)

    time = property(lambda s: s.L.orc_mesh_time(s.h))
    dt = property(lambda s: s.L.orc_mesh_dt(s.h))
    nstep = property(lambda s: s.L.orc_mesh_nstep(s.h))


def deck_for(problem, g):
    """The deck of a golden SMR fixture: ours, with the <domainN> block the fixture carries appended (decks stop at <domain3>)."""
    import tempfile
    base = os.path.join(DECKS, "athinput." + problem)
    extra = str(g["extra_deck"]) if "extra_deck" in g.files else ""
    if not extra:
        return base
    f = tempfile.NamedTemporaryFile("w", prefix="athinput_", suffix="." + problem, delete=False)
    f.write(open(base).read() + extra); f.close()
    return f.name


def make_mesh(problem, deck_path=None, overrides=None, integrator="ctu", order=2, nscal=None):
    aa = importlib.import_module("atmospheric-athena_amd")
    par = aa.athinput.ParTable.from_file(deck_path or os.path.join(DECKS, "athinput." + problem)).cmdline(overrides)
    run = aa.config.from_par(par, problem)
    run.integrator = integrator
    run.order = order
    if nscal is not None:
        run.nscal = nscal
    return Mesh(aa.config.levels(par, run)).problem()


# ---- function-level kernels ---------------------------------------------------------
def cons_to_prim(U, gamma, nscal):
    U = np.ascontiguousarray(U, dtype=np.float64); W = np.empty_like(U)
    lib().orc_cons_to_prim(U.shape[0], nscal, gamma, _dp(U), _dp(W)); return W


def cfast(U, gamma, nscal):
    U = np.ascontiguousarray(U, dtype=np.float64); c = np.empty(U.shape[0])
    lib().orc_cfast(U.shape[0], nscal, gamma, _dp(U), _dp(c)); return c


def fluxes(Ul, Ur, eta, gamma, nscal):
    Ul = np.ascontiguousarray(Ul, dtype=np.float64); Ur = np.ascontiguousarray(Ur, dtype=np.float64)
    eta = np.ascontiguousarray(eta, dtype=np.float64); F = np.zeros_like(Ul)
    lib().orc_fluxes(Ul.shape[0], nscal, gamma, _dp(Ul), _dp(Ur), _dp(eta), _dp(F)); return F


def lr_states(W, dt, dx, il, iu, gamma, nscal, order=2):
    W = np.ascontiguousarray(W, dtype=np.float64)
    Wl = np.zeros_like(W); Wr = np.zeros_like(W)
    f = lib().orc_lr_states_ppm if order == 3 else lib().orc_lr_states
    f(W.shape[0], nscal, gamma, _dp(W), dt, dx, il, iu, _dp(Wl), _dp(Wr))
    return Wl, Wr
