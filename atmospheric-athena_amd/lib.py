"""ctypes binding of the C-ABI (include/athena_amd.h) and of the host-side C problem files.

There is no CPU fallback: if libathena_amd.so is missing or no MI355X is visible the calls
raise.  ``Grid`` mirrors the reference's per-step call sites one-to-one (bvals_mhd, new_dt,
integrate_3d_ctu, ion_radtransfer_3d; main.c:519-669) on a device-resident Grid.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .config import GridConfig, NGHOST

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class AthenaError(RuntimeError):
    """ath_error() of the reference (utils.c:118): every failure is fatal to the run."""


class aa_params(C.Structure):
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
        ("maxiter", C.c_int), ("device", C.c_int), ("integrator", C.c_int), ("level", C.c_int),
        ("order", C.c_int), ("ion_path", C.c_int), ("nslab", C.c_int),
    ]


ION_WORDS = 8     # AA_ION_WORDS of include/athena_amd.h
TEST_PICK_SCALARS = 16     # AA_TEST_PICK_SCALARS: a row of aa_test_ion_pick's `prev` / `out`
HST_ROW = 11      # AA_HST_ROW: doubles of a row of aa_run_hst_rows (time, dt, the nine sums of aa_history)

GRAVPOT = C.CFUNCTYPE(C.c_double, C.c_double, C.c_double, C.c_double)
GATHER = C.CFUNCTYPE(C.c_int, C.c_void_p)      # aa_gather_fn of include/athena_amd.h

_libs = {}
_host = None


def build(force: bool = False) -> None:
    """Compile the HIP libraries and the host C library in-tree (hipcc cross-compiles gfx950)."""
    import subprocess
    args = ["make", "-C", os.path.join(HERE, "csrc"), "-j8"] + (["-B"] if force else [])
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(HERE, "host")] + (["-B"] if force else []),
                          stdout=subprocess.DEVNULL)


def strict_default() -> bool:
    return os.environ.get("ATHENA_AMD_STRICT", "0") not in ("", "0")


def load(strict: bool | None = None) -> C.CDLL:
    strict = strict_default() if strict is None else strict
    if strict in _libs:
        return _libs[strict]
    name = "libathena_amd_strict.so" if strict else "libathena_amd.so"
    if os.environ.get("ATHENA_AMD_VARIANT") and not strict:        # A/B experiment builds (csrc/Makefile `variant`)
        name = f"libathena_amd_{os.environ['ATHENA_AMD_VARIANT']}.so"
    path = os.path.join(HERE, name)
    if not os.path.exists(path):
        raise AthenaError(f"{path} is missing: run __graft_entry__.build() (no CPU fallback exists)")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.  If this library pulled
    # in the system runtime first, a later `import torch` in the same process would find "No HIP
    # GPUs".  Loading torch first makes both share torch's runtime (same SONAME).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    P = C.c_void_p; D = C.c_double; I = C.c_int; LL = C.c_longlong
    dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int); llp = C.POINTER(C.c_longlong)
    sig = {
        "aa_create": (I, [C.POINTER(aa_params), C.POINTER(P)]),
        "aa_create_cut": (I, [C.POINTER(aa_params), I, I, ip, C.POINTER(P)]),
        "aa_mesh_nslab": (I, [P]), "aa_mesh_halo_counts": (I, [P, llp]),
        "aa_destroy": (None, [P]),
        "aa_last_error": (C.c_char_p, []),
        "aa_set_stream": (I, [P, P]),
        "aa_sync": (I, [P]),
        "aa_device_bytes": (LL, [P]),
        "aa_upload_cons": (I, [P, dp]), "aa_download_cons": (I, [P, dp]), "aa_download_ghost_zones": (I, [P, dp]),
        "aa_upload_edgeflux": (I, [P, dp]), "aa_download_edgeflux": (I, [P, dp]),
        "aa_get_mesh_state": (I, [P, dp, dp, ip]), "aa_set_mesh_state": (I, [P, D, D, I]),
        "aa_set_static_grav_pot": (I, [P, GRAVPOT]),
        "aa_set_cooling": (I, [P, I]),
        "aa_set_fofc": (I, [P, I]), "aa_get_fofc": (I, [P]), "aa_get_fofc_counts": (I, [P, llp]),
        "aa_set_static_grav_tables": (I, [P, dp, dp, dp, dp]),
        "aa_set_pinned_cells": (I, [P, LL, llp, dp]), "aa_apply_pinned_cells": (I, [P]),
        "aa_add_radplane_3d": (I, [P, I, D]), "aa_has_radplane": (I, [P]),
        "aa_bvals_mhd": (I, [P]), "aa_bvals_mhd_side": (I, [P, I, I]), "aa_bvals_ionrad": (I, [P]), "aa_new_dt": (I, [P]),
        "aa_integrate_3d_ctu": (I, [P]), "aa_integrate_begin": (I, [P]), "aa_cfl_in_update": (I, [P, I]), "aa_integrate_3d_vl": (I, [P]),
        "aa_integrate_2d_ctu": (I, [P]), "aa_integrate_2d_vl": (I, [P]), "aa_ion_radtransfer_3d": (I, [P, ip]),
        "aa_set_order_2d": (I, [P, I]), "aa_get_order_2d": (I, [P]),
        "aa_integrate_1d_ctu": (I, [P]), "aa_integrate_1d_vl": (I, [P]), "aa_run_1d": (I, [P, D, D, I, ip]),
        "aa_run_2d": (I, [P, D, D, I, ip]), "aa_run_2d_batch": (I, [P]),
        "aa_run_3d": (I, [P, D, D, I, ip]), "aa_run_3d_batch": (I, [P]),
        "aa_run_hst_arm": (I, [P, D, D, I]), "aa_run_hst_rows": (I, [P, I, dp, ip, dp]),
        "aa_mesh_run_hst_arm": (I, [P, D, D, I]), "aa_mesh_run_hst_rows": (I, [P, I, I, dp, ip, dp]),
        "aa_run_1d_cap": (I, []), "aa_step_1d_block": (I, []),
        "aa_start": (I, [P]), "aa_step": (I, [P, ip]),
        "aa_new_dt_local": (I, [P, dp]), "aa_ion_begin": (I, [P]), "aa_ion_rates": (I, [P, dp, dp]),
        "aa_ion_update": (I, [P, D, llp, dp]),
        "aa_ion_is_fused": (I, [P]), "aa_ion_speculate": (I, [P, D]), "aa_ion_pass": (I, [P, I, I, P]), "aa_ion_pick": (I, [P, P, I, I, D]),
        "aa_ion_fetch": (I, [P, dp, ip, dp, dp, llp, dp, ip]), "aa_ion_finish": (I, [P]), "aa_ion_lean_counts": (I, [P, llp]),
        "aa_set_ion_batch": (I, [P, I]), "aa_ion_batch": (I, [P]), "aa_ion_batch_active": (I, [P]), "aa_ion_batch_counts": (I, [P, llp]),
        "aa_ion_radtransfer_3d_gather": (I, [P, P, P, I, GATHER, P, ip]), "aa_host_syncs": (I, [P, I]),
        "aa_halo_doubles": (LL, [P]), "aa_pack_x3": (I, [P, I, P]), "aa_unpack_x3": (I, [P, I, P]),
        "aa_halo_doubles_x2": (LL, [P]), "aa_pack_x2": (I, [P, I, P]), "aa_unpack_x2": (I, [P, I, P]),
        "aa_halo_doubles_dir": (LL, [P, I]), "aa_halo_get": (I, [P, I, I, dp]), "aa_halo_put": (I, [P, I, I, dp]), "aa_device_count": (I, []),
        "aa_mesh_create": (I, [I, C.POINTER(P), ip, C.POINTER(P)]), "aa_mesh_destroy": (None, [P]),
        "aa_mesh_create_2d": (I, [I, C.POINTER(P), ip, C.POINTER(P)]),
        "aa_mesh_get_state": (I, [P, dp, dp, ip]), "aa_mesh_set_state": (I, [P, D, D, I]),
        "aa_mesh_set_stream": (I, [P, P]), "aa_mesh_restrict_correct_pair": (I, [P, I]),
        "aa_mesh_restrict_correct": (I, [P]), "aa_mesh_ionrad_restrict_correct": (I, [P]),
        "aa_mesh_prolongate": (I, [P]), "aa_mesh_new_dt": (I, [P]), "aa_mesh_ion_radtransfer": (I, [P, I, ip]),
        "aa_mesh_start": (I, [P]), "aa_mesh_step": (I, [P, ip]),
        "aa_mesh_run_2d": (I, [P, D, D, I, ip]), "aa_mesh_run_2d_batch": (I, [P]),
        "aa_mesh_run_3d": (I, [P, D, D, I, ip]), "aa_mesh_run_3d_batch": (I, [P]),
        "aa_mesh_ionflux_prolong": (I, [P, I]), "aa_mesh_create_local": (I, [I, C.POINTER(P), ip, C.POINTER(P)]),
        "aa_flux_x3_export": (I, [P, I, P]), "aa_flux_x3_apply": (I, [P, I, I, I, I, I, P]), "aa_cfl_max_v": (I, [P, dp]),
        "aa_test_fluxes": (I, [I, D, I, dp, dp, dp, dp]),
        "aa_test_lr_states": (I, [I, D, I, dp, D, D, I, I, dp, dp]),
        "aa_test_lr_states_ppm": (I, [I, D, I, dp, D, D, I, I, dp, dp]),
        "aa_test_explog": (I, [I, dp, dp, dp]),
        "aa_test_ion_pick": (I, [I, dp, I, D, I, dp, dp, dp]),
        "aa_test_ion_batch": (I, [I, dp, I, D, D, I, I, dp, dp]),
        "aa_test_xdiv": (I, [I, dp, dp, dp]),
        "aa_test_zone_offsets": (I, [C.c_uint, dp, dp]),
        "aa_history": (I, [P, dp]),
        "aa_dump_sections": (I, [P, I]), "aa_dump_section_floats": (LL, [P, I, I]),
        "aa_dump_section": (I, [P, I, I, I, C.POINTER(C.c_float)]),
        "aa_dump_snapshot_bytes": (LL, [P, I]), "aa_dump_snapshot_begin": (I, [P, I, I, I, LL]),
        "aa_dump_snapshot_ready": (I, [P, I]), "aa_dump_snapshot_wait": (I, [P, I]),
        "aa_dump_snapshot_section": (C.c_void_p, [P, I, I, llp]), "aa_dump_snapshot_release": (I, [P, I]),
        "aa_outdata_dims": (I, [P, I, ip, ip, ip, ip]), "aa_outdata": (I, [P, I, ip, ip, ip, dp, ip, dp, dp]),
        "aa_outdata_gray": (I, [P, I, ip, ip, ip, D, D, C.POINTER(C.c_ubyte), ip]),
        "aa_rst_sections": (I, [P]), "aa_rst_section_label": (I, [P, I, C.c_char_p, I]), "aa_rst_section_doubles": (LL, [P, I]),
        "aa_rst_section_get": (I, [P, I, dp]), "aa_rst_section_put": (I, [P, I, dp]),
        "aa_rst_section_get_box": (I, [P, I, ip, ip, dp]), "aa_rst_section_put_box": (I, [P, I, ip, ip, dp]),
        "aa_rst_snapshot_bytes": (LL, [P]), "aa_rst_snapshot_begin": (I, [P, I, LL]),
        "aa_rst_snapshot_ready": (I, [P, I]), "aa_rst_snapshot_wait": (I, [P, I]),
        "aa_rst_snapshot_section": (C.c_void_p, [P, I, I, llp]), "aa_rst_snapshot_release": (I, [P, I]),
        "aa_resume": (I, [P]), "aa_mesh_resume": (I, [P]),
        "aa_profile_enable": (I, [P, I]), "aa_profile_reset": (I, [P]), "aa_profile_count": (I, [P]),
        "aa_profile_name": (C.c_char_p, [P, I]), "aa_profile_get": (I, [P, I, dp, llp]),
    }
    variant = name not in ("libathena_amd_strict.so", "libathena_amd.so")
    for name_, (res, args) in sig.items():
        if variant and not hasattr(L, name_):
            continue                   # (an A/B build of older sources lacks what was added since)
        f = getattr(L, name_)          # AttributeError here = header and library disagree
        f.restype = res; f.argtypes = args
    L._sig = sig
    _libs[strict] = L
    return L


def host() -> C.CDLL:
    global _host
    if _host is None:
        path = os.path.join(HERE, "libathena_amd_host.so")
        if not os.path.exists(path):
            raise AthenaError(f"{path} is missing: run __graft_entry__.build()")
        H = C.CDLL(path)
        dp = C.POINTER(C.c_double); pp = C.POINTER(aa_params); D = C.c_double
        H.aa_problem_ifront.argtypes = [pp, D, D, dp]; H.aa_problem_ifront.restype = C.c_int
        H.aa_problem_ioniz_sphere.argtypes = [pp, D, D, D, D, dp]; H.aa_problem_ioniz_sphere.restype = C.c_int
        H.aa_problem_ioniz_sphere_restart.argtypes = [pp, D, D, D, D]; H.aa_problem_ioniz_sphere_restart.restype = C.c_int
        H.aa_problem_blast.argtypes = [pp, D, D, D, D, D, dp]; H.aa_problem_blast.restype = C.c_int
        H.aa_problem_shkset1d.argtypes = [pp, dp, dp, C.c_int, dp]; H.aa_problem_shkset1d.restype = C.c_int
        H.aa_planet_pot.argtypes = [D, D, D]; H.aa_planet_pot.restype = D
        H.aa_ioniz_sphere_pinned.argtypes = [pp, C.POINTER(C.c_longlong), dp]
        H.aa_ioniz_sphere_pinned.restype = C.c_longlong
        _host = H
    return _host


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def params_from_grid(g: GridConfig, device: int = 0, ion_path: int = 0, nslab: int = 1) -> aa_params:
    r = g.run
    p = aa_params()
    for d in range(3):
        p.Nx[d] = g.Nx[d]; p.rootNx[d] = r.rootNx[d]
        p.xmin[d] = r.xmin[d]; p.xmax[d] = r.xmax[d]; p.MinX[d] = g.MinX[d]
    for b in range(6):
        p.bc[b] = g.bc[b]
    p.nscal = r.nscal; p.ion = 1 if r.ion else 0
    p.gamma = r.gamma; p.cour_no = r.cour_no; p.tlim = r.tlim
    for k, v in r.ionp.items():
        setattr(p, k, v)
    p.maxiter = r.maxiter
    p.device = device
    p.integrator = {"ctu": 0, "vl": 1, "ctu-noh": 2}[r.integrator]
    p.level = g.level
    p.order = getattr(r, "order", 2)
    p.ion_path = ion_path
    p.nslab = nslab
    return p


class Snapshot:
    """One slot of a Grid's dump snapshots between aa_dump_snapshot_begin and _release (Grid.dump_snapshot makes it).  Every
    method calls HIP and belongs to the thread that drives the run; the arrays of `section` are plain page-locked host memory,
    which any thread may read until `release`."""

    def __init__(self, grid: "Grid", slot: int, fmt: int, prim: bool):
        self._g, self.slot, self.fmt, self.prim = grid, slot, fmt, prim
        self.nsections = int(grid.L.aa_dump_sections(grid._h, fmt))

    def _grid(self) -> "Grid":
        if self._g is None:
            raise AthenaError("[Snapshot]: released, or its Grid is closed")
        return self._g

    def ready(self) -> bool:
        """whether the payload is on the host: one event query, never blocks"""
        g = self._grid()
        rc = g.L.aa_dump_snapshot_ready(g._h, self.slot)
        if rc < 0:
            g._chk(rc)
        return rc == 1

    def wait(self) -> "Snapshot":
        g = self._grid(); g._chk(g.L.aa_dump_snapshot_wait(g._h, self.slot)); return self

    def section(self, i: int) -> np.ndarray:
        """section i of the payload: a view of the page-locked buffer, no copy (float32 holding the file's words, as
        Grid.dump_section returns them); valid until release"""
        g = self._grid()
        n = C.c_longlong()
        p = g.L.aa_dump_snapshot_section(g._h, self.slot, int(i), C.byref(n))
        if not p:
            raise AthenaError(g.L.aa_last_error().decode() or "[aa_dump_snapshot_section]")
        a = np.ctypeslib.as_array((C.c_float * n.value).from_address(p))
        a.flags.writeable = False
        return a

    def sections(self) -> list:
        return [self.section(i) for i in range(self.nsections)]

    def release(self) -> None:
        """frees the slot (waits first if the copy is still in flight); the arrays of `section` are dead afterwards"""
        g, self._g = self._g, None
        if g is not None and g._h is not None:
            g._snaps[self.slot] = None
            g._chk(g.L.aa_dump_snapshot_release(g._h, self.slot))


class RstSnapshot:
    """The slot of a Grid's restart snapshot between aa_rst_snapshot_begin and _release (Grid.rst_snapshot makes it): the
    double-precision payload of a restart dump.  The threading rule is Snapshot's: every method from the thread that drives the
    run; the arrays of `sections` are plain page-locked host memory, which any thread may read until `release`."""

    RST_SLOTS = 1                        # AA_RST_SLOTS

    def __init__(self, grid: "Grid", slot: int):
        self._g, self.slot = grid, slot
        self.labels = [label for label, _ in grid.rst_sections()]
        self.nsections = len(self.labels)

    def _grid(self) -> "Grid":
        if self._g is None:
            raise AthenaError("[RstSnapshot]: released, or its Grid is closed")
        return self._g

    def ready(self) -> bool:
        """whether the payload is on the host: one event query, never blocks"""
        g = self._grid()
        rc = g.L.aa_rst_snapshot_ready(g._h, self.slot)
        if rc < 0:
            g._chk(rc)
        return rc == 1

    def wait(self) -> "RstSnapshot":
        g = self._grid(); g._chk(g.L.aa_rst_snapshot_wait(g._h, self.slot)); return self

    def section(self, i: int) -> np.ndarray:
        """section i of the payload: a float64 view of the page-locked buffer, no copy (what Grid.rst_section returns, bit for
        bit); valid until release"""
        g = self._grid()
        n = C.c_longlong()
        p = g.L.aa_rst_snapshot_section(g._h, self.slot, int(i), C.byref(n))
        if not p:
            raise AthenaError(g.L.aa_last_error().decode() or "[aa_rst_snapshot_section]")
        a = np.ctypeslib.as_array((C.c_double * n.value).from_address(p))
        a.flags.writeable = False
        return a

    def sections(self) -> list:
        """[(label, float64 array over the page-locked buffer)] in file order"""
        return [(label, self.section(i)) for i, label in enumerate(self.labels)]

    def release(self) -> None:
        """frees the slot (waits first if the copy is still in flight); the arrays of `sections` are dead afterwards"""
        g, self._g = self._g, None
        if g is not None and g._h is not None:
            g._rst_snaps[self.slot] = None
            g._chk(g.L.aa_rst_snapshot_release(g._h, self.slot))


class Grid:
    """Device-resident Grid.  Method names follow the reference's call sites."""

    def __init__(self, grid: GridConfig, device: int = 0, strict: bool | None = None, ion_path: int = 0, nslab: int = 1, cuts=None):
        """nslab > 1: the Grid is cut into x3 slabs inside the library (aa_params.nslab), one per GPU.
        cuts (root planes K_0 = 0 .. K_nslab = rootNx3): the Grid is one level of a Mesh cut at those planes (aa_create_cut)."""
        self.cfg = grid
        self.L = load(strict)
        self.params = params_from_grid(grid, device, ion_path, 1 if cuts is not None else nslab)
        self.nvar = 5 + grid.run.nscal
        self._composite = cuts is not None or nslab > 1
        # (N1, N2, N3); a direction with one zone has no ghost zones (a 2-D Grid: N3 = 1, a 1-D Grid: N2 = N3 = 1; init_grid.c:144-174)
        self.N = tuple(n + 2 * NGHOST if n > 1 else 1 for n in grid.Nx)
        self.ndim = sum(1 for n in grid.Nx if n > 1)
        self.npin = 0                           # zones pinned by set_pinned_cells (aa_run_1d / aa_run_2d take none)
        self.in_mesh = False                    # a level of a Mesh (Mesh sets it): aa_run_2d refuses those
        h = C.c_void_p()
        self._h = None
        if cuts is not None:
            cuts = [int(k) for k in cuts]
            self._chk(self.L.aa_create_cut(C.byref(self.params), int(grid.disp[2]) if grid.level else 0, len(cuts) - 1,
                                           (C.c_int * len(cuts))(*cuts), C.byref(h)))
        else:
            self._chk(self.L.aa_create(C.byref(self.params), C.byref(h)))
        self._h = h
        self._keep = []
        # third order on a 2-D run, opt-in (config.RunConfig.order_2d): the setter behind aa_create, before any state arrives
        if getattr(grid.run, "order_2d", 2) != 2:
            try:
                self.set_order_2d(grid.run.order_2d)
            except AthenaError:
                self.close()
                raise

    def _chk(self, rc: int):
        if rc != 0:
            raise AthenaError(self.L.aa_last_error().decode() or f"athena_amd error {rc}")

    def close(self):
        if self._h is not None:
            # (aa_destroy waits for a snapshot in flight; its memory goes with the Grid)
            for s in list(getattr(self, "_snaps", ())) + list(getattr(self, "_rst_snaps", ())):
                if s is not None:
                    s._g = None
            self.L.aa_destroy(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state --------------------------------------------------------------------
    def new_host_block(self) -> np.ndarray:
        """A zeroed host ConsS block [N3][N2][N1][nvar] (GridS.U of the reference)."""
        return np.zeros((self.N[2], self.N[1], self.N[0], self.nvar), dtype=np.float64)

    def upload(self, U: np.ndarray):
        assert U.shape == (self.N[2], self.N[1], self.N[0], self.nvar) and U.dtype == np.float64
        U = np.ascontiguousarray(U)
        self._chk(self.L.aa_upload_cons(self._h, _dp(U)))

    def download(self) -> np.ndarray:
        U = self.new_host_block()
        self._chk(self.L.aa_download_cons(self._h, _dp(U)))
        return U

    def download_ghost_zones(self, U: np.ndarray):
        """refresh only the ghost zones of a host block whose active zones are current"""
        self._chk(self.L.aa_download_ghost_zones(self._h, _dp(U)))

    def download_edgeflux(self) -> np.ndarray:
        nx = self.cfg.Nx
        ef = np.zeros((nx[2] + 1, nx[1] + 1, nx[0] + 1))
        self._chk(self.L.aa_download_edgeflux(self._h, _dp(ef)))
        return ef

    def mesh_state(self):
        t = C.c_double(); dt = C.c_double(); n = C.c_int()
        self.L.aa_get_mesh_state(self._h, C.byref(t), C.byref(dt), C.byref(n))
        return t.value, dt.value, n.value

    def set_mesh_state(self, time: float, dt: float, nstep: int):
        self.L.aa_set_mesh_state(self._h, time, dt, nstep)

    time = property(lambda s: s.mesh_state()[0])
    dt = property(lambda s: s.mesh_state()[1])
    nstep = property(lambda s: s.mesh_state()[2])

    def set_stream(self, stream_ptr: int): self._chk(self.L.aa_set_stream(self._h, C.c_void_p(stream_ptr)))
    def sync(self): self._chk(self.L.aa_sync(self._h))
    def device_bytes(self) -> int: return int(self.L.aa_device_bytes(self._h))

    # ---- hooks --------------------------------------------------------------------
    def set_static_grav_pot(self, cfunc):
        """cfunc: a C function pointer double(double,double,double) (or None)."""
        cb = GRAVPOT(0) if cfunc is None else C.cast(cfunc, GRAVPOT)
        self._keep.append(cb)
        self._chk(self.L.aa_set_static_grav_pot(self._h, cb))

    def set_pinned_cells(self, index: np.ndarray, values: np.ndarray):
        index = np.ascontiguousarray(index, dtype=np.int64); values = np.ascontiguousarray(values, dtype=np.float64)
        self._chk(self.L.aa_set_pinned_cells(self._h, len(index),
                                             index.ctypes.data_as(C.POINTER(C.c_longlong)), _dp(values)))
        self.npin = len(index)

    def add_radplane_3d(self, dir: int, flux: float): self._chk(self.L.aa_add_radplane_3d(self._h, dir, flux))
    def has_radplane(self) -> bool: return bool(self.L.aa_has_radplane(self._h))

    # ---- call sites of the main loop ------------------------------------------------
    def bvals_mhd(self): self._chk(self.L.aa_bvals_mhd(self._h))
    def bvals_ionrad(self): self._chk(self.L.aa_bvals_ionrad(self._h))
    def new_dt(self): self._chk(self.L.aa_new_dt(self._h))
    def set_cooling(self, kind: int = 1):
        """CoolingFunc = KoyInut (kind 1, AA_COOL_KOYINUT) or NULL (0); CTU integrator only."""
        self._chk(self.L.aa_set_cooling(self._h, int(kind)))

    def set_fofc(self, on: bool = True):
        """configure --enable-fofc: first-order flux correction of the van Leer integrator (integrate_3d_vl.c Steps 10, 14);
        refused (AthenaError) for the CTU integrator, third order, levels of a Mesh and Grids cut into slabs."""
        self._chk(self.L.aa_set_fofc(self._h, 1 if on else 0))

    def fofc(self) -> bool: return bool(self.L.aa_get_fofc(self._h))

    def set_order_2d(self, order: int = 3):
        """configure --with-order on a 2-D Grid (Nx3 = 1), opt-in: 3 = piecewise parabolic (lr_states_ppm.c), 2 = piecewise linear.
        Before start / resume / the first step and before the Grid joins a Mesh; refused (AthenaError) on 1-D and 3-D Grids (those
        take aa_params.order), with CTU without H-correction, on a Grid that has stepped and on a level of a Mesh."""
        self._chk(self.L.aa_set_order_2d(self._h, int(order)))

    @property
    def order(self) -> int:
        """the effective reconstruction order: aa_params.order, or what set_order_2d made of a 2-D Grid"""
        return int(self.L.aa_get_order_2d(self._h))

    def fofc_counts(self):
        """(zones that had d < 0, zones that had P < 0, second-order fluxes replaced) of the last integrate_3d_vl"""
        c = (C.c_longlong * 3)(); self._chk(self.L.aa_get_fofc_counts(self._h, c)); return int(c[0]), int(c[1]), int(c[2])

    def integrate_3d_ctu(self): self._chk(self.L.aa_integrate_3d_ctu(self._h))
    def integrate_3d_vl(self): self._chk(self.L.aa_integrate_3d_vl(self._h))
    def integrate_2d_ctu(self): self._chk(self.L.aa_integrate_2d_ctu(self._h))
    def integrate_2d_vl(self): self._chk(self.L.aa_integrate_2d_vl(self._h))
    def integrate_1d_ctu(self): self._chk(self.L.aa_integrate_1d_ctu(self._h))
    def integrate_1d_vl(self): self._chk(self.L.aa_integrate_1d_vl(self._h))
    def integrate_begin(self): self._chk(self.L.aa_integrate_begin(self._h))
    def ion_speculate(self, limit: float): self._chk(self.L.aa_ion_speculate(self._h, float(limit)))
    def cfl_in_update(self, on: bool = True): self._chk(self.L.aa_cfl_in_update(self._h, 1 if on else 0))

    def integrate(self):
        """(*Integrate)(pD): the function pointer integrate_init() selected (integrate.c:63-75)."""
        vl = self.cfg.run.integrator == "vl"
        if self.ndim == 1:                                      # integrate.c:36-47
            self.integrate_1d_vl() if vl else self.integrate_1d_ctu()
        elif self.ndim == 2:                                    # :49-58
            self.integrate_2d_vl() if vl else self.integrate_2d_ctu()
        elif vl:
            self.integrate_3d_vl()
        else:
            self.integrate_3d_ctu()
    def apply_pinned_cells(self): self._chk(self.L.aa_apply_pinned_cells(self._h))
    def start(self): self._chk(self.L.aa_start(self._h))

    def resume(self):
        """The start sequence of a restarted run (main.c:398-451): bvals_mhd and bvals_ionrad, NO new_dt."""
        self._chk(self.L.aa_resume(self._h))

    def ion_radtransfer_3d(self) -> int:
        n = C.c_int(); self._chk(self.L.aa_ion_radtransfer_3d(self._h, C.byref(n))); return n.value

    def step(self) -> int:
        n = C.c_int(); self._chk(self.L.aa_step(self._h, C.byref(n))); return n.value

    def _run(self, call, t_stop, tlim, nstep_stop) -> int:
        """the arguments of aa_run_1d / aa_run_2d / aa_run_3d: tlim None is the deck's, nstep_stop None is 2^20 steps ahead -> the steps taken"""
        n = C.c_int()
        tlim = self.cfg.run.tlim if tlim is None else tlim
        stop = self.nstep + (1 << 20) if nstep_stop is None else int(nstep_stop)
        self._chk(call(self._h, float(t_stop), float(tlim), stop, C.byref(n)))
        return n.value

    def run_cap(self) -> int:
        """most active zones of a 1-D Grid that run_until keeps resident in one workgroup (aa_run_1d_cap)"""
        return int(self.L.aa_run_1d_cap())

    def can_run_until(self) -> bool:
        """whether run_until takes this Grid: 1-D, up to run_cap() active zones, no pinned zones -- the refusals of aa_run_1d"""
        return self.ndim == 1 and self.cfg.Nx[0] <= self.run_cap() and self.npin == 0

    def run_until(self, t_stop: float, tlim: float | None = None, nstep_stop: int | None = None) -> int:
        """Whole passes of the main loop on a 1-D Grid in ONE launch (aa_run_1d): until time >= t_stop, nstep == nstep_stop or
        dt <= 0; new_dt clips at tlim (default: the deck's).  nstep_stop None: 2^20 steps ahead at the most.  Returns the steps
        taken.  AthenaError on a Grid that is not 1-D, is above run_cap() zones or has pinned zones (can_run_until)."""
        return self._run(self.L.aa_run_1d, t_stop, tlim, nstep_stop)

    def run_2d_batch(self) -> int:
        """steps run_2d queues per read-back on this Grid (AA_2D_BATCH when the Grid was made; 0: it steps one at a time)"""
        return int(self.L.aa_run_2d_batch(self._h))

    def can_run_2d(self) -> bool:
        """whether run_2d takes this Grid: 2-D, no pinned zones, not a level of a Mesh -- the refusals of aa_run_2d"""
        return self.ndim == 2 and self.npin == 0 and not self.in_mesh and self.cfg.level == 0

    def run_2d(self, t_stop: float, tlim: float | None = None, nstep_stop: int | None = None) -> int:
        """Whole passes of the main loop on a 2-D Grid with the time step picked on the device (aa_run_2d): AA_2D_BATCH steps are
        queued per read-back instead of one; until time >= t_stop, nstep == nstep_stop or dt <= 0; new_dt clips at tlim (default:
        the deck's).  nstep_stop None: 2^20 steps ahead at the most.  Returns the steps taken; the same bits as that many step()
        calls.  AthenaError on a Grid that is not 2-D, has pinned zones or is a level of a Mesh (can_run_2d)."""
        return self._run(self.L.aa_run_2d, t_stop, tlim, nstep_stop)

    def run_3d_batch(self) -> int:
        """steps run_3d queues per read-back on this Grid (AA_3D_BATCH when the Grid was made); 0: it steps one at a time -- the
        knob at 0, or a Grid off the default CTU chain (van Leer, cooling, ion radiation, a kernel switch, fewer than 4 zones along
        a direction) -- or the Grid is not 3-D"""
        return int(self.L.aa_run_3d_batch(self._h))

    def can_run_3d(self) -> bool:
        """whether run_3d takes this Grid: 3-D, no pinned zones, not cut into slabs, not a level of a Mesh -- the refusals of aa_run_3d"""
        return self.ndim == 3 and self.npin == 0 and not self._composite and not self.in_mesh and self.cfg.level == 0

    def run_3d(self, t_stop: float, tlim: float | None = None, nstep_stop: int | None = None) -> int:
        """Whole passes of the main loop on a 3-D hydro Grid with the time step picked on the device (aa_run_3d): AA_3D_BATCH steps
        of the default CTU chain are queued per read-back instead of one; until time >= t_stop, nstep == nstep_stop or dt <= 0;
        new_dt clips at tlim (default: the deck's).  nstep_stop None: 2^20 steps ahead at the most.  Returns the steps taken; the
        same bits as that many step() calls (a Grid with run_3d_batch() == 0 takes them one at a time).  AthenaError on a Grid
        that is not 3-D, has pinned zones, is cut into slabs or is a level of a Mesh (can_run_3d)."""
        return self._run(self.L.aa_run_3d, t_stop, tlim, nstep_stop)

    def run_hst_arm(self, t_next: float, dt_out: float, nlim: int | None = None) -> None:
        """Arms a history schedule for the NEXT run_2d / run_3d call only (aa_run_hst_arm): behind every step of that call after
        which the main loop goes on (time < tlim, nstep != nlim; None: no such limit) and time >= t_next, a row is made on the
        device -- queued or step by step inside the call, the same rows -- and t_next += dt_out ONCE.  The call disarms itself.
        AthenaError on a 1-D Grid, a Grid cut into slabs, a level of a Mesh."""
        self._chk(self.L.aa_run_hst_arm(self._h, float(t_next), float(dt_out), -1 if nlim is None else int(nlim)))

    def run_hst_rows(self):
        """-> (rows, t_next) of the last armed run call (aa_run_hst_rows): rows[n][11] = time, dt and the nine sums of history()
        behind the n-th step that had a row due; t_next: the schedule's next time behind them"""
        n, t = C.c_int(), C.c_double()
        self._chk(self.L.aa_run_hst_rows(self._h, 0, None, C.byref(n), C.byref(t)))
        rows = np.zeros((n.value, HST_ROW))
        if n.value:
            self._chk(self.L.aa_run_hst_rows(self._h, n.value, _dp(rows), C.byref(n), C.byref(t)))
        return rows, t.value

    # ---- phases ----------------------------------------------------------------------
    def new_dt_local(self) -> float:
        v = C.c_double(); self._chk(self.L.aa_new_dt_local(self._h, C.byref(v))); return v.value

    def ion_begin(self): self._chk(self.L.aa_ion_begin(self._h))

    def ion_rates(self):
        a = C.c_double(); b = C.c_double()
        self._chk(self.L.aa_ion_rates(self._h, C.byref(a), C.byref(b))); return a.value, b.value

    def ion_update(self, dt: float):
        c = C.c_longlong(); h = C.c_double()
        self._chk(self.L.aa_ion_update(self._h, dt, C.byref(c), C.byref(h))); return c.value, h.value

    # the one-kernel sub-cycle (aa_ion_is_fused): pass / [all-gather of the words] / pick / fetch
    def ion_is_fused(self) -> bool: return bool(self.L.aa_ion_is_fused(self._h))

    def ion_pass(self, update: bool, sweep: bool, dev_words: int = 0):
        self._chk(self.L.aa_ion_pass(self._h, int(update), int(sweep), C.c_void_p(dev_words or None)))

    def ion_pick(self, dev_words_all: int, nranks: int, first: bool, limit: float):
        self._chk(self.L.aa_ion_pick(self._h, C.c_void_p(dev_words_all or None), nranks, int(first), limit))

    def ion_fetch(self):
        """-> (dt, limit_hit, dt_chem, dt_therm, cellcount, dt_hydro, neg_dt_chem) of the update the last pass applied:
        the one read-back of a sub-cycle"""
        dt = C.c_double(); a = C.c_double(); b = C.c_double(); h = C.c_double(); hit = C.c_int(); neg = C.c_int(); n = C.c_longlong()
        self._chk(self.L.aa_ion_fetch(self._h, C.byref(dt), C.byref(hit), C.byref(a), C.byref(b), C.byref(n), C.byref(h), C.byref(neg)))
        return dt.value, bool(hit.value), a.value, b.value, n.value, h.value, bool(neg.value)

    def ion_finish(self): self._chk(self.L.aa_ion_finish(self._h))

    def ion_lean_counts(self):
        """(dense, lean, redone): speculating first passes in either form, and lean ones that were refuted (AA_ION_LEAN)."""
        n = (C.c_longlong * 3)()
        self._chk(self.L.aa_ion_lean_counts(self._h, n))
        return tuple(int(v) for v in n)

    def set_ion_batch(self, k: int):
        """radiation sub-cycles queued per host visit (1 .. 256; AA_ION_BATCH when the Grid was made, default 1 = a read-back per
        sub-cycle): with k > 1 the library's loop (ion_radtransfer_3d, step) applies the stop tests on the device.  Same bits."""
        self._chk(self.L.aa_set_ion_batch(self._h, int(k)))

    @property
    def ion_batch(self) -> int: return int(self.L.aa_ion_batch(self._h))

    def ion_batch_active(self) -> bool:
        """whether this Grid's ion step takes the queued loop: ion_batch > 1 on the one-kernel sub-cycle with the fused pick, one device"""
        return bool(self.L.aa_ion_batch_active(self._h))

    def ion_batch_counts(self):
        """(host visits, sub-cycles executed, queued sub-cycles that left at once) of the queued loop since the Grid was made"""
        n = (C.c_longlong * 3)()
        self._chk(self.L.aa_ion_batch_counts(self._h, n))
        return tuple(int(v) for v in n)

    def ion_radtransfer_3d_gather(self, dev_words: int, dev_words_all: int, nranks: int, gather) -> int:
        """ion_radtransfer_3d of one rank of a multi-rank run in ONE call: `gather()` is the driver's all-gather of the
        AA_ION_WORDS doubles at dev_words into dev_words_all, called once per pass on this Grid's stream."""
        err = []

        def cb(_ctx):
            try:
                gather(); return 0
            except BaseException as e:      # an exception must not cross the C frames: hand it over afterwards
                err.append(e); return 1
        n = C.c_int()
        rc = self.L.aa_ion_radtransfer_3d_gather(self._h, C.c_void_p(dev_words), C.c_void_p(dev_words_all), nranks, GATHER(cb), None, C.byref(n))
        if err:
            raise err[0]
        self._chk(rc)
        return n.value

    def host_syncs(self, reset: bool = False) -> int: return int(self.L.aa_host_syncs(self._h, int(reset)))

    def cfl_max_v(self):
        v = (C.c_double * 3)(); self._chk(self.L.aa_cfl_max_v(self._h, v)); return list(v)

    def flux_x3_export(self, side: int, dev_ptr: int): self._chk(self.L.aa_flux_x3_export(self._h, side, C.c_void_p(dev_ptr)))

    def flux_x3_apply(self, side: int, i0: int, j0: int, n1: int, n2: int, dev_ptr: int):
        self._chk(self.L.aa_flux_x3_apply(self._h, side, i0, j0, n1, n2, C.c_void_p(dev_ptr)))

    def halo_doubles(self) -> int: return int(self.L.aa_halo_doubles(self._h))
    def pack_x3(self, side: int, dev_ptr: int): self._chk(self.L.aa_pack_x3(self._h, side, C.c_void_p(dev_ptr)))
    def unpack_x3(self, side: int, dev_ptr: int): self._chk(self.L.aa_unpack_x3(self._h, side, C.c_void_p(dev_ptr)))
    def halo_doubles_x2(self) -> int: return int(self.L.aa_halo_doubles_x2(self._h))
    def pack_x2(self, side: int, dev_ptr: int): self._chk(self.L.aa_pack_x2(self._h, side, C.c_void_p(dev_ptr)))
    def unpack_x2(self, side: int, dev_ptr: int): self._chk(self.L.aa_unpack_x2(self._h, side, C.c_void_p(dev_ptr)))
    def bvals_mhd_side(self, dir: int, side: int): self._chk(self.L.aa_bvals_mhd_side(self._h, dir, side))

    def history(self) -> np.ndarray:
        """Volume integrals of this Grid in .hst column order (dump_history.c:157-200)."""
        s = np.zeros(9); self._chk(self.L.aa_history(self._h, _dp(s))); return s

    # ---- data dumps (dump_vtk.c / dump_binary.c) ----------------------------------------
    def dump_sections(self, fmt) -> int:
        from . import dumps
        return int(self.L.aa_dump_sections(self._h, dumps.FORMATS.get(fmt, fmt)))

    def dump_section(self, fmt, prim: bool, section: int, out: np.ndarray | None = None) -> np.ndarray:
        """Section `section` of the vtk / bin payload of the ACTIVE zones, made on the device in file order and byte order
        (csrc/dump.hip; fmt "vtk" | "bin").  The array holds the file's words: view it as ">f4" (vtk) or "<f4" (bin) for values."""
        from . import dumps
        fmt = dumps.FORMATS.get(fmt, fmt)
        n = int(self.L.aa_dump_section_floats(self._h, fmt, section))
        if n <= 0:
            raise AthenaError(f"[dump_section]: no section {section} in format {fmt}")
        if out is None:
            out = np.empty(n, dtype=np.float32)
        assert out.dtype == np.float32 and out.size == n and out.flags.c_contiguous
        self._chk(self.L.aa_dump_section(self._h, fmt, 1 if prim else 0, section, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def write_dump(self, path: str, fmt, prim: bool, level: int | None = None, domain: int = 0,
                   time: float | None = None, dt: float | None = None):
        """dump_vtk / dump_binary of this Grid: the header from the Grid's geometry and MeshS time / dt (or the ones given:
        a driver that keeps them itself), the sections from the device."""
        from . import dumps
        buf = {}

        def section(i):
            n = int(self.L.aa_dump_section_floats(self._h, dumps.FORMATS.get(fmt, fmt), i))
            if n not in buf:
                buf[n] = np.empty(n, dtype=np.float32)
            return self.dump_section(fmt, prim, i, buf[n])
        dumps.write_dump(path, fmt, section, **self.dump_geometry(prim, level, domain, time, dt))

    def dump_geometry(self, prim: bool, level: int | None = None, domain: int = 0, time: float | None = None,
                      dt: float | None = None) -> dict:
        """what the header of a dump of this Grid says (the keywords of dumps.write_dump / dumps.dump_head)"""
        g = self.cfg; r = g.run
        lev = g.level if level is None else level
        # (init_mesh.c:331-337: a direction with one zone -- x3 of a 2-D Grid -- keeps the root's extent on every level)
        dx = tuple(r.dx[d] / float(1 << g.level) if g.Nx[d] > 1 else r.dx[d] for d in range(3))
        if time is None or dt is None:
            t_, dt_, _ = self.mesh_state()
            time = t_ if time is None else time; dt = dt_ if dt is None else dt
        return dict(nx=g.Nx, minx=g.MinX, dx=dx, time=time, dt=dt, gamma=r.gamma, prim=prim, nscal=r.nscal, level=lev, domain=domain)

    # ---- single-variable outputs (output.c OutData1/2/3, expr_*; csrc/outdata.hip) -------------------------------------------
    def _outdata_args(self, expr, reduce, lo, hi):
        from . import dumps
        ex = dumps.EXPR[expr] if isinstance(expr, str) else int(expr)
        I3 = C.c_int * 3
        return ex, I3(*[1 if r else 0 for r in reduce]), I3(*[int(v) for v in lo]), I3(*[int(v) for v in hi]), I3()

    def outdata(self, expr, reduce=(0, 0, 0), lo=(0, 0, 0), hi=(0, 0, 0)):
        """-> (payload [n3][n2][n1] of doubles, a reduced direction having one element; dmin; dmax) of the expression `expr`
        ("d" .. "cs2", "flux", or its AA_OUT_* code) over the active zones: reduce[a] sums zones lo[a] .. hi[a] (inclusive, from 0)
        of direction a and multiplies by 1.0/count, as OutData1/2 do (aa_outdata)."""
        ex, red, l, h, dims = self._outdata_args(expr, reduce, lo, hi)
        self._chk(self.L.aa_outdata_dims(self._h, ex, red, l, h, dims))
        data = np.empty((dims[2], dims[1], dims[0]), dtype=np.float64)
        dmin, dmax = C.c_double(), C.c_double()
        self._chk(self.L.aa_outdata(self._h, ex, red, l, h, _dp(data), dims, C.byref(dmin), C.byref(dmax)))
        return data, dmin.value, dmax.value

    def outdata_gray(self, expr, reduce, lo, hi, dmin: float, dmax: float) -> np.ndarray:
        """the bytes of the pgm image of the same payload scaled with dmin / dmax, in file order (aa_outdata_gray)"""
        ex, red, l, h, dims = self._outdata_args(expr, reduce, lo, hi)
        self._chk(self.L.aa_outdata_dims(self._h, ex, red, l, h, dims))
        img = np.empty(dims[0] * dims[1] * dims[2], dtype=np.uint8)
        self._chk(self.L.aa_outdata_gray(self._h, ex, red, l, h, float(dmin), float(dmax),
                                         img.ctypes.data_as(C.POINTER(C.c_ubyte)), dims))
        return img

    # ---- the same payload beside the run: one kernel, one copy, two slots (csrc/dump.hip aa_dump_snapshot_*) -----------------
    DUMP_SLOTS = 2                       # AA_DUMP_SLOTS

    @property
    def composite(self) -> bool:
        """a Grid cut into slabs inside the library: one handle for several devices (no snapshots: dump_section is the path)"""
        return bool(getattr(self, "_composite", False))

    def dump_snapshot_bytes(self, fmt) -> int:
        from . import dumps
        return int(self.L.aa_dump_snapshot_bytes(self._h, dumps.FORMATS.get(fmt, fmt)))

    def dump_snapshot(self, fmt, prim: bool, max_bytes: int = 8 << 30) -> "Snapshot":
        """The whole payload of a dump of the state as it is now, on its way to page-locked host memory while the run goes on:
        the kernel is queued behind what the step launched, the copy runs beside what comes next, nothing waits.  Takes the
        first free slot of the two; with both held the library refuses (AthenaError) -- release one.  Call this, and every
        method of the Snapshot, from the thread that drives the run; another thread may read the arrays `section` returns."""
        from . import dumps
        fmt = dumps.FORMATS.get(fmt, fmt)
        if not hasattr(self, "_snaps"):
            self._snaps = [None] * self.DUMP_SLOTS      # the Snapshots that hold this Grid's slots
        free =[i for i, s in enumerate(self._snaps) if s is None]
        slot = free[0] if free else 0                 # (none free: the library names the refusal)
        self._chk(self.L.aa_dump_snapshot_begin(self._h, slot, fmt, 1 if prim else 0, int(max_bytes)))
        s = self._snaps[slot] = Snapshot(self, slot, fmt, prim)
        return s

    # ---- restart dumps (restart.c): the sections of this Grid to and from the device -----------
    def rst_sections(self):
        """[(label, doubles)] of this Grid's sections in file order (csrc/restart.hip)."""
        out = []
        buf = C.create_string_buffer(32)
        for s in range(int(self.L.aa_rst_sections(self._h))):
            self._chk(self.L.aa_rst_section_label(self._h, s, buf, len(buf)))
            out.append((buf.value.decode(), int(self.L.aa_rst_section_doubles(self._h, s))))
        return out

    def rst_section(self, s: int, out: np.ndarray | None = None) -> np.ndarray:
        """Section `s` of the restart payload: the ACTIVE zones [k][j][i] of one variable (or EdgeFlux) in double precision."""
        n = int(self.L.aa_rst_section_doubles(self._h, s))
        if n <= 0:
            raise AthenaError(f"[rst_section]: no section {s}")
        if out is None:
            out = np.empty(n, dtype=np.float64)
        assert out.dtype == np.float64 and out.size == n and out.flags.c_contiguous
        self._chk(self.L.aa_rst_section_get(self._h, s, _dp(out)))
        return out

    # ---- the restart payload beside the run: one kernel, one copy, ONE slot (csrc/restart.hip aa_rst_snapshot_*) ---------------
    RST_SLOTS = 1                        # AA_RST_SLOTS

    def rst_snapshot_bytes(self) -> int:
        """of the restart payload with its padding: what the slot's device buffer and its page-locked twin each take"""
        return int(self.L.aa_rst_snapshot_bytes(self._h))

    def rst_snapshot(self, max_bytes: int = 8 << 30) -> "RstSnapshot":
        """The restart payload of the state as it is now -- every section of rst_sections() -- on its way to page-locked host
        memory while the run goes on (k_rst_payload and the EdgeFlux copy queued behind what the step launched, one copy beside
        what comes next, nothing waits; the face-state area and the sweeps of integrate_begin are left alone).  One slot: while
        it is held the library refuses (AthenaError) -- release it.  The threading rule is dump_snapshot's."""
        if not hasattr(self, "_rst_snaps"):
            self._rst_snaps = [None] * self.RST_SLOTS      # the RstSnapshots that hold this Grid's slots
        free = [i for i, s in enumerate(self._rst_snaps) if s is None]
        slot = free[0] if free else 0                    # (none free: the library names the refusal)
        self._chk(self.L.aa_rst_snapshot_begin(self._h, slot, int(max_bytes)))
        s = self._rst_snaps[slot] = RstSnapshot(self, slot)
        return s

    def put_rst_section(self, s: int, arr: np.ndarray):
        """The inverse of rst_section: writes the active zones on the device and no ghost zone."""
        n = int(self.L.aa_rst_section_doubles(self._h, s))
        if n <= 0:
            raise AthenaError(f"[put_rst_section]: no section {s}")
        assert arr.dtype == np.float64 and arr.size == n and arr.flags.c_contiguous
        self._chk(self.L.aa_rst_section_put(self._h, s, _dp(arr)))

    def _rst_buffer(self) -> np.ndarray:
        n = max(n for _, n in self.rst_sections())
        if getattr(self, "_rst_buf", None) is None or self._rst_buf.size < n:
            self._rst_buf = np.empty(n, dtype=np.float64)
        return self._rst_buf

    def write_rst_payload(self, f):
        """This Grid's labelled sections as dump_restart writes them (restart.c:531-770), one at a time through one host buffer."""
        buf = self._rst_buffer()
        for s, (label, n) in enumerate(self.rst_sections()):
            f.write(b"\n" + label.encode() + b"\n")
            f.write(memoryview(self.rst_section(s, buf[:n])).cast("B"))

    def read_rst_payload(self, f):
        """The inverse: `f` stands at this Grid's first label (restart_grids, restart.c:52-456)."""
        from . import restart
        buf = self._rst_buffer()
        for s, (label, n) in enumerate(self.rst_sections()):
            restart.expect_label(f, label)
            if f.readinto(memoryview(buf[:n]).cast("B")) != 8 * n:
                raise restart.RestartError(f"[restart_grids]: Expected {n} doubles of {label}, found the end of the file")
            self.put_rst_section(s, buf[:n])

    # ---- boxes of a section: resuming on, and writing for, another decomposition ------------------
    def rst_get_box(self, s: int, lo, n, out: np.ndarray | None = None) -> np.ndarray:
        """The part [lo, lo + n) of section `s`, (x1, x2, x3) in the section's own index space (active zones; the face indices
        for EDGEFLUX): [n3][n2][n1] doubles, the slice of rst_section."""
        lo3 = (C.c_int * 3)(*[int(v) for v in lo]); n3 = (C.c_int * 3)(*[int(v) for v in n])
        cnt = max(0, int(n[0])) * max(0, int(n[1])) * max(0, int(n[2]))
        if out is None:
            out = np.empty(cnt, dtype=np.float64)
        assert out.dtype == np.float64 and out.size == cnt and out.flags.c_contiguous
        self._chk(self.L.aa_rst_section_get_box(self._h, s, lo3, n3, _dp(out)))
        return out.reshape(max(0, int(n[2])), max(0, int(n[1])), max(0, int(n[0])))

    def rst_put_box(self, s: int, lo, n, arr: np.ndarray):
        """The inverse: writes the box and nothing outside it (no ghost zone)."""
        lo3 = (C.c_int * 3)(*[int(v) for v in lo]); n3 = (C.c_int * 3)(*[int(v) for v in n])
        cnt = max(0, int(n[0])) * max(0, int(n[1])) * max(0, int(n[2]))
        assert arr.dtype == np.float64 and arr.size == cnt and arr.flags.c_contiguous
        self._chk(self.L.aa_rst_section_put_box(self._h, s, lo3, n3, _dp(arr)))

    def write_rst_box_payload(self, f, lo, n):
        """The labelled sections of the Grid [lo, lo + n) of this Grid's active zones, as a rank that held just that Grid would
        write them (EDGEFLUX with its n + 1 faces)."""
        for s, (label, _cnt) in enumerate(self.rst_sections()):
            e = 1 if label == "EDGEFLUX" else 0
            f.write(b"\n" + label.encode() + b"\n")
            f.write(memoryview(self.rst_get_box(s, lo, [int(v) + e for v in n])).cast("B"))

    def read_rst_boxes(self, sources, Nx, lo, n):
        """This Grid = [lo, lo + n) of a Domain of `Nx` zones from the files that hold it -- restart.scan_sources for the root
        Domain of a single-level run, one Domain's list of restart.scan_mesh_sources for a refined mesh (lo relative to the
        Domain): section by section, every source's part of it (restart.box_pieces) straight to the device -- never more than
        one such part in host memory."""
        from . import restart
        for s, (label, _cnt) in enumerate(self.rst_sections()):
            e = 1 if label == "EDGEFLUX" else 0
            for src, slo, dlo, ext in restart.box_pieces(sources, Nx, lo, [int(v) + e for v in n], bool(e)):
                found = src["levels"][src.get("entry", 0)][s][0]
                if found != label:
                    raise restart.RestartError(f"[restart_grids]: Expected {label}, found {found}")
                self.rst_put_box(s, dlo, ext, restart.read_box(src, s, slo, ext))

    def read_rst_joined(self, sources, Nx):
        """The same for a handle that takes whole sections only (a Grid cut into slabs inside the library): one section of this
        Grid = the whole Domain at a time is joined on the host (restart.read_section_boxes) and goes in through put_rst_section."""
        from . import restart
        for s, (label, cnt) in enumerate(self.rst_sections()):
            found = sources[0]["levels"][sources[0].get("entry", 0)][s][0]
            if found != label:
                raise restart.RestartError(f"[restart_grids]: Expected {label}, found {found}")
            a = restart.read_section_boxes(sources, Nx, s).reshape(-1)
            if a.size != cnt:
                raise restart.RestartError(f"[restart_grids]: Expected {cnt} doubles of {label}, found {a.size}")
            self.put_rst_section(s, a)

    # ---- measurement -------------------------------------------------------------------
    def profile_enable(self, on: bool = True): self.L.aa_profile_enable(self._h, 1 if on else 0)
    def profile_reset(self): self.L.aa_profile_reset(self._h)

    def profile(self):
        out = {}
        for i in range(self.L.aa_profile_count(self._h)):
            ms = C.c_double(); n = C.c_longlong()
            self._chk(self.L.aa_profile_get(self._h, i, C.byref(ms), C.byref(n)))
            out[self.L.aa_profile_name(self._h, i).decode()] = (ms.value, n.value)
        return out


def setup_problem(grid: GridConfig, device: int = 0, strict: bool | None = None, ion_path: int = 0, nslab: int = 1,
                  initial: bool = True, cuts=None) -> Grid:
    """problem(DomainS*) of the reference for the shipped decks: fill the host block with the
    C problem generator, upload it, register the hooks (main.c:393).  initial = False is problem_read_restart
    (ioniz_sphere.c:191-239): the hooks only -- no host block is built, the state comes from a restart dump."""
    r = grid.run; pr = r.prob
    g = Grid(grid, device, strict, ion_path, nslab, cuts)
    if getattr(r, "fofc", False):
        try:
            g.set_fofc(True)
        except AthenaError:
            g.close()
            raise
    H = host()
    U = g.new_host_block() if initial else None
    if r.problem not in ("ifront", "ioniz_sphere", "blast", "shkset1d"):
        raise AthenaError(f"unknown problem {r.problem}")
    if not initial:
        rc = 0
        if r.problem == "ioniz_sphere":          # the constants behind PlanetPot and the pinned zones (a process that resumes never ran the generator)
            rc = H.aa_problem_ioniz_sphere_restart(C.byref(g.params), pr["cs"], pr.get("rp", 1.2e10), pr.get("mp", 1.0e30),
                                                   pr.get("np", 6.0e8))
    elif r.problem == "ifront":
        rc = H.aa_problem_ifront(C.byref(g.params), pr["n_H"], pr["cs"], _dp(U))
    elif r.problem == "ioniz_sphere":
        rc = H.aa_problem_ioniz_sphere(C.byref(g.params), pr["cs"], pr.get("rp", 1.2e10),
                                       pr.get("mp", 1.0e30), pr.get("np", 6.0e8), _dp(U))
    elif r.problem == "blast":
        rc = H.aa_problem_blast(C.byref(g.params), pr["radius"], pr["pamb"], pr.get("damb", 1.0),
                                pr.get("drat", 1.0), pr["prat"], _dp(U))
    elif r.problem == "shkset1d":
        wl = np.array([pr["dl"], pr["pl"], pr["v1l"], pr["v2l"], pr["v3l"]])
        wr = np.array([pr["dr"], pr["pr"], pr["v1r"], pr["v2r"], pr["v3r"]])
        rc = H.aa_problem_shkset1d(C.byref(g.params), _dp(wl), _dp(wr), int(pr["shk_dir"]), _dp(U))
    else:
        raise AthenaError(f"unknown problem {r.problem}")
    if rc != 0:
        raise AthenaError(f"problem generator {r.problem} rejected the configuration")
    if initial:
        g.upload(U)
    if r.problem == "ioniz_sphere":
        g.set_static_grav_pot(H.aa_planet_pot)                           # StaticGravPot = PlanetPot
        n = H.aa_ioniz_sphere_pinned(C.byref(g.params), None, None)
        idx = np.zeros(max(n, 1), dtype=np.int64); val = np.zeros((max(n, 1), 6))
        H.aa_ioniz_sphere_pinned(C.byref(g.params), idx.ctypes.data_as(C.POINTER(C.c_longlong)), _dp(val))
        g.set_pinned_cells(idx[:n], val[:n])
    if r.ion:
        if pr.get("trad", 0.0) >= 1.0e-20:                               # ioniz_sphere.c:168-170
            g.close()
            raise AthenaError("Delaying ionization not currently enabled for use with SMR + MPI")
        g.add_radplane_3d(-1, pr["flux"])
    g.host_initial = U
    return g


class Mesh:
    """Nested static-mesh-refinement levels on one GPU (MeshS; one or several Domains per level: grids level by level
    from the root, deck order inside a level, as config.levels() returns them).  Method
    names follow the reference: RestrictCorrect, Prolongate (smr.c), new_dt, and the per-level
    ion_radtransfer_3d with its coarse -> fine EdgeFlux hand-off (ionrad_smr.c)."""

    def __init__(self, grids, device: int = 0, strict: bool | None = None, links=None, ion_path: int = 0, initial: bool = True,
                 nslab: int = 1, cuts=None):
        """links: config.LinkConfig list for one rank's stack of slabs (multi-GPU SMR); None = the whole Mesh.
        initial = False: the hooks only, the state of every level comes from a restart dump (setup_problem).
        nslab > 1 (or cuts given): every level is cut at the same root x3 planes, one slab stack per GPU, inside the library
        (aa_create_cut + aa_mesh_create); cuts = None: config.balanced_cuts(grids, nslab)."""
        from . import config
        if cuts is not None:
            nslab = len(cuts) - 1
        self.nslab = int(nslab)
        self.cuts = None
        if self.nslab > 1 or cuts is not None:
            if links is not None:
                raise AthenaError("[Mesh]: a rank's stack of slabs (links) is not cut again inside the library")
            self.cuts = tuple(int(k) for k in (cuts if cuts is not None else config.balanced_cuts(list(grids), self.nslab)))
        self.lev = []
        try:
            for g in grids:
                self.lev.append(setup_problem(g, device, strict, ion_path, initial=initial, cuts=self.cuts))
        except Exception:
            for g in self.lev:
                g.close()
            raise
        self.L = self.lev[0].L
        n = len(grids)
        hs = (C.c_void_p * n)(*[g._h for g in self.lev])
        h = C.c_void_p()
        self._h = None
        if links is None:
            disp = (C.c_int * (3 * n))(*[g.disp[d] if g.level else 0 for g in grids for d in range(3)])
            # (Grids with Nx3 = 1: the 2-D constructor -- nesting in x1 and x2, the 2-D integrators and coupling kernels)
            create = self.L.aa_mesh_create_2d if all(g.Nx[2] == 1 for g in grids) else self.L.aa_mesh_create
            self._chk(create(n, hs, disp, C.byref(h)))
        else:
            flat = [v for L_ in links for v in (*L_.cs, *L_.n, *L_.prol, *L_.corr, *L_.cdisp)]
            arr = (C.c_int * max(1, len(flat)))(*flat)
            self._chk(self.L.aa_mesh_create_local(n, hs, arr, C.byref(h)))
        self._h = h
        self.links = links                      # a rank's stack of slabs (run_2d refuses it)
        for g in self.lev:
            g.in_mesh = True                    # (the levels step together: Grid.can_run_2d says no)

    def _chk(self, rc: int):
        if rc != 0:
            raise AthenaError(self.L.aa_last_error().decode() or f"athena_amd error {rc}")

    def close(self):
        if self._h is not None:
            self.L.aa_mesh_destroy(self._h); self._h = None
            for g in self.lev:
                g.in_mesh = False
        for g in self.lev:
            g.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def state(self):
        t = C.c_double(); dt = C.c_double(); n = C.c_int()
        self.L.aa_mesh_get_state(self._h, C.byref(t), C.byref(dt), C.byref(n))
        return t.value, dt.value, n.value

    time = property(lambda s: s.state()[0])
    dt = property(lambda s: s.state()[1])
    nstep = property(lambda s: s.state()[2])

    def set_stream(self, stream_ptr: int): self._chk(self.L.aa_mesh_set_stream(self._h, C.c_void_p(stream_ptr)))
    def RestrictCorrect(self): self._chk(self.L.aa_mesh_restrict_correct(self._h))
    def restrict_correct_pair(self, l: int): self._chk(self.L.aa_mesh_restrict_correct_pair(self._h, l))
    def ionradRestrictCorrect(self): self._chk(self.L.aa_mesh_ionrad_restrict_correct(self._h))
    def Prolongate(self): self._chk(self.L.aa_mesh_prolongate(self._h))
    def new_dt(self): self._chk(self.L.aa_mesh_new_dt(self._h))

    def ion_radtransfer_3d(self, level: int) -> int:
        n = C.c_int(); self._chk(self.L.aa_mesh_ion_radtransfer(self._h, level, C.byref(n))); return n.value

    def ionflux_prolong(self, level: int): self._chk(self.L.aa_mesh_ionflux_prolong(self._h, level))

    def set_ion_batch(self, k: int):
        """Grid.set_ion_batch on every level"""
        for g in self.lev:
            g.set_ion_batch(k)

    def start(self):
        self._chk(self.L.aa_mesh_start(self._h)); return self

    def resume(self):
        """aa_mesh_start without new_dt: the start sequence of a restarted run (main.c:398-451)"""
        self._chk(self.L.aa_mesh_resume(self._h)); return self

    def set_state(self, time: float, dt: float, nstep: int):
        """MeshS time / dt / nstep, and every level's copy of them (as aa_mesh_new_dt leaves them)"""
        self._chk(self.L.aa_mesh_set_state(self._h, time, dt, nstep))
        for g in self.lev:
            g.set_mesh_state(time, dt, nstep)

    # ---- restart snapshots, per level (lib.Grid.rst_snapshot of self.lev[l]; driver.MeshRun hands outputs.overlapped_restart the levels)
    RST_SLOTS = RstSnapshot.RST_SLOTS

    def rst_snapshot_bytes(self, l: int) -> int: return self.lev[l].rst_snapshot_bytes()
    def rst_snapshot(self, l: int, max_bytes: int = 8 << 30) -> "RstSnapshot": return self.lev[l].rst_snapshot(max_bytes)

    def domain_numbers(self):
        """(level, domain) of every Grid in self.lev: Domains of a level are numbered in deck order (MeshS.Domain[nl][nd])."""
        seen, out = {}, []
        for g in self.lev:
            l = g.cfg.level
            out.append((l, seen.get(l, 0))); seen[l] = seen.get(l, 0) + 1
        return out

    def write_dump(self, rundir: str, basename: str, num: int, fmt, prim: bool, level: int = -1, domain: int = -1,
                   time: float | None = None, dt: float | None = None):
        """dump_vtk / dump_binary over the Mesh: one file per Domain (level / domain = -1: all), named by ath_fname;
        -> the relative paths written.  Every level carries the Mesh's time and dt (or the ones given: a driver that
        keeps them itself, driver.MeshDriver)."""
        from . import dumps
        ext = {dumps.VTK: "vtk", dumps.BIN: "bin"}[dumps.FORMATS.get(fmt, fmt)]
        t, dt_, n = self.state()
        t = t if time is None else time; dt = dt_ if dt is None else dt
        out = []
        for g, (l, d) in zip(self.lev, self.domain_numbers()):
            if (level == -1 or level == l) and (domain == -1 or domain == d):
                rel = dumps.fname(basename, l, d, num, ext)
                g.write_dump(os.path.join(rundir, rel), fmt, prim, level=l, domain=d, time=t, dt=dt)
                out.append(rel)
        return out

    def halo_counts(self):
        """(pack + unpack launches, copies, exchanges) of the all-level x3 exchanges of a cut Mesh so far"""
        c = (C.c_longlong * 3)(); self._chk(self.L.aa_mesh_halo_counts(self._h, c)); return int(c[0]), int(c[1]), int(c[2])

    def step(self):
        it = (C.c_int * len(self.lev))()
        self._chk(self.L.aa_mesh_step(self._h, it))
        return list(it)

    def run_2d_batch(self) -> int:
        """steps run_2d queues per read-back on this Mesh (AA_2D_BATCH when the Mesh was made, else the Mesh's own default; 0: it
        steps one at a time)"""
        return int(self.L.aa_mesh_run_2d_batch(self._h))

    def can_run_2d(self) -> bool:
        """whether run_2d queues steps on this Mesh: every level 2-D, not cut into slabs, not a rank's stack (links), no level with
        pinned zones -- the refusals of aa_mesh_run_2d -- and a batch above 0"""
        return (all(g.ndim == 2 for g in self.lev) and self.cuts is None and self.links is None
                and all(g.npin == 0 for g in self.lev) and self.run_2d_batch() > 0)

    def run_2d(self, t_stop: float, tlim: float | None = None, nstep_stop: int | None = None) -> int:
        """Whole passes of step()'s loop on a Mesh of 2-D Grids with ONE clock on the device for all levels (aa_mesh_run_2d):
        AA_2D_BATCH steps are queued per read-back; until time >= t_stop, nstep == nstep_stop or dt <= 0; new_dt clips at tlim
        (default: the deck's).  nstep_stop None: 2^20 steps ahead at the most.  Returns the steps taken; the same bits as that many
        step() calls.  AthenaError on a Mesh of 3-D Grids, one cut into slabs or made from links, a level with pinned zones."""
        n = C.c_int()
        tlim = self.lev[0].cfg.run.tlim if tlim is None else tlim
        stop = self.nstep + (1 << 20) if nstep_stop is None else int(nstep_stop)
        self._chk(self.L.aa_mesh_run_2d(self._h, float(t_stop), float(tlim), stop, C.byref(n)))
        return n.value

    def run_3d_batch(self) -> int:
        """steps run_3d queues per read-back on this Mesh (AA_3D_BATCH when the Mesh was made, else the Mesh's own default); 0: it
        steps one at a time -- the knob at 0, or a level off the chain whose kernels read the device clock (van Leer, cooling, ion
        radiation, the tile kernels of a small level, ...: include/athena_amd.h)"""
        return int(self.L.aa_mesh_run_3d_batch(self._h))

    def can_run_3d(self) -> bool:
        """whether run_3d queues steps on this Mesh: every level 3-D, not cut into slabs, not a rank's stack (links), no level with
        pinned zones -- the refusals of aa_mesh_run_3d -- and a batch above 0"""
        return (all(g.ndim == 3 for g in self.lev) and self.cuts is None and self.links is None
                and all(g.npin == 0 for g in self.lev) and self.run_3d_batch() > 0)

    def run_3d(self, t_stop: float, tlim: float | None = None, nstep_stop: int | None = None) -> int:
        """Whole passes of step()'s loop on a Mesh of 3-D Grids with the time step picked on the device for all levels
        (aa_mesh_run_3d): AA_3D_BATCH steps are queued per read-back; until time >= t_stop, nstep == nstep_stop or dt <= 0; new_dt
        clips at tlim (default: the deck's).  nstep_stop None: 2^20 steps ahead at the most.  Returns the steps taken; the same
        bits as that many step() calls (a Mesh whose batch is 0 takes them one at a time inside the call).  AthenaError on a Mesh
        of 2-D Grids, one cut into slabs or made from links, a level with pinned zones."""
        n = C.c_int()
        tlim = self.lev[0].cfg.run.tlim if tlim is None else tlim
        stop = self.nstep + (1 << 20) if nstep_stop is None else int(nstep_stop)
        self._chk(self.L.aa_mesh_run_3d(self._h, float(t_stop), float(tlim), stop, C.byref(n)))
        return n.value

    def run_hst_arm(self, t_next: float, dt_out: float, nlim: int | None = None) -> None:
        """Grid.run_hst_arm for the next run_2d / run_3d call of this Mesh (aa_mesh_run_hst_arm): ONE schedule for all levels, a
        row of every Grid where one is due.  AthenaError on a Mesh cut into slabs or made from links."""
        self._chk(self.L.aa_mesh_run_hst_arm(self._h, float(t_next), float(dt_out), -1 if nlim is None else int(nlim)))

    def run_hst_rows(self):
        """-> ([rows of Grid 0, rows of Grid 1, ...], t_next) of the last armed run call (aa_mesh_run_hst_rows): every Grid's
        rows[n][11] = time, dt and the nine sums of its history(), the same n for all"""
        out, t = [], C.c_double()
        for l in range(len(self.lev)):
            n = C.c_int()
            self._chk(self.L.aa_mesh_run_hst_rows(self._h, l, 0, None, C.byref(n), C.byref(t)))
            rows = np.zeros((n.value, HST_ROW))
            if n.value:
                self._chk(self.L.aa_mesh_run_hst_rows(self._h, l, n.value, _dp(rows), C.byref(n), C.byref(t)))
            out.append(rows)
        return out, t.value
