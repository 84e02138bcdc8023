// api2d.hip -- the C-ABI of a 2-D Grid's integrators (include/athena_amd.h: aa_integrate_2d_ctu, aa_integrate_2d_vl, aa_run_2d): the kernel
// chains of csrc/hydro2d_kernels.hip in the order of integrate_2d_ctu.c / integrate_2d_vl.c.  Everything else a 2-D Grid needs
// (creation, transfers, bvals_mhd, new_dt, aa_start / aa_step, outputs) is the code of api.hip, dump.hip and restart.hip, which
// branch on aa_grid::two_d where a 2-D Grid differs.  (The stage names below are not in bench.py's table of bytes per stage:
// the benchmark has no 2-D workload; profiles/rate_2d.py reads them.)
#include <hip/hip_runtime.h>
#include <string.h>
#include "api_internal.h"

using namespace aa;

extern "C" {

// ---- the 2-D integrators (hydro2d_kernels.hip): integrate_2d_ctu.c / integrate_2d_vl.c for a Grid with Nx3 = 1 ----------------
// new_dt's maxima ride on the update kernel (aa_cfl_in_update) unless zones are pinned: those are rewritten behind it
static void cfl_arm_2d(aa_grid *g)
{
  g->cfl_ready = g->cfl_in_update && g->npin == 0;
  if (g->cfl_ready) (void)hipMemsetAsync(g->sc->max_v, 0, 3*sizeof(unsigned long long), g->st);
}
int aa_integrate_2d_ctu(aa_grid *g)
{
  if (!g) return aa_fail(-1, "[aa_integrate_2d_ctu]: null argument");
  if (g->one_d) return aa_fail(-1, "[aa_integrate_2d_ctu]: this is a 1-D Grid (Nx2 = Nx3 = 1): aa_integrate_1d_ctu");
  if (!g->two_d) return aa_fail(-1, "[aa_integrate_2d_ctu]: this is a 3-D Grid: aa_integrate_3d_ctu");
  if (g->p.integrator == 1) return aa_fail(-1, "[aa_integrate_2d_ctu]: this Grid was created for the van Leer integrator");
  g->cfl_ready = false; g->active_dirty = true;
  const HostGrid &d = g->d; const Real dt = g->dt;
  { Scope s(g, "ctu2d_first"); launch_2d_ctu_first(d, dt, g->edge2d, g->st); }
  // (integrator 2: a reference built without --enable-h-correction has no eta arrays: etah = 0 in every flux)
  { Scope s(g, "ctu2d_correct"); launch_2d_ctu_correct(d, dt, g->p.integrator == 0, g->st); }
  { Scope s(g, "ctu2d_flux2_update");
    cfl_arm_2d(g);
    // (a level of a Mesh: the instantiation that also leaves the second-pass fluxes on the level-boundary lines in F)
    if (g->keep_flux) launch_2d_ctu_flux2_update_keep(d, dt, g->edge2d, g->cfl_ready ? g->sc : nullptr, g->keep, g->st);
    else launch_2d_ctu_flux2_update(d, dt, g->edge2d, g->cfl_ready ? g->sc : nullptr, g->st); }
  HIPCHK(hipGetLastError());
  return 0;
}
int aa_integrate_2d_vl(aa_grid *g)
{
  if (!g) return aa_fail(-1, "[aa_integrate_2d_vl]: null argument");
  if (g->one_d) return aa_fail(-1, "[aa_integrate_2d_vl]: this is a 1-D Grid (Nx2 = Nx3 = 1): aa_integrate_1d_vl");
  if (!g->two_d) return aa_fail(-1, "[aa_integrate_2d_vl]: this is a 3-D Grid: aa_integrate_3d_vl");
  if (g->p.integrator != 1) return aa_fail(-1, "[aa_integrate_2d_vl]: this Grid was created for the CTU integrator (its cour_no was checked for that one)");
  g->cfl_ready = false; g->active_dirty = true;
  const HostGrid &d = g->d; const Real dt = g->dt;
  { Scope s(g, "vl2d_predict"); launch_2d_vl_predict(d, dt, g->edge2d, g->st); }
  { Scope s(g, "vl2d_flux2_update");
    cfl_arm_2d(g);
    if (g->keep_flux) launch_2d_vl_flux2_update_keep(d, dt, g->edge2d, g->cfl_ready ? g->sc : nullptr, g->keep, g->st);
    else launch_2d_vl_flux2_update(d, dt, g->edge2d, g->cfl_ready ? g->sc : nullptr, g->st); }
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- many steps per host visit: the time step picked on the device (hydro2d_kernels.hip k2d_advance) ---------------------------
// the clock in device memory and its page-locked mirror, made by the first call
static int run2d_buffers(aa_grid *g)
{
  if (g->run2d_dev) return 0;
  Run2DMirror *h = nullptr, *hm = nullptr; Run2D *d = nullptr;
  if (hipHostMalloc(&h, sizeof(Run2DMirror), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&hm, h, 0) != hipSuccess || hipMalloc(&d, sizeof(Run2D)) != hipSuccess) {
    if (h) hipHostFree(h);
    (void)hipGetLastError();
    return aa_fail(-2, "[aa_run_2d]: clock buffers");
  }
  memset(h, 0, sizeof(Run2DMirror));
  g->run2d = h; g->run2d_map = hm; g->run2d_dev = d;
  return 0;
}
// one step of the queue: the integrator's chain with new_dt's maxima on board, k2d_advance, bvals_mhd (main.c:572-644 without
// Userwork_in_loop: a Grid with pinned zones is refused).  The stage names are those of aa_integrate_2d_* / aa_bvals_mhd.
static void queue_step_2d(aa_grid *g)
{
  const HostGrid &d = g->d; const Run2D *rc = g->run2d_dev;
  if (g->p.integrator == 1) {
    { Scope s(g, "vl2d_predict"); launch_2d_vl_predict_dc(d, rc, g->edge2d, g->st); }
    { Scope s(g, "vl2d_flux2_update"); launch_2d_vl_flux2_update_dc(d, rc, g->edge2d, g->sc, g->st); }
  } else {
    { Scope s(g, "ctu2d_first"); launch_2d_ctu_first_dc(d, rc, g->edge2d, g->st); }
    { Scope s(g, "ctu2d_correct"); launch_2d_ctu_correct_dc(d, rc, g->p.integrator == 0, g->st); }
    { Scope s(g, "ctu2d_flux2_update"); launch_2d_ctu_flux2_update_dc(d, rc, g->edge2d, g->sc, g->st); }
  }
  { Scope s(g, "run2d_advance"); launch_2d_advance(d, g->run2d_dev, g->sc, g->run2d_map, g->st); }
  // The boundary kernels (k_bc) take no dt and are not predicated.  With four or more zones per direction every ghost zone is a
  // copy of an ACTIVE zone (x1 pass) or of a row whose x1 ghost zones that pass has just filled (x2 pass), so behind a stopped
  // step -- U untouched -- they write again what is there: idempotent.  (Grids with fewer zones step one at a time, below.)
  { Scope s(g, "bvals_mhd");
    for (int a = 0; a < 2; a++) launch_bc_dir(d, g->p.nscal, a, g->p.bc[2*a], g->p.bc[2*a + 1], g->st); }
}
int aa_run_2d_batch(const aa_grid *g) { return g && g->two_d ? g->batch_2d : 0; }
// main.c:519-669 until time >= t_stop, nstep == nstep_stop or dt <= 0: AA_2D_BATCH steps queued per read of the clock, or step
// by step (AA_2D_BATCH=0)
int aa_run_2d(aa_grid *g, double t_stop, double tlim, int nstep_stop, int *nsteps_done)
{
  if (!g) return aa_fail(-1, "[aa_run_2d]: null argument");
  if (g->one_d) return aa_fail(-1, "[aa_run_2d]: this is a 1-D Grid (Nx2 = Nx3 = 1): aa_run_1d");
  if (!g->two_d) return aa_fail(-1, "[aa_run_2d]: this is a 3-D Grid: only 1-D and 2-D Grids run many steps per host visit");
  if (g->npin > 0) return aa_fail(-1, "[aa_run_2d]: a 2-D Grid with pinned zones steps one at a time: aa_step");
  if (g->keep_flux || g->level > 0)
    return aa_fail(-1, "[aa_run_2d]: this Grid is a level of a Mesh (level %d): the levels step together, aa_mesh_step", g->level);
  const long long span = (long long)nstep_stop - g->nstep;
  if (span < 0 || span > (1LL << 20))
    return aa_fail(-1, "[aa_run_2d]: nstep_stop=%d from nstep=%d: a call covers 0 .. 2^20 steps", nstep_stop, g->nstep);
  if (tlim != g->p.tlim) return aa_fail(-1, "[aa_run_2d]: tlim=%.17g, but the Grid was created with %.17g (new_dt clips at that one)", tlim, g->p.tlim);
  const int nstep0 = g->nstep;
  // (fewer zones than ghost zones along a direction: a boundary kernel reads ghost zones there, see queue_step_2d)
  if (g->batch_2d == 0 || g->d.Nx1 < AA_NGHOST || g->d.Nx2 < AA_NGHOST) {
    while (g->time < t_stop && g->nstep != nstep_stop && g->dt > 0.0) { int rc = aa_step(g, nullptr); if (rc) return rc; }
    if (nsteps_done) *nsteps_done = g->nstep - nstep0;
    return 0;
  }
  if (nsteps_done) *nsteps_done = 0;
  if (!(g->time < t_stop && g->nstep != nstep_stop && g->dt > 0.0)) return 0;
  if (int rc = run2d_buffers(g)) return rc;
  g->cfl_ready = false; g->active_dirty = true;
  Run2D seed;
  seed.dt = g->dt; seed.live = 1; seed.nstep = g->nstep; seed.time = g->time;
  seed.t_stop = t_stop; seed.tlim = tlim; seed.cour_no = g->p.cour_no; seed.nstep_stop = nstep_stop; seed.pad = 0;
  launch_2d_seed(g->run2d_dev, seed, g->sc, g->st);
  // every launch ends whatever the data are, so the queue drains; a step behind the stop costs its launches and nothing else
  // (up to AA_2D_BATCH - 1 of them per call)
  for (;;) {
    for (int k = 0; k < g->batch_2d; k++) queue_step_2d(g);
    HIPCHK(hipGetLastError());
    g->host_syncs++;
    HIPCHK(hipStreamSynchronize(g->st));
    if (!g->run2d->live) break;
  }
  g->time = g->run2d->time; g->dt = g->run2d->dt; g->nstep = g->run2d->nstep;
  if (nsteps_done) *nsteps_done = g->nstep - nstep0;
  return 0;
}

}  // extern "C"
