// api2d.hip -- the C-ABI of a 2-D Grid's integrators (include/athena_amd.h: aa_integrate_2d_ctu, aa_integrate_2d_vl; aa_run_2d is run.hip): the kernel
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
  g->cfl_ready = false; g->active_dirty = true; g->stepped_2d = true;
  const HostGrid &d = g->d; const Real dt = g->dt;
  { Scope s(g, "ctu2d_first"); launch_2d_ctu_first(d, dt, g->edge2d, g->order_2d, g->st); }
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
  g->cfl_ready = false; g->active_dirty = true; g->stepped_2d = true;
  const HostGrid &d = g->d; const Real dt = g->dt;
  { Scope s(g, "vl2d_predict"); launch_2d_vl_predict(d, dt, g->edge2d, g->st); }
  { Scope s(g, "vl2d_flux2_update");
    cfl_arm_2d(g);
    if (g->keep_flux) launch_2d_vl_flux2_update_keep(d, dt, g->edge2d, g->cfl_ready ? g->sc : nullptr, g->keep, g->st);
    else launch_2d_vl_flux2_update(d, dt, g->edge2d, g->cfl_ready ? g->sc : nullptr, g->order_2d, g->st); }
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- third-order reconstruction, opt-in (include/athena_amd.h): the ORD = 3 instantiations of hydro2d_kernels.hip ---------------
// Accepted where a third-order reference build pins the behaviour (blast_ppm: CTU + H-correction; blast_vl_ppm: van Leer), refused
// elsewhere.  The direct form of the kernels reads the zones' neighbours from U (or U^{n+1/2}): no slope arrays, nothing to allocate.
int aa_set_order_2d(aa_grid *g, int order)
{
  if (!g) return aa_fail(-1, "[aa_set_order_2d]: null argument");
  if (!g->two_d) return aa_fail(-1, "[aa_set_order_2d]: this is a %s Grid: its reconstruction order is aa_params.order at aa_create", g->one_d ? "1-D" : "3-D");
  if (order != 2 && order != 3) return aa_fail(-1, "[aa_set_order_2d]: order %d (2: PLM, 3: PPM)", order);
  if (g->keep_flux) return aa_fail(-1, "[aa_set_order_2d]: this Grid belongs to a Mesh: set the order of every level before aa_mesh_create_2d");
  if (g->stepped_2d || g->nstep != 0) return aa_fail(-1, "[aa_set_order_2d]: this Grid has already stepped (nstep = %d): set the order behind aa_create, before aa_start / aa_resume", g->nstep);
  if (order == 3 && g->p.integrator == 2)
    return aa_fail(-1, "[aa_set_order_2d]: integrator = 2 (CTU without H-correction) at third order: no reference build pins it");
  g->order_2d = order;
  return 0;
}
int aa_get_order_2d(const aa_grid *g) { return !g ? 0 : (g->two_d ? g->order_2d : (g->p.order == 3 ? 3 : 2)); }

}  // extern "C"
