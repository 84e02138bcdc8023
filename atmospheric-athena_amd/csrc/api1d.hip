// api1d.hip -- the C-ABI of a 1-D Grid's integrators (include/athena_amd.h: aa_integrate_1d_ctu, aa_integrate_1d_vl; aa_run_1d is run.hip):
// the kernels of csrc/hydro1d_kernels.hip.  Everything else a 1-D Grid needs (creation, transfers, bvals_mhd, new_dt, aa_start /
// aa_step) is the code of api.hip, which branches on aa_grid::one_d where a 1-D Grid differs.  (The stage names below are not in
// bench.py's table of bytes per stage: the benchmark has no 1-D workload; profiles/rate_1d.py measures whole runs.)
#include <hip/hip_runtime.h>
#include <string.h>
#include <utility>
#include "api_internal.h"

using namespace aa;

extern "C" {

int aa_step_1d_block(void) { return step1d_block(); }

// one launch: k1d_step reads U and writes the second buffer, which is U from here on (hydro1d_kernels.hip, header)
static int integrate_1d(aa_grid *g, bool vl)
{
  g->active_dirty = true;
  // new_dt's maximum rides on the step (aa_cfl_in_update) unless zones are pinned: those are rewritten behind it
  g->cfl_ready = g->cfl_in_update && g->npin == 0;
  if (g->cfl_ready) HIPCHK(hipMemsetAsync(g->sc->max_v, 0, 3*sizeof(unsigned long long), g->st));
  { Scope s(g, vl ? "vl1d_step" : "ctu1d_step");
    launch_1d_step(g->d, vl, g->p.order == 3, g->dt, g->d.LR, g->cfl_ready ? g->sc : nullptr, g->st); }
  std::swap(g->d.U, g->d.LR);
  HIPCHK(hipGetLastError());
  return 0;
}
int aa_integrate_1d_ctu(aa_grid *g)
{
  if (!g) return aa_fail(-1, "[aa_integrate_1d_ctu]: null argument");
  if (!g->one_d) return aa_fail(-1, "[aa_integrate_1d_ctu]: this is a %s Grid: aa_integrate_%s_ctu", g->two_d ? "2-D" : "3-D", g->two_d ? "2d" : "3d");
  if (g->p.integrator == 1) return aa_fail(-1, "[aa_integrate_1d_ctu]: this Grid was created for the van Leer integrator");
  return integrate_1d(g, false);      // (integrators 0 and 2: integrate_1d_ctu.c has no H-correction)
}
int aa_integrate_1d_vl(aa_grid *g)
{
  if (!g) return aa_fail(-1, "[aa_integrate_1d_vl]: null argument");
  if (!g->one_d) return aa_fail(-1, "[aa_integrate_1d_vl]: this is a %s Grid: aa_integrate_%s_vl", g->two_d ? "2-D" : "3-D", g->two_d ? "2d" : "3d");
  if (g->p.integrator != 1) return aa_fail(-1, "[aa_integrate_1d_vl]: this Grid was created for the CTU integrator (its cour_no was checked for that one)");
  return integrate_1d(g, true);
}

}  // extern "C"
