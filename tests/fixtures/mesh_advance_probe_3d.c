/* csrc/time_step.h as k3d_mesh_advance (aa_mesh_run_3d) uses it -- run_advance_levels over the Grids of a Mesh with three
 * directions, then run_step_ratios of the new dt over every Grid's own dx -- through a plain function
 * (tests/test_time_step_3d_mesh.py compiles this with the host compilers, as C99 and as C++; no device).
 * clock: dt, time in and out; ints: live, nstep in and out.  max_v and dx hold three doubles per Grid; ratios takes six per Grid:
 * dt/dx_1..3, then 0.5*(dt/dx_1..3). */
#include "time_step.h"

#ifdef __cplusplus
extern "C" {
#endif

void probe_mesh_advance_3d(double *clock, int *ints, double t_stop, double tlim, double cour_no, int nstep_stop,
                           int ngrid, const double *max_v, const double *dx, double *ratios)
{
  RunClock c;
  int l;
  c.dt = clock[0]; c.time = clock[1]; c.live = ints[0]; c.nstep = ints[1];
  run_advance_levels(&c, t_stop, tlim, cour_no, nstep_stop, ngrid, 3, max_v, dx);
  for (l = 0; l < ngrid; l++) run_step_ratios(c.dt, dx + 3*l, ratios + 6*l, ratios + 6*l + 3);
  clock[0] = c.dt; clock[1] = c.time; ints[0] = c.live; ints[1] = c.nstep;
}

#ifdef __cplusplus
}
#endif
