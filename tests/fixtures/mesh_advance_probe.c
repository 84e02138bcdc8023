/* csrc/time_step.h run_advance_levels -- the arithmetic of k2d_mesh_advance (aa_mesh_run_2d) -- through a plain function
 * (tests/test_run_2d_mesh_host.py compiles this with the host compilers, as C99 and as C++; no device).
 * clock: dt, time in and out; ints: live, nstep in and out.  max_v and dx hold ndir doubles per Grid. */
#include "time_step.h"

#ifdef __cplusplus
extern "C" {
#endif

void probe_advance_levels(double *clock, int *ints, double t_stop, double tlim, double cour_no, int nstep_stop,
                          int ngrid, int ndir, const double *max_v, const double *dx)
{
  RunClock c;
  c.dt = clock[0]; c.time = clock[1]; c.live = ints[0]; c.nstep = ints[1];
  run_advance_levels(&c, t_stop, tlim, cour_no, nstep_stop, ngrid, ndir, max_v, dx);
  clock[0] = c.dt; clock[1] = c.time; ints[0] = c.live; ints[1] = c.nstep;
}

#ifdef __cplusplus
}
#endif
