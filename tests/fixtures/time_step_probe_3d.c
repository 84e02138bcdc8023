/* The host side of aa_run_3d's device clock: csrc/time_step.h run_advance_grid and run_step_ratios, which k3d_advance and k3d_seed
 * (csrc/hydro_kernels.hip) call on the device, through plain functions (tests/test_time_step_3d.py compiles this with the host
 * compilers, as C++ and as C99, like time_step_probe.c). */
#include "time_step.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one pass of k3d_advance's arithmetic on the clock (time, dt, nstep); out: time, dt; returns nstep*2 + live */
int probe_advance_grid(double time, double dt, int nstep, double t_stop, double tlim, double cour_no, int nstep_stop,
                       int ndir, const double *max_v, const double *dx, double *out)
{
  RunClock c;
  c.dt = dt; c.live = 1; c.nstep = nstep; c.time = time;
  run_advance_grid(&c, t_stop, tlim, cour_no, nstep_stop, ndir, max_v, dx);
  out[0] = c.time; out[1] = c.dt;
  return c.nstep*2 + c.live;
}

/* out: dt/dx_1..3, then 0.5*(dt/dx_1..3) */
void probe_step_ratios(double dt, const double *dx, double *out) { run_step_ratios(dt, dx, out, out + 3); }

double probe_dt_over_dx(double dt, double dx) { return dt_over_dx(dt, dx); }
double probe_half_dt_over_dx(double dt, double dx) { return half_dt_over_dx(dt, dx); }

#ifdef __cplusplus
}
#endif
