/* csrc/time_step.h through plain functions (tests/test_time_step.py compiles this with the host compilers: as C++ into a shared
 * object it calls through ctypes, and as C99, which is how host/athena_shim.c takes the header).
 * probe_fold_levels: nl levels x 3 maxima and 3 zone sizes, carried and folded as a Mesh's new_dt does; the others are the
 * header's functions one by one.  probe_two_halves is the MPI shim's order: the factor two, a MIN with what another rank found,
 * then the clip. */
#include "time_step.h"

#ifdef __cplusplus
extern "C" {
#endif

double probe_fold(double max_dti, const double *max_v, const double *dx, int ndir) { return dt_fold(max_dti, max_v, dx, ndir); }

double probe_fold_levels(int nl, const double *max_v, const double *dx, int ndir)
{
  double cum[3] = {0.0, 0.0, 0.0}, max_dti = 0.0;
  int l;
  for (l = 0; l < nl; l++) max_dti = dt_fold_level(max_dti, cum, max_v + 3*l, dx + 3*l, ndir);
  return max_dti;
}

double probe_courant(double cour_no, double max_dti) { return dt_courant(cour_no, max_dti); }
double probe_grow(int nstep, double dt, double dt_cfl) { return dt_grow(nstep, dt, dt_cfl); }
double probe_clip(double dt, double time, double tlim) { return dt_clip(dt, time, tlim); }
double probe_pick(int nstep, double dt, double dt_cfl, double time, double tlim) { return dt_pick(nstep, dt, dt_cfl, time, tlim); }

double probe_two_halves(int nstep, double dt, double dt_cfl, double other_rank, double time, double tlim)
{
  const double mine = dt_grow(nstep, dt, dt_cfl);
  return dt_clip((other_rank < mine) ? other_rank : mine, time, tlim);
}

int probe_live(double time, double t_stop, int nstep, int nstep_stop, double dt) { return run_live(time, t_stop, nstep, nstep_stop, dt); }

/* the clock the run calls share: dt and live in the first 16 bytes (the 2-D step kernels load the two at once) */
int probe_clock_layout(void)
{
  RunClock c;
  return sizeof c == 24 && (char*)&c.dt - (char*)&c == 0 && (char*)&c.live - (char*)&c == 8 && (char*)&c.nstep - (char*)&c == 12 &&
         (char*)&c.time - (char*)&c == 16;
}

#ifdef __cplusplus
}
#endif
