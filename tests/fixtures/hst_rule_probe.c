/* csrc/time_step.h hst_row_due as the host compilers build it (C99 and C++), for tests/test_hst_run_host.py */
#include "time_step.h"

#ifdef __cplusplus
extern "C" {
#endif

int probe_hst_row_due(double time, int nstep, double tlim, int nlim, double dt_out, double *t_next)
{
  return hst_row_due(time, nstep, tlim, nlim, dt_out, t_next);
}

/* the block's next time after `n` steps that all have a row due (time far ahead of it); *fired: the rows */
double probe_hst_many(double t_next, double dt_out, int n, int *fired)
{
  int k;
  *fired = 0;
  for (k = 0; k < n; k++) *fired += hst_row_due(1.0e300, k + 1, 2.0e300, -1, dt_out, &t_next);
  return t_next;
}

int probe_hst_sched_bytes(void) { return (int)sizeof(HstSched); }

#ifdef __cplusplus
}
#endif
