/* ion_stop_rule of csrc/ion_subcycle.h -- the one function the host's loop (ion_subcycles) and the device's queued pick share -- under a
 * loop of this file's own (tests/test_ion_stop_rule.py compiles this with the host compiler).  The loop is the device's, not
 * ion_subcycles: per sub-cycle the negative-dt_chem exit in front of everything, the pick (ion_pick_step), the booking of the applied
 * step, the rule -- so the rule is held to the table on its own, whoever calls it.
 * rows: n sub-cycles x (dt_chem, dt_therm, cellcount, dt_hydro, negative-dt_chem flag).  A level enters with dt_in (the root: also
 * its limit) under tcoarse_in; out: niter, the level's dt, tcoarse, dt_done, the stop code, the steps applied (n doubles) and what
 * ion_close_root said (root only).  Returns 0, -4 where a flagged sub-cycle was met, -100 where the script ran out with the loop open. */
#include "ion_subcycle.h"

extern "C" int probe_ion_stop_rule(int fine, int hit, long long cellcount, double dt_hydro, double dt_done)
{ return ion_stop_rule(fine, hit, cellcount, dt_hydro, dt_done); }

extern "C" int probe_ion_stop_loop(int fine, double limit, int maxiter, double dt_in, double tcoarse_in, int n, const double *rows,
                                   int *niter, double *dt_out, double *tcoarse_out, double *dt_done_out, int *stop_out, double *steps, int *rc_close)
{
  double dt_done = 0.0;
  int k = 0, stop = ION_GO_ON;
  while (stop == ION_GO_ON) {
    if (k >= n) return -100;
    const double *s = rows + 5*k;
    if (s[4] != 0.0) { stop = ION_STOP_NEG; break; }
    int hit;
    const double dt = ion_pick_step(s[0], s[1], dt_done, limit, &hit);
    steps[k++] = dt;
    dt_done += dt;
    stop = ion_stop_rule(fine, hit, (long long)s[2], s[3], dt_done);
  }
  double dt = dt_in, tcoarse = tcoarse_in;
  if (stop == ION_STOP_CUT) dt = dt_done;
  *rc_close = 0;
  if (stop != ION_STOP_NEG && !fine) *rc_close = ion_close_root(k, maxiter, dt_done, &dt, &tcoarse);
  *niter = k; *dt_out = dt; *tcoarse_out = tcoarse; *dt_done_out = dt_done; *stop_out = stop;
  return stop == ION_STOP_NEG ? -4 : 0;
}
