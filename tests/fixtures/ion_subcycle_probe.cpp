/* csrc/ion_subcycle.h under a scripted callable (tests/test_ion_subcycles.py compiles this with the host compiler).
 * rows: n sub-cycles x (dt_chem, dt_therm, cellcount, dt_hydro, negative-dt_chem flag).  The callable picks its step with
 * ion_pick_step and hands back the row's stop operands; a flagged row makes it fail with -4, a call past the script with -100.
 * A level enters with dt_in (the root: also its limit) under tcoarse_in; out: niter, the level's dt, tcoarse, the steps applied
 * (n doubles) and what ion_close_root said (root only).  Returns the loop's rc.
 * -DPROBE_MAIN adds a main() that runs a few scripts (for a sanitizer run of the header on the host). */
#include "ion_subcycle.h"

extern "C" int probe_maxcellcount(void) { return AA_MAXCELLCOUNT; }

/* ion_pick_step alone: what the device's picks are held to (tests/test_gpu_ion_subcycles.py) */
extern "C" double probe_ion_pick_step(double dt_chem, double dt_therm, double dt_done, double limit, int *hit)
{ return ion_pick_step(dt_chem, dt_therm, dt_done, limit, hit); }

extern "C" int probe_ion_subcycles(int fine, double limit, int maxiter, double dt_in, double tcoarse_in, int n, const double *rows,
                                   int *niter, double *dt_out, double *tcoarse_out, double *steps, int *rc_close)
{
  int k = 0;
  const IonSubcycles r = ion_subcycles(fine != 0, [&](double dt_done, double *dt, int *hit, long long *cellcount, double *dt_hydro) -> int {
    if (k >= n) return -100;
    const double *s = rows + 5*k;
    if (s[4] != 0.0) return -4;
    *dt = ion_pick_step(s[0], s[1], dt_done, limit, hit);
    *cellcount = (long long)s[2]; *dt_hydro = s[3];
    steps[k++] = *dt;
    return 0;
  });
  double dt = dt_in, tcoarse = tcoarse_in;
  if (r.cut) dt = r.dt_done;
  *rc_close = 0;
  if (!r.rc && !fine) *rc_close = ion_close_root(r.niter, maxiter, r.dt_done, &dt, &tcoarse);
  *niter = r.niter; *dt_out = dt; *tcoarse_out = tcoarse;
  return r.rc;
}

#ifdef PROBE_MAIN
#include <stdio.h>
int main(void)
{
  const double inf = 1.0/0.0;
  const double a[] = {0.2, 4.0, 0, inf, 0,  4.0, 4.0, 21, inf, 0};                        /* cut by check_range on the covering sub-cycle */
  const double b[] = {0.2, 4.0, 1000, 0.0, 0,  4.0, 4.0, 1000, 0.0, 0};                   /* a refined level */
  const double c[] = {1.0, 2.0, 0, inf, 0,  -1.0, 2.0, 0, inf, 1};                        /* the callable fails */
  const double d[] = {1.0, 1.0, 0, inf, 0};                                               /* negative step handed in; then past the script */
  struct { int fine; double limit; int maxiter, n; const double *rows; } run[] = {
    {0, 0.9, 100, 2, a}, {1, 0.9, 2, 2, b}, {0, 8.0, 100, 2, c}, {0, -1.0, 100, 1, d}, {0, 8.0, 100, 1, d}};
  for (unsigned q = 0; q < sizeof run/sizeof run[0]; q++) {
    int niter = 0, rc_close = 0; double dt = 0, tc = 0, steps[2] = {0, 0};
    const int rc = probe_ion_subcycles(run[q].fine, run[q].limit, run[q].maxiter, run[q].fine ? 3.0 : run[q].limit, run[q].fine ? run[q].limit : 123.0,
                                       run[q].n, run[q].rows, &niter, &dt, &tc, steps, &rc_close);
    printf("script %u: rc %d close %d niter %d dt %a tcoarse %a steps %a %a\n", q, rc, rc_close, niter, dt, tc, steps[0], steps[1]);
  }
  return probe_maxcellcount() == 20 ? 0 : 1;
}
#endif
