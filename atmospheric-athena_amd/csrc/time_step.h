/* time_step.h -- the time-step rule of new_dt.c:156-185 and the loop condition of main.c:519, once, for host and device
 * (C99 and C++, no HIP include; the drop-in shim, the C library, k1d_run, k2d_advance and k2d_mesh_advance all call these).
 *
 * However the maxima of |v| + a reach the caller -- one Grid, slabs, the levels of a Mesh, MPI ranks, a kernel that keeps the
 * clock on the device -- the operations, their order and their comparison forms are the ones written here:
 *   dt_fold        :156-161  max_dti = MAX(max_dti, max_v_d/dx_d) over the directions with more than one zone
 *   dt_carry       :33, :53  max_v1..3 are zeroed once, in front of the loop over Grids: a level's maxima include the coarser ones'
 *   dt_fold_level            the two of a level: carry, then fold
 *   dt_courant     :168      CourNo/max_dti (max_dti = 0: +inf)
 *   dt_grow        :167-171  nstep == 0 ? dt_cfl : MIN(2.0*dt, dt_cfl), MIN(a,b) = (a < b) ? a : b (defs.h.in:146): a NaN dt_cfl
 *                            gives NaN.  With MPI this half stands before the MPI_Allreduce(MIN) of :177 ...
 *   dt_clip        :183-185  ... and this half, the clip at tlim, behind it
 *   dt_pick        :167-185  the two composed
 *   run_live       main.c:519 as the run calls use it: time < t_stop && nstep != nstep_stop && dt > 0.0 (a NaN dt stops)
 *   hst_row_due    main.c:524, output.c:509-512: whether a history block fires behind a taken step, and its next time
 *   run_advance_levels        main.c:618-629 of a Mesh: nstep++, time += dt, the fold over its Grids, the pick, run_live
 *   dt_over_dx, half_dt_over_dx   the update kernels' dt/dx and 0.5*(dt/dx) as the host's launch wrappers form them
 * No operation is contracted with another (the pragma inside every body: a file-scope one would reach the including file).
 * (driver.py holds pick_dt / fold_levels for the Python drivers; tests/test_time_step.py runs one table of cases through both;
 * oracle/athena_oracle.c keeps its own text: it is what the library is tested against.)
 */
#ifndef AA_TIME_STEP_H
#define AA_TIME_STEP_H

#ifdef __HIPCC__
#define TS_FN static inline __host__ __device__
#else
#define TS_FN static inline
#endif
#ifdef __clang__
#define TS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TS_NO_CONTRACT
#endif

/* MeshS.time / dt / nstep while a run call (aa_run_1d, aa_run_2d) has the main loop on the device, and whether the loop goes on.
 * dt and live lead: every kernel of a queued 2-D step reads the two in one 16-byte uniform load (hydro2d_launch.h Run2D). */
typedef struct RunClock { double dt; int live, nstep; double time; } RunClock;

TS_FN double dt_fold(double max_dti, const double *max_v, const double *dx, int ndir)
{
  TS_NO_CONTRACT
  int d;
  for (d = 0; d < ndir; d++) { const double q = max_v[d]/dx[d]; max_dti = (max_dti > q) ? max_dti : q; }
  return max_dti;
}

TS_FN void dt_carry(double *cum, const double *max_v, int ndir)
{
  int d;
  for (d = 0; d < ndir; d++) cum[d] = (cum[d] > max_v[d]) ? cum[d] : max_v[d];
}

TS_FN double dt_fold_level(double max_dti, double *cum, const double *max_v, const double *dx, int ndir)
{
  dt_carry(cum, max_v, ndir);
  return dt_fold(max_dti, cum, dx, ndir);
}

TS_FN double dt_courant(double cour_no, double max_dti)
{
  TS_NO_CONTRACT
  return cour_no/max_dti;
}

TS_FN double dt_grow(int nstep, double dt, double dt_cfl)
{
  TS_NO_CONTRACT
  if (nstep == 0) return dt_cfl;
  return (2.0*dt < dt_cfl) ? 2.0*dt : dt_cfl;
}

TS_FN double dt_clip(double dt, double time, double tlim)
{
  TS_NO_CONTRACT
  if ((time < tlim) && ((tlim - time) < dt)) dt = tlim - time;
  return dt;
}

TS_FN double dt_pick(int nstep, double dt, double dt_cfl, double time, double tlim)
{
  return dt_clip(dt_grow(nstep, dt, dt_cfl), time, tlim);
}

TS_FN int run_live(double time, double t_stop, int nstep, int nstep_stop, double dt)
{
  return time < t_stop && nstep != nstep_stop && dt > 0.0;
}

/* The schedule of ONE <outputN> block with out_fmt = hst while a run call has it armed (aa_run_hst_arm): the block's next time
 * and spacing, the loop's nlim (-1: none), the rows made so far in the call, and the step number the schedule has looked at last
 * (a queued step behind the stop leaves the clock's nstep where it was: no step was taken, nothing is asked). */
typedef struct HstSched { double t_next, dt_out; int nlim, nrows, nstep_seen, pad; } HstSched;

/* data_output(&Mesh, 0) at the top of the pass that follows a taken step (main.c:524, output.c:509-512) for one block: whether its
 * row is due behind the step that left `time` and `nstep`, and *t_next advanced by dt_out ONCE if so.  The call is reached only
 * if the loop goes on (main.c:519): behind the step that ends it -- time >= tlim (a NaN time too), nstep at nlim -- no row is
 * due, the forced data_output(&Mesh, 1) behind the loop writes that one.  A step that merely ends a run CALL (t_stop < tlim, the
 * span of 2^20 steps) is not the end of the loop. */
TS_FN int hst_row_due(double time, int nstep, double tlim, int nlim, double dt_out, double *t_next)
{
  TS_NO_CONTRACT
  if (!(time < tlim) || (nlim >= 0 && nstep >= nlim)) return 0;
  if (!(time >= *t_next)) return 0;
  *t_next += dt_out;
  return 1;
}

/* dt/dx and dt/2dx of the update kernels as the launch wrappers evaluate them on the host for the kernels that take dt as an
 * argument: one IEEE division, one multiplication by 0.5, never contracted with anything around them -- so a kernel that keeps the
 * clock on the device (k2d_step_dc; k3d_seed / k3d_advance for the StepRatios of the 3-D kernels) forms the same bits. */
TS_FN double dt_over_dx(double dt, double dx)
{
  TS_NO_CONTRACT
  return dt/dx;
}
TS_FN double half_dt_over_dx(double dt, double dx)
{
  TS_NO_CONTRACT
  const double q = dt/dx;
  return 0.5*q;
}
/* ... the six of a 3-D step (hydro_kernels.hip StepRatios), for the clock of aa_run_3d */
TS_FN void run_step_ratios(double dt, const double *dx, double *dtodx, double *q)
{
  int d;
  for (d = 0; d < 3; d++) { dtodx[d] = dt_over_dx(dt, dx[d]); q[d] = half_dt_over_dx(dt, dx[d]); }
}

/* main.c:618-629 for ONE Grid whose loop is on the device (aa_run_3d; k3d_advance calls this, and aa_step + aa_new_dt_local +
 * aa_new_dt are the same operations on the host): nstep++, time += dt, the fold over the Grid's ndir directions, the pick with
 * the clip at tlim, and whether the call's loop goes on. */
TS_FN void run_advance_grid(RunClock *c, double t_stop, double tlim, double cour_no, int nstep_stop,
                            int ndir, const double *max_v, const double *dx)
{
  TS_NO_CONTRACT
  c->nstep++;
  c->time += c->dt;
  c->dt = dt_pick(c->nstep, c->dt, dt_courant(cour_no, dt_fold(0.0, max_v, dx, ndir)), c->time, tlim);
  c->live = run_live(c->time, t_stop, c->nstep, nstep_stop, c->dt);
}

/* main.c:618-629 for the Grids of a Mesh whose loop is on the device (aa_mesh_run_2d; k2d_mesh_advance calls this, and
 * aa_mesh_step + aa_mesh_new_dt are the same operations on the host): nstep++, time += dt, then new_dt.c:32 over the Grids in the
 * Mesh's order -- the maxima carried from Grid to Grid, every Grid's own dx, ndir directions -- the pick with the clip at tlim,
 * and whether the call's loop goes on.  max_v and dx hold ndir doubles per Grid. */
TS_FN void run_advance_levels(RunClock *c, double t_stop, double tlim, double cour_no, int nstep_stop,
                              int ngrid, int ndir, const double *max_v, const double *dx)
{
  TS_NO_CONTRACT
  double cum[3] = {0.0, 0.0, 0.0}, max_dti = 0.0;
  int l;
  c->nstep++;
  c->time += c->dt;
  for (l = 0; l < ngrid; l++) max_dti = dt_fold_level(max_dti, cum, max_v + ndir*l, dx + ndir*l, ndir);
  c->dt = dt_pick(c->nstep, c->dt, dt_courant(cour_no, max_dti), c->time, tlim);
  c->live = run_live(c->time, t_stop, c->nstep, nstep_stop, c->dt);
}

#endif
