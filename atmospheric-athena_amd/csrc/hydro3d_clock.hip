// hydro3d_clock.hip -- the two kernels that write the device clock of aa_run_3d (hydro3d_launch.h Run3D).  The kernels of the step
// that read it are the *_dc entries of hydro_kernels.hip; csrc/run.hip queues both.
#include "hydro3d_launch.h"

namespace aa {

// (the six StepRatios of a dt are the bits step_ratios() forms on the host: one thread, nothing contracted -- time_step.h run_step_ratios)
// the clock of a call: what aa_run_3d knows on the host, the ratios of its dt, and the maxima zeroed for the first step's update kernel
__global__ void __launch_bounds__(64)
k3d_seed(Run3D *rc, Run3D v, DevScalars *sc, Real dx0, Real dx1, Real dx2)
{
  if (threadIdx.x != 0) return;
  const Real dx[3] = {dx0, dx1, dx2};
  *rc = v;
  run_step_ratios(v.c.dt, dx, rc->dtodx, rc->q);
  sc->max_v[0] = 0ULL; sc->max_v[1] = 0ULL; sc->max_v[2] = 0ULL;
}
// One wavefront behind the boundary pass of every queued step: what aa_step does on the host behind the integrator (main.c:618-629;
// api.hip aa_step, aa_new_dt_local, aa_new_dt), with the same operations in the same order, none contracted (time_step.h
// run_advance_grid), then the ratios of the new dt for the next step's kernels.  Zeroing the maxima here replaces cfl_arm's
// memset.  Launch rule (as k1d_run and k2d_advance state it for themselves): a plain launch in stream order; nothing here waits
// for another workgroup or spins on memory, so the launch ends whatever the data are.
__global__ void __launch_bounds__(64)
k3d_advance(Run3D *rc, DevScalars *sc, Real dx0, Real dx1, Real dx2, RunClock *out)
{
  if (threadIdx.x != 0 || !rc->c.live) return;
  RunClock c = rc->c;
  const Real dx[3] = {dx0, dx1, dx2};
  const Real max_v[3] = {__longlong_as_double((long long)sc->max_v[0]), __longlong_as_double((long long)sc->max_v[1]),
                         __longlong_as_double((long long)sc->max_v[2])};
  run_advance_grid(&c, rc->t_stop, rc->tlim, rc->cour_no, rc->nstep_stop, 3, max_v, dx);       // new_dt.c:156-185; a NaN dt stops too
  sc->max_v[0] = 0ULL; sc->max_v[1] = 0ULL; sc->max_v[2] = 0ULL;                               // for the next step's update kernel
  run_step_ratios(c.dt, dx, rc->dtodx, rc->q);
  rc->c = c; *out = c;
}

void launch_3d_seed(const DevGrid &g, Run3D *rc, const Run3D &v, DevScalars *sc, hipStream_t st)
{ hipLaunchKernelGGL(k3d_seed, dim3(1), dim3(64), 0, st, rc, v, sc, g.dx[0], g.dx[1], g.dx[2]); }
void launch_3d_advance(const DevGrid &g, Run3D *rc, DevScalars *sc, RunClock *out, hipStream_t st)
{ hipLaunchKernelGGL(k3d_advance, dim3(1), dim3(64), 0, st, rc, sc, g.dx[0], g.dx[1], g.dx[2], out); }

}  // namespace aa
