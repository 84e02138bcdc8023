// hydro3d_clock.hip -- the kernels that write the device clock of aa_run_3d (hydro3d_launch.h Run3D: k3d_seed, k3d_advance) and the
// clocks of the Grids of a Mesh in aa_mesh_run_3d (k3d_mesh_seed, k3d_mesh_advance).  The kernels of the step that read them are the
// *_dc entries of hydro_kernels.hip and smr.hip; csrc/run.hip and csrc/smr.hip queue both.
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

// ---- the Grids of a 3-D Mesh on one clock (aa_mesh_run_3d, csrc/smr.hip) ----------------------------------------------------------
// The clocks of a call: lane l writes the Run3D of Grid l -- the call's clock and limits, the ratios of the Grid's own dx -- and
// zeroes the Grid's maxima for the first step.
__global__ void __launch_bounds__(64)
k3d_mesh_seed(Run3D *rc, Run3D v, MeshClockTab3 tab)
{
  const int l = threadIdx.x;
  if (l >= tab.n) return;
  rc[l] = v;
  run_step_ratios(v.c.dt, tab.dx + 3*l, rc[l].dtodx, rc[l].q);
  DevScalars *sc = tab.sc[l];
  sc->max_v[0] = 0ULL; sc->max_v[1] = 0ULL; sc->max_v[2] = 0ULL;
}
// One wavefront behind the level coupling of every queued step: what aa_mesh_step does on the host between RestrictCorrect and
// bvals_mhd (main.c:618-629; smr.hip aa_mesh_step, aa_mesh_new_dt) -- the arithmetic is time_step.h run_advance_levels with three
// directions, the maxima are those the update kernels (Grids without children) and k_cfl (Grids with children) left in every
// Grid's DevScalars.  Lane l reads and zeroes the maxima of Grid l, lane 0 advances the clock, and lane l then writes the clock and
// the ratios of the new dt over its Grid's own dx into the Run3D of Grid l: dt_over_dx / half_dt_over_dx, so they are the bits
// step_ratios() forms on the host for that Grid.  `stepped` tells the kernels queued behind this one whether the step in front of
// it was taken (k_box_copy_dc).  Launch rule as k3d_advance: a plain launch in stream order, no waiting; the barriers are reached
// by the whole workgroup (the early return is uniform).
__global__ void __launch_bounds__(64)
k3d_mesh_advance(Run3D *rc, MeshClockTab3 tab, RunClock *out)
{
  __shared__ Real mv[3*AA_3D_MESH_GRIDS], dx[3*AA_3D_MESH_GRIDS];
  __shared__ RunClock next;
  const int l = threadIdx.x, live = rc[0].c.live;
  if (!live) { if (l < tab.n) rc[l].stepped = 0; return; }
  if (l < tab.n) {
    DevScalars *sc = tab.sc[l];
    for (int d = 0; d < 3; d++) { mv[3*l + d] = __longlong_as_double((long long)sc->max_v[d]); dx[3*l + d] = tab.dx[3*l + d]; }
    sc->max_v[0] = 0ULL; sc->max_v[1] = 0ULL; sc->max_v[2] = 0ULL;                              // for the next step
  }
  __syncthreads();
  if (l == 0) {
    RunClock c = rc[0].c;
    run_advance_levels(&c, rc[0].t_stop, rc[0].tlim, rc[0].cour_no, rc[0].nstep_stop, tab.n, 3, mv, dx);
    next = c; *out = c;
  }
  __syncthreads();
  if (l >= tab.n) return;
  const RunClock c = next;
  run_step_ratios(c.dt, dx + 3*l, rc[l].dtodx, rc[l].q);
  rc[l].c = c; rc[l].stepped = 1;
}

void launch_3d_seed(const DevGrid &g, Run3D *rc, const Run3D &v, DevScalars *sc, hipStream_t st)
{ hipLaunchKernelGGL(k3d_seed, dim3(1), dim3(64), 0, st, rc, v, sc, g.dx[0], g.dx[1], g.dx[2]); }
void launch_3d_advance(const DevGrid &g, Run3D *rc, DevScalars *sc, RunClock *out, hipStream_t st)
{ hipLaunchKernelGGL(k3d_advance, dim3(1), dim3(64), 0, st, rc, sc, g.dx[0], g.dx[1], g.dx[2], out); }

void launch_3d_mesh_seed(Run3D *rc, const Run3D &v, const MeshClockTab3 &tab, hipStream_t st)
{ hipLaunchKernelGGL(k3d_mesh_seed, dim3(1), dim3(64), 0, st, rc, v, tab); }
void launch_3d_mesh_advance(Run3D *rc, const MeshClockTab3 &tab, RunClock *out, hipStream_t st)
{ hipLaunchKernelGGL(k3d_mesh_advance, dim3(1), dim3(64), 0, st, rc, tab, out); }

}  // namespace aa
