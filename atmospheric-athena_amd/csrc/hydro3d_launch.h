// hydro3d_launch.h -- the device clock of aa_run_3d and the launch interface of what reads and writes it: the *_dc entries of the
// default 3-D CTU chain (hydro_kernels.hip) and the clock's own two kernels (hydro3d_clock.hip).  Kept apart from grid.h and
// hydro_launch.h, as hydro2d_launch.h is: the chain that takes dt as a kernel argument (aa_step) is declared there.
#pragma once
#include "grid.h"
#include "time_step.h"
#include "field_offsets.h"      // field_offsets_fit: the Grids the marching kernels' 32-bit zone offsets reach (aa_create asks it)

// steps aa_run_3d queues between two reads of the clock where AA_3D_BATCH is not set (0: one aa_step at a time); DESIGN section 8
#define AA_3D_BATCH_DEFAULT 8
// ... and aa_mesh_run_3d on a Mesh of 3-D Grids (the Mesh's own default: the smallest K within the spread of the best one on two
// 128^3 levels, profiles/rate_3d_smr_run_result.json)
#define AA_3D_MESH_BATCH_DEFAULT 4
// Grids of a Mesh the argument table of k3d_mesh_seed / k3d_mesh_advance holds; a Mesh with more steps one aa_mesh_step at a time
#define AA_3D_MESH_GRIDS 16

namespace aa {

// The clock (time_step.h RunClock) of a 3-D Grid while aa_run_3d has steps queued, with the call's limits, in DEVICE memory -- the
// Run2D of hydro2d_launch.h with the six StepRatios of the step beside dt: the 3-D kernels keep dt/dx_d and half of it in scalar
// registers (hydro_kernels.hip StepRatios), so the *_dc entries fetch them by uniform loads instead of dividing per lane.  k3d_seed
// and k3d_advance form them once, in one thread, with the operations of step_ratios() (time_step.h dt_over_dx / half_dt_over_dx).
// live = 0: the call's stop rule has fired; what is queued behind it returns without a store.
struct Run3D {
  RunClock c;                       // dt and live lead: one 16-byte uniform load
  Real dtodx[3], q[3];              // of c.dt: dt/dx_d, 0.5*(dt/dx_d)
  Real t_stop, tlim, cour_no;       // of the call: main.c's loop condition, new_dt.c's clip and CourNo
  int nstep_stop;
  int stepped;                      // a Mesh's clocks only (k3d_mesh_advance): the step in front of that kernel was taken (smr.hip k_box_copy_dc)
};
// The Grids of a Mesh as k3d_mesh_seed / k3d_mesh_advance see them: new_dt's maxima and the zone sizes, in the Mesh's order.  The
// levels of a Mesh share time, dt, nstep and the stop rule but not dt/dx_d, and the 3-D kernels read the six ratios from the clock
// they are handed: every Grid of a Mesh has a Run3D of its own, Grid l the l-th of ONE device array, all with the same c, t_stop,
// tlim, cour_no and nstep_stop and each with the ratios of its own dx.  The *_dc entries and their argument stay what they are.
struct MeshClockTab3 { int n, pad; DevScalars *sc[AA_3D_MESH_GRIDS]; Real dx[3*AA_3D_MESH_GRIDS]; };
// hydro3d_clock.hip: the clock of a call (v.dtodx / v.q are formed by the kernel); new_dt's maxima zeroed
void launch_3d_seed(const DevGrid &g, Run3D *rc, const Run3D &v, DevScalars *sc, hipStream_t st);
// ... and nstep++, time += dt, new_dt with the clip at tlim, the maxima zeroed again, the next step's ratios, the stop rule; `out`: the host's mirror
void launch_3d_advance(const DevGrid &g, Run3D *rc, DevScalars *sc, RunClock *out, hipStream_t st);
// hydro_kernels.hip (namespace aa only: a Grid with a cooling function steps one aa_step at a time): the chain aa_integrate_3d_ctu
// launches by default, dt and the ratios from the clock, same launch geometry
void launch_sweep_x2_dc(const HostGrid &g, int nscal, const Run3D *rc, bool grav, hipStream_t st);       // as launch_sweep(.., 1, ..)
bool correct_all_dc_built(int nscal, bool grav);      // false: this build has no k_correct_all_dc for the combination (it would spill): aa_step
void launch_correct_all_dc(const HostGrid &g, int nscal, const Run3D *rc, bool grav, hipStream_t st);    // as launch_correct_all(.., x3f = true, ..): tile-edge x1 fluxes, k_correct_all, k_eta_edges
void launch_flux2_update_dc(const HostGrid &g, int nscal, const Run3D *rc, bool grav, DevScalars *sc, hipStream_t st);   // as launch_flux2_update(.., sc): always with new_dt's maxima
// ... of a level of a Mesh (aa_mesh_run_3d): as launch_flux2_update(.., &kp, .., sc, nullptr) -- the second-pass fluxes on the planes of
// `kp` stay in F; sc == nullptr: without new_dt's maxima (a Grid with children: k_cfl takes them behind RestrictCorrect)
bool flux2_update_keep_dc_built(int nscal, bool grav);      // false: this build has no k_flux2_update_keep_dc for the combination (it would spill): aa_mesh_step
void launch_flux2_update_keep_dc(const HostGrid &g, int nscal, const Run3D *rc, bool grav, DevScalars *sc, const KeepPlanes &kp, hipStream_t st);
// history_dc.hip, for 2-D and 3-D Grids alike: launch_history behind a queued step of a run call with a history schedule armed
// (k_history_dc: the body and the launch geometry of k_history; nothing is stored unless the step in front was taken and a row is
// due -- time_step.h hst_row_due on `clock`, the RunClock at the head of the call's Run2D / Run3D, and `sched`).  Returns the
// number of partial rows, the same as launch_history's.
int launch_history_dc(const DevGrid &g, int nscal, Real *partial, const RunClock *clock, Real tlim, const HstSched *sched, hipStream_t st);
// hydro3d_clock.hip: the clocks of a Mesh's Grids (rc[0 .. tab.n - 1]) for a call, the ratios of every Grid's own dx, the maxima zeroed ...
void launch_3d_mesh_seed(Run3D *rc, const Run3D &v, const MeshClockTab3 &tab, hipStream_t st);
// ... and main.c:618-629 over all Grids (time_step.h run_advance_levels, three directions), every Grid's next ratios, `stepped`; `out`: the host's mirror
void launch_3d_mesh_advance(Run3D *rc, const MeshClockTab3 &tab, RunClock *out, hipStream_t st);

}  // namespace aa
