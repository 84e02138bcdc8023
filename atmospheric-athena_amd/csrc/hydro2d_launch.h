// hydro2d_launch.h -- the device clock of aa_run_2d and the launch interface of the 2-D kernel chains that read it
// (hydro2d_kernels.hip).  Kept apart from grid.h, which the 3-D kernel files include; the chains that take dt as a kernel argument
// (aa_step on a 2-D Grid) are declared there.
#pragma once
#include "grid.h"
#include "time_step.h"

// steps aa_run_2d queues between two reads of the clock where AA_2D_BATCH is not set (0: one aa_step at a time); DESIGN section 8
// has the measurement it comes from
#define AA_2D_BATCH_DEFAULT 32
// ... and steps aa_mesh_run_2d queues for the Grids of a 2-D Mesh (0: one aa_mesh_step at a time); section 8 has its own measurement
#define AA_2D_MESH_BATCH_DEFAULT 8
// Grids of a Mesh the argument table of k2d_mesh_advance / k2d_mesh_seed holds; a Mesh with more steps one aa_mesh_step at a time
#define AA_2D_MESH_GRIDS 16

namespace aa {

// The clock (time_step.h RunClock) of a 2-D Grid while aa_run_2d has steps queued, with the call's limits, in DEVICE memory: every
// kernel of a queued step reads `dt` and `live` (one 16-byte uniform load), k2d_advance behind the step's update kernel writes the
// next ones -- and a copy of the clock into the page-locked RunClock the host reads ONCE per batch of queued steps.  live = 0: the
// call's stop rule has fired; what is queued behind it returns without a store.
struct Run2D {
  RunClock c;
  Real t_stop, tlim, cour_no;       // of the call: main.c's loop condition, new_dt.c's clip and CourNo
  int nstep_stop;
  int stepped;                      // aa_mesh_run_2d only: the step this advance kernel stands behind was taken (`live` before it ran)
};

// the Grids of a Mesh as k2d_mesh_seed / k2d_mesh_advance see them: new_dt's maxima and the zone sizes, in the Mesh's order
struct MeshClockTab { int n, pad; DevScalars *sc[AA_2D_MESH_GRIDS]; Real dx[2*AA_2D_MESH_GRIDS]; };

// the two chains of grid.h that reconstruct, with the Grid's effective reconstruction order (2: PLM; 3: PPM, aa_set_order_2d): the CTU
// first pass and the van Leer corrector.  (grid.h's declarations of the same names, without `order`, are the second-order forms.)
void launch_2d_ctu_first(const DevGrid &g, Real dt, Real *edge, int order, hipStream_t st);
void launch_2d_vl_flux2_update(const DevGrid &g, Real dt, Real *edge, DevScalars *sc, int order, hipStream_t st);
void launch_2d_seed(Run2D *rc, const Run2D &v, DevScalars *sc, hipStream_t st);               // the clock of a call; new_dt's maxima zeroed
void launch_2d_ctu_first_dc(const DevGrid &g, const Run2D *rc, Real *edge, int order, hipStream_t st);          // as launch_2d_ctu_first ...
void launch_2d_ctu_correct_dc(const DevGrid &g, const Run2D *rc, bool hcorr, hipStream_t st);
void launch_2d_ctu_flux2_update_dc(const DevGrid &g, const Run2D *rc, Real *edge, DevScalars *sc, hipStream_t st);   // (always with new_dt's maxima)
void launch_2d_vl_predict_dc(const DevGrid &g, const Run2D *rc, Real *edge, hipStream_t st);
void launch_2d_vl_flux2_update_dc(const DevGrid &g, const Run2D *rc, Real *edge, DevScalars *sc, int order, hipStream_t st);
// nstep++, time += dt, new_dt with the clip at tlim, the maxima zeroed again, the stop rule; `out`: the host's mirror
void launch_2d_advance(const DevGrid &g, Run2D *rc, DevScalars *sc, RunClock *out, hipStream_t st);
// the Grids of a 2-D Mesh on ONE clock (aa_mesh_run_2d): the flux-keeping update kernels (sc == nullptr: without new_dt's maxima, for
// a Grid that restriction and flux correction rewrite behind it), the clock of a call with every Grid's maxima zeroed, and
// aa_mesh_step's nstep++ / time += dt / aa_mesh_new_dt over the Grids of `tab` (time_step.h run_advance_levels)
void launch_2d_ctu_flux2_update_keep_dc(const DevGrid &g, const Run2D *rc, Real *edge, DevScalars *sc, const KeepPlanes &kp, hipStream_t st);
void launch_2d_vl_flux2_update_keep_dc(const DevGrid &g, const Run2D *rc, Real *edge, DevScalars *sc, const KeepPlanes &kp, hipStream_t st);
void launch_2d_mesh_seed(Run2D *rc, const Run2D &v, const MeshClockTab &tab, hipStream_t st);
void launch_2d_mesh_advance(Run2D *rc, const MeshClockTab &tab, RunClock *out, hipStream_t st);

}  // namespace aa
