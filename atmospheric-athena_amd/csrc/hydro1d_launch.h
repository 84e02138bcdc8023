// hydro1d_launch.h -- launch interface of hydro1d_kernels.hip: a 1-D Grid (Nx2 = Nx3 = 1: one row of N1 zones per field, fields
// nc = sJ apart; aa_create).  Kept apart from grid.h, which the 3-D kernel files include.
#pragma once
#include "grid.h"
#include "time_step.h"

namespace aa {

int  run1d_cap();                                  // most active zones of the resident kernel
int  step1d_block();                               // active zones per block of k1d_step
// one step of integrate_1d_ctu.c (vl false) / integrate_1d_vl.c (vl true), second or third order, from U into Unew (ghost zones
// copied); sc: and new_dt's maximum
void launch_1d_step(const DevGrid &g, bool vl, bool third, Real dt, Real *Unew, DevScalars *sc, hipStream_t st);
// whole passes of the main loop in one workgroup; rs: time, dt, nstep in and out (time_step.h RunClock; `live` is not looked at)
void launch_1d_run(const DevGrid &g, bool vl, bool third, int bc_in, int bc_out, Real cour_no, Real t_stop, Real tlim, int nstep_stop, RunClock *rs, hipStream_t st);

}  // namespace aa
