// run.hip -- the C-ABI of the run calls (include/athena_amd.h: aa_run_1d, aa_run_2d, aa_run_3d): main.c:519-669 until time >= t_stop,
// nstep == nstep_stop or dt <= 0 with the loop's clock on the device -- a 1-D Grid in ONE launch (hydro1d_kernels.hip k1d_run), a 2-D
// Grid as AA_2D_BATCH queued steps per read of the clock (hydro2d_kernels.hip k2d_advance), a 3-D hydro Grid on the default CTU chain
// as AA_3D_BATCH queued steps (hydro_kernels.hip k3d_advance; what that chain does not cover loops over aa_step) -- or, with the
// knob of any at 0, step by step.  One body behind the three names: the refusals, the fallback and the seed / synchronise / read-back
// frame are written once (run_frame, which aa_mesh_run_2d and aa_mesh_run_3d of smr.hip share for the Grids of a Mesh on one clock).
// The rule of the step and the loop condition are those of time_step.h, on the host and in the two kernels.
// aa_run_hst_arm / aa_run_hst_rows: the history rows of the next run call without a stop (k_hst_row here, k_history_dc of
// history_dc.hip behind every queued step; aa_history behind every single step), by time_step.h hst_row_due in both forms.
#include <hip/hip_runtime.h>
#include <string.h>
#include "api_internal.h"

using namespace aa;

// The clock of a run call: ONE page-locked, device-visible RunClock per Grid -- k1d_run reads and writes it in place; k2d_advance
// copies the clock it keeps in device memory (Run2D, 2-D Grids only) into it for the host's one read per batch, and k3d_advance
// does the same from the Run3D of a 3-D Grid.  Made by the first call that reaches the device; aa_destroy frees them.
static int run_buffers(aa_grid *g, const char *who)
{
  if (g->clock) return 0;
  RunClock *h = nullptr, *hd = nullptr; Run2D *d = nullptr; Run3D *d3 = nullptr;
  if (hipHostMalloc(&h, sizeof(RunClock), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&hd, h, 0) != hipSuccess || (g->two_d && hipMalloc(&d, sizeof(Run2D)) != hipSuccess) ||
      (!g->two_d && !g->one_d && hipMalloc(&d3, sizeof(Run3D)) != hipSuccess)) {
    if (h) hipHostFree(h);
    (void)hipGetLastError();
    return aa_fail(-2, "[%s]: clock buffers", who);
  }
  memset(h, 0, sizeof(RunClock));
  g->clock = h; g->clock_dev = hd; g->run2d_dev = d; g->run3d_dev = d3;
  return 0;
}

// ---- history rows behind queued steps (aa_run_hst_arm; time_step.h HstSched / hst_row_due) -----------------------------------------
// the schedule of a call, and its mirror for the host
__global__ void __launch_bounds__(64)
k_hst_seed(HstSched *s, HstSched *mirror, HstSched v)
{
  if (threadIdx.x != 0) return;
  *s = v; *mirror = v;
}
// One workgroup behind k_history_dc, with that kernel's predicate on the same clock and the same schedule: nothing to do behind a
// step that was not taken.  Behind a taken step with a row due, lane q < 9 adds column q of the `nb` partial rows in block order
// and multiplies by dVol -- the loop of aa_history on the host (api.hip), one addition after the other, nothing contracted -- and
// the row {time, dt, sums[9]} goes to slot nrows % cap of the ring, time and dt being the clock's behind the advance kernel.  The
// launch with `commit` (a Grid's only one; the last of a Mesh's Grids, the others leaving the schedule as they found it) then
// writes the schedule -- it is its only writer behind the seed -- and the mirror: the next time, the row count, the step seen.
// Launch rule as k1d_run states it: a plain launch in stream order; the barrier is reached by all 64 lanes (the early return is
// uniform), nothing waits on memory or on another workgroup, no atomics.
__global__ void __launch_bounds__(64)
k_hst_row(const Real *partial, int nb, Real dVol, const RunClock *clock, Real tlim, HstSched *sched, HstSched *mirror,
          Real *ring, int cap, int commit)
{
#pragma clang fp contract(off)
  const RunClock c = *clock; HstSched s = *sched;
  if (c.nstep == s.nstep_seen) return;
  const int lane = threadIdx.x;
  const int due = hst_row_due(c.time, c.nstep, tlim, s.nlim, s.dt_out, &s.t_next);
  if (due) {
    Real *row = ring + (long)(s.nrows % cap)*AA_HST_ROW;
    if (lane < 9) {
      Real sum = 0.0;
      for (int b = 0; b < nb; b++) sum += partial[(long)b*9 + lane];
      row[2 + lane] = dVol*sum;
    } else if (lane == 9) row[0] = c.time;
    else if (lane == 10) row[1] = c.dt;
  }
  __syncthreads();                                   // every lane has read the schedule
  if (!commit || lane != 0) return;
  s.nrows += due; s.nstep_seen = c.nstep;
  *sched = s; *mirror = s;
}

int hst_grid_buffers(aa_grid *g, int cap, const char *who)
{
  if (cap < 1) cap = 1;
  if (g->hst_ring && g->hst_ring_cap >= cap) return 0;
  hst_free_grid(g);
  double *h = nullptr, *hd = nullptr; Real *p = nullptr;
  if (hipHostMalloc(&h, (size_t)cap*AA_HST_ROW*sizeof(double), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&hd, h, 0) != hipSuccess || hipMalloc(&p, (size_t)1024*9*sizeof(Real)) != hipSuccess) {
    if (h) hipHostFree(h);
    (void)hipGetLastError();
    return aa_fail(-2, "[%s]: history row buffers", who);
  }
  g->hst_ring = h; g->hst_ring_dev = hd; g->hst_ring_cap = cap; g->hst_part = p;
  return 0;
}
int hst_sched_buffers(HstRun &h, const char *who)
{
  if (h.sched) return 0;
  HstSched *d = nullptr, *m = nullptr, *md = nullptr;
  if (hipHostMalloc(&m, sizeof(HstSched), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&md, m, 0) != hipSuccess || hipMalloc(&d, sizeof(HstSched)) != hipSuccess) {
    if (m) hipHostFree(m);
    (void)hipGetLastError();
    return aa_fail(-2, "[%s]: history schedule buffers", who);
  }
  memset(m, 0, sizeof(HstSched));
  h.sched = d; h.mirror = m; h.mirror_dev = md;
  return 0;
}
void hst_free_grid(aa_grid *g)
{
  if (g->hst_ring) hipHostFree(g->hst_ring);
  if (g->hst_part) hipFree(g->hst_part);
  g->hst_ring = g->hst_ring_dev = nullptr; g->hst_part = nullptr; g->hst_ring_cap = 0;
}
void hst_free_sched(HstRun &h)
{
  if (h.mirror) hipHostFree(h.mirror);
  if (h.sched) hipFree(h.sched);
  h.sched = h.mirror = h.mirror_dev = nullptr;
}
int hst_row_host(aa_grid *g, double time, double dt)
{
  double row[AA_HST_ROW] = {time, dt};
  if (int rc = aa_history(g, row + 2)) return rc;
  g->hst_rows.insert(g->hst_rows.end(), row, row + AA_HST_ROW);
  return 0;
}
void hst_drain_grid(aa_grid *g, const HstRun &h)
{
  for (int r = h.drained; r < h.mirror->nrows; r++) {
    const double *row = g->hst_ring + (size_t)(r % h.cap)*AA_HST_ROW;
    g->hst_rows.insert(g->hst_rows.end(), row, row + AA_HST_ROW);
  }
}
void launch_hst_seed(HstRun &h, int nstep, hipStream_t st)
{
  const HstSched v = {h.t_next, h.dt_out, h.nlim, 0, nstep, 0};
  h.drained = 0;
  hipLaunchKernelGGL(k_hst_seed, dim3(1), dim3(64), 0, st, h.sched, h.mirror_dev, v);
}
void launch_hst_row(aa_grid *g, int nb, const RunClock *clock, double tlim, const HstRun &h, bool commit, hipStream_t st)
{
  const double dVol = g->d.dx[0]*g->d.dx[1]*g->d.dx[2];      // (aa_history's expression)
  hipLaunchKernelGGL(k_hst_row, dim3(1), dim3(64), 0, st, g->hst_part, nb, dVol, clock, tlim, h.sched, h.mirror_dev,
                     g->hst_ring_dev, h.cap, commit ? 1 : 0);
}
// the two launches behind a queued step of a stand-alone Grid (clock: the RunClock at the head of its Run2D / Run3D)
static void queue_hst(aa_grid *g, const RunClock *clock, double tlim)
{
  Scope s(g, "hst_row");
  const int nb = launch_history_dc(g->d, g->p.nscal, g->hst_part, clock, tlim, g->hst.sched, g->st);
  launch_hst_row(g, nb, clock, tlim, g->hst, true, g->st);
}

// The integrator's chain of a 2-D Grid on the clock `rc`, on g->st.  The stage names are those of aa_integrate_2d_*.  A stand-alone
// Grid (aa_run_2d: its own clock, new_dt's maxima always on board) and a level of a Mesh (aa_mesh_run_2d in smr.hip: the Mesh's one
// clock, the update kernel in its flux-keeping form, sc == nullptr where the level's maxima are taken later) share it.
void queue_chain_2d(aa_grid *g, const Run2D *rc, DevScalars *sc)
{
  const HostGrid &d = g->d;
  g->stepped_2d = true;
  if (g->p.integrator == 1) {
    { Scope s(g, "vl2d_predict"); launch_2d_vl_predict_dc(d, rc, g->edge2d, g->st); }
    { Scope s(g, "vl2d_flux2_update");
      if (g->keep_flux) launch_2d_vl_flux2_update_keep_dc(d, rc, g->edge2d, sc, g->keep, g->st);
      else launch_2d_vl_flux2_update_dc(d, rc, g->edge2d, sc, g->order_2d, g->st); }
  } else {
    { Scope s(g, "ctu2d_first"); launch_2d_ctu_first_dc(d, rc, g->edge2d, g->order_2d, g->st); }
    { Scope s(g, "ctu2d_correct"); launch_2d_ctu_correct_dc(d, rc, g->p.integrator == 0, g->st); }
    { Scope s(g, "ctu2d_flux2_update");
      if (g->keep_flux) launch_2d_ctu_flux2_update_keep_dc(d, rc, g->edge2d, sc, g->keep, g->st);
      else launch_2d_ctu_flux2_update_dc(d, rc, g->edge2d, sc, g->st); }
  }
}

// one step of the queue: the integrator's chain with new_dt's maxima on board, k2d_advance, bvals_mhd (main.c:572-644 without
// Userwork_in_loop: a Grid with pinned zones is refused).  The stage names are those of aa_integrate_2d_* / aa_bvals_mhd.
static void queue_step_2d(aa_grid *g, double tlim)
{
  const HostGrid &d = g->d;
  queue_chain_2d(g, g->run2d_dev, g->sc);
  { Scope s(g, "run2d_advance"); launch_2d_advance(d, g->run2d_dev, g->sc, g->clock_dev, g->st); }
  // The boundary kernels (k_bc) take no dt and are not predicated.  With four or more zones per direction every ghost zone is a
  // copy of an ACTIVE zone (x1 pass) or of a row whose x1 ghost zones that pass has just filled (x2 pass), so behind a stopped
  // step -- U untouched -- they write again what is there: idempotent.  (Grids with fewer zones step one at a time, below.)
  { Scope s(g, "bvals_mhd");
    for (int a = 0; a < 2; a++) launch_bc_dir(d, g->p.nscal, a, g->p.bc[2*a], g->p.bc[2*a + 1], g->st); }
  // (only while a history schedule is armed: with none a queued step launches what it always did)
  if (g->hst.active) queue_hst(g, &g->run2d_dev->c, tlim);
}

// Whether aa_run_3d queues this Grid's steps: what aa_integrate_3d_ctu launches BY DEFAULT for one hydro Grid on one device -- the x2
// march, the tile-edge x1 fluxes, k_correct_all with both other first passes on board, k_flux2_update with new_dt's maxima -- is the
// chain whose kernels have entries on the device clock.  Everything else loops over aa_step, with the same results: the van Leer
// integrator (and fofc with it), a cooling function (namespace aa_cool), ion radiation, the tile kernels of a small Grid
// (AA_CORRECT_ALL off), AA_X3_FUSED=0, AA_FUSED_UPDATE=0, AA_CFL_FUSED=0, AA_EDGE_OVERLAP=1 (a second stream), first-pass sweeps
// already done by aa_integrate_begin, a direction with fewer zones than ghost zones (queue_step_3d says why), and in the strict
// build a passive scalar together with a static potential (correct_all_dc_built: that k_correct_all needs scratch there).
// The part of that which is the Grid's own -- asked of a stand-alone Grid here and of every level of a Mesh by aa_mesh_run_3d
// (smr.hip), which adds what a level needs on top: the flux-keeping update entry (flux2_update_keep_dc_built).  (p.ion keeps a
// level off the queue as it does a Grid: with a plane on the root, the radiation step of aa_mesh_step comes first.)
bool on_queued_chain_3d(const aa_grid *g)
{
  const LaunchCfg &c = g->d.cfg;
  const bool x3_fused = c.x3_fused_mode >= 0 ? c.x3_fused_mode != 0 : true;      // (api.hip x3_fused)
  return !g->one_d && !g->two_d && g->slab.empty() && (g->p.integrator == 0 || g->p.integrator == 2) && !g->fofc &&
         !g->cool && !g->p.ion && c.correct_all && x3_fused && c.fused_update && c.cfl_step && !c.edge_overlap && !g->inner_swept &&
         g->d.Nx1 >= AA_NGHOST && g->d.Nx2 >= AA_NGHOST && g->d.Nx3 >= AA_NGHOST && correct_all_dc_built(g->p.nscal, g->grav);
}
static bool queues_3d(const aa_grid *g) { return g->batch_3d > 0 && on_queued_chain_3d(g); }

// one step of the 3-D queue: aa_integrate_3d_ctu's default chain with dt and the StepRatios from the clock, bvals_mhd, k3d_advance
// (main.c:572-644 without Userwork_in_loop: a Grid with pinned zones is refused).  The stage names are those of
// aa_integrate_3d_ctu / aa_bvals_mhd.  Plain launches in stream order; nothing is captured, nothing launched cooperatively, no kernel
// waits on memory or on another workgroup; the host reads the clock only behind run_frame's hipStreamSynchronize.
// (the chain and the boundary pass are queue_chain_3d / queue_bvals_3d, which the levels of a Mesh share: smr.hip mesh_queue_step_3d)
void queue_chain_3d(aa_grid *g, const Run3D *rc, DevScalars *sc)
{
  const HostGrid &d = g->d; const int ns = g->p.nscal;
  if (d.slope) { Scope s(g, "ppm_slopes"); for (int dir = 0; dir < 3; dir++) launch_slopes(d, ns, dir, g->st, nullptr); }
  { Scope s(g, "sweep_x2"); launch_sweep_x2_dc(d, ns, rc, g->grav, g->st); }
  { Scope s(g, "correct_all"); launch_correct_all_dc(d, ns, rc, g->grav, g->st); }
  if (g->p.integrator == 2) { Scope s(g, "no_h_correction"); (void)hipMemsetAsync(d.eta, 0, (size_t)3*d.nc*sizeof(Real), g->st); }
  { Scope s(g, "flux2_update");
    if (g->keep_flux) launch_flux2_update_keep_dc(d, ns, rc, g->grav, sc, g->keep, g->st);      // a level of a Mesh; sc == nullptr: without new_dt's maxima
    else launch_flux2_update_dc(d, ns, rc, g->grav, sc, g->st); }
}
void queue_bvals_3d(aa_grid *g)
{
  const HostGrid &d = g->d; const int ns = g->p.nscal;
  Scope s(g, "bvals_mhd");
  if (d.cfg.bc_one) launch_bc_shell(d, ns, g->p.bc, g->st);
  else for (int a = 0; a < 3; a++) launch_bc_dir(d, ns, a, g->p.bc[2*a], g->p.bc[2*a + 1], g->st);
}
static void queue_step_3d(aa_grid *g, double tlim)
{
  const HostGrid &d = g->d;
  queue_chain_3d(g, g->run3d_dev, g->sc);
  // What takes no dt is not predicated: k_slopes* (slope arrays), k_eta_edges and the eta memset (eta arrays) write scratch of the
  // step that the next taken step fills again before it reads it, and behind the stop there is no such step in this call.  The
  // boundary kernels write U.  k_bc_shell gives every ghost zone the value of ONE source zone, found by mapping its ghost
  // coordinates into the active range (k_bc, one pass per direction, does the same in three copies); with AA_NGHOST or more zones
  // in every direction that source is an ACTIVE zone, never itself a target.  Behind a stopped step the active zones are untouched,
  // so the kernel writes again what the last taken step's boundary pass wrote: idempotent, in either form (AA_BC_ONE).  A Grid
  // with fewer zones along a direction has ghost zones among its sources and steps one at a time (queues_3d).
  queue_bvals_3d(g);
  { Scope s(g, "run3d_advance"); launch_3d_advance(d, g->run3d_dev, g->sc, g->clock_dev, g->st); }
  if (g->hst.active) queue_hst(g, &g->run3d_dev->c, tlim);      // (as queue_step_2d)
}

// ---- the frame of every run call (api_internal.h RunOps): the span and tlim refusals, the loop over single steps, and the seed /
// queue / synchronise / read the clock loop.  aa_run_1d and aa_run_2d come here through run_to_time, aa_mesh_run_2d from smr.hip.
int run_frame(const RunOps &o, double t_stop, double tlim, int nstep_stop, int *nsteps_done)
{
  const char *who = o.who;
  const long long span = (long long)nstep_stop - *o.nstep;
  if (span < 0 || span > (1LL << 20))
    return aa_fail(-1, "[%s]: nstep_stop=%d from nstep=%d: a call covers 0 .. 2^20 steps", who, nstep_stop, *o.nstep);
  if (tlim != o.tlim) return aa_fail(-1, "[%s]: tlim=%.17g, but the %s was created with %.17g (new_dt clips at that one)", who, tlim, o.owner, o.tlim);
  const int nstep0 = *o.nstep;
  HstRun *h = o.hst;
  if (o.stepwise) {
    while (run_live(*o.time, t_stop, *o.nstep, nstep_stop, *o.dt)) {
      int rc = o.step(o.self); if (rc) return rc;
      // data_output's rule for the armed block behind the step, on the host: the same function the kernels of the queued form call
      if (h && hst_row_due(*o.time, *o.nstep, tlim, h->nlim, h->dt_out, &h->t_next)) { rc = o.hst_row(o.self); if (rc) return rc; }
    }
    if (nsteps_done) *nsteps_done = *o.nstep - nstep0;
    return 0;
  }
  if (nsteps_done) *nsteps_done = 0;
  if (!run_live(*o.time, t_stop, *o.nstep, nstep_stop, *o.dt)) return 0;      // nothing launched, nothing read back
  RunClock *clock = nullptr;
  const RunClock seed = {*o.dt, 1, *o.nstep, *o.time};
  if (int rc = o.begin(o.self, seed, t_stop, tlim, nstep_stop, &clock)) return rc;
  if (h) { if (int rc = o.hst_begin(o.self, seed.nstep)) return rc; }
  // Every launch ends whatever the data are, so the queue drains.  1-D: the one launch runs to the stop and leaves live = 0.  2-D: a
  // step behind the stop costs its launches and nothing else (up to AA_2D_BATCH - 1 of them per call); 3-D likewise (AA_3D_BATCH).
  do {
    if (int rc = o.batch(o.self, t_stop, tlim, nstep_stop)) return rc;
    HIPCHK(hipGetLastError());
    (*o.host_syncs)++;
    HIPCHK(hipStreamSynchronize(o.st));
    // the rows this batch left (at most one per step) move to the host's memory: the rings never hold more than a batch
    if (h) { o.hst_drain(o.self); h->drained = h->mirror->nrows; }
  } while (clock->live);
  if (h) h->t_next = h->mirror->t_next;
  *o.time = clock->time; *o.dt = clock->dt; *o.nstep = clock->nstep;
  if (o.end) o.end(o.self);
  if (nsteps_done) *nsteps_done = *o.nstep - nstep0;
  return 0;
}

// a Grid behind that frame
static int grid_step(void *self) { return aa_step((aa_grid*)self, nullptr); }
static int grid_begin(void *self, const RunClock &seed, double t_stop, double tlim, int nstep_stop, RunClock **clock)
{
  aa_grid *g = (aa_grid*)self;
  if (int rc = run_buffers(g, g->one_d ? "aa_run_1d" : g->two_d ? "aa_run_2d" : "aa_run_3d")) return rc;
  g->cfl_ready = false; g->active_dirty = true;
  if (g->one_d) *g->clock = seed;
  else if (!g->two_d) {
    Run3D v = {seed, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, t_stop, tlim, g->p.cour_no, nstep_stop, 0};      // (k3d_seed forms the ratios; `stepped` is a Mesh's)
    launch_3d_seed(g->d, g->run3d_dev, v, g->sc, g->st);
  } else {
    const Run2D v = {seed, t_stop, tlim, g->p.cour_no, nstep_stop, 0};
    launch_2d_seed(g->run2d_dev, v, g->sc, g->st);
  }
  *clock = g->clock;
  return 0;
}
static int grid_batch(void *self, double t_stop, double tlim, int nstep_stop)
{
  aa_grid *g = (aa_grid*)self;
  if (g->one_d) {
    Scope s(g, g->p.integrator == 1 ? "vl1d_run" : "ctu1d_run");
    launch_1d_run(g->d, g->p.integrator == 1, g->p.order == 3, g->p.bc[0], g->p.bc[1], g->p.cour_no, t_stop, tlim, nstep_stop, g->clock_dev, g->st);
  } else if (g->two_d) for (int k = 0; k < g->batch_2d; k++) queue_step_2d(g, tlim);
  else for (int k = 0; k < g->batch_3d; k++) queue_step_3d(g, tlim);
  return 0;
}

// ... and its history schedule, where the call has one
static int grid_hst_row(void *self) { aa_grid *g = (aa_grid*)self; return hst_row_host(g, g->time, g->dt); }
static int grid_hst_begin(void *self, int nstep) { aa_grid *g = (aa_grid*)self; launch_hst_seed(g->hst, nstep, g->st); return 0; }
static void grid_hst_drain(void *self) { aa_grid *g = (aa_grid*)self; hst_drain_grid(g, g->hst); }

// `who`: the entry's name for its messages; ndim: the Grids it takes
static int run_to_time(aa_grid *g, const char *who, int ndim, double t_stop, double tlim, int nstep_stop, int *nsteps_done)
{
  if (!g) return aa_fail(-1, "[%s]: null argument", who);
  // a schedule armed for this call is taken over here and disarmed, whatever the call returns
  struct Disarm { HstRun &h; ~Disarm() { h.active = false; } } disarm = {g->hst};
  g->hst.active = g->hst.armed; g->hst.armed = false;
  if (g->hst.active) g->hst_rows.clear();
  if (ndim == 1) {
    if (!g->one_d) return aa_fail(-1, "[%s]: this is a %s Grid: only a 1-D Grid runs many steps per launch", who, g->two_d ? "2-D" : "3-D");
    // (before the knob is looked at: AA_1D_RESIDENT=0 does not lift it)
    if (g->d.Nx1 > run1d_cap())
      return aa_fail(-1, "[%s]: a 1-D Grid of %d zones is above the %d the resident kernel keeps in one workgroup's LDS: aa_step", who, g->d.Nx1, run1d_cap());
  } else if (ndim == 3) {
    if (g->one_d) return aa_fail(-1, "[%s]: this is a 1-D Grid (Nx2 = Nx3 = 1): aa_run_1d", who);
    if (g->two_d) return aa_fail(-1, "[%s]: this is a 2-D Grid (Nx3 = 1): aa_run_2d", who);
    if (!g->slab.empty()) return aa_fail(-1, "[%s]: a Grid cut into slabs steps one at a time: aa_step", who);
  } else {
    if (g->one_d) return aa_fail(-1, "[%s]: this is a 1-D Grid (Nx2 = Nx3 = 1): aa_run_1d", who);
    if (!g->two_d) return aa_fail(-1, "[%s]: this is a 3-D Grid: only 1-D and 2-D Grids run many steps per host visit", who);
  }
  if (g->npin > 0) return aa_fail(-1, "[%s]: a %d-D Grid with pinned zones steps one at a time: aa_step", who, ndim);
  if (g->keep_flux || g->level > 0)      // (2-D and 3-D: a 1-D Grid is never a level of a Mesh)
    return aa_fail(-1, "[%s]: this Grid is a level of a Mesh (level %d): the levels step together, aa_mesh_step", who, g->level);
  // step by step: either knob at 0, or fewer zones than ghost zones along a direction of a 2-D Grid (a boundary kernel reads ghost
  // zones there, see queue_step_2d)
  RunOps o;
  o.who = who; o.owner = "Grid"; o.self = g; o.time = &g->time; o.dt = &g->dt; o.nstep = &g->nstep; o.tlim = g->p.tlim;
  o.stepwise = ndim == 1 ? !g->resident_1d : ndim == 3 ? !queues_3d(g) : (g->batch_2d == 0 || g->d.Nx1 < AA_NGHOST || g->d.Nx2 < AA_NGHOST);
  o.step = grid_step; o.begin = grid_begin; o.batch = grid_batch; o.end = nullptr; o.st = g->st; o.host_syncs = &g->host_syncs;
  if (g->hst.active) { o.hst = &g->hst; o.hst_row = grid_hst_row; o.hst_begin = grid_hst_begin; o.hst_drain = grid_hst_drain; }
  return run_frame(o, t_stop, tlim, nstep_stop, nsteps_done);
}

extern "C" {

int aa_run_1d_cap(void) { return run1d_cap(); }
int aa_run_2d_batch(const aa_grid *g) { return g && g->two_d ? g->batch_2d : 0; }
int aa_run_1d(aa_grid *g, double t_stop, double tlim, int nstep_stop, int *nsteps_done)
{ return run_to_time(g, "aa_run_1d", 1, t_stop, tlim, nstep_stop, nsteps_done); }
int aa_run_2d(aa_grid *g, double t_stop, double tlim, int nstep_stop, int *nsteps_done)
{ return run_to_time(g, "aa_run_2d", 2, t_stop, tlim, nstep_stop, nsteps_done); }
int aa_run_3d_batch(const aa_grid *g) { return g && queues_3d(g) ? g->batch_3d : 0; }
int aa_run_3d(aa_grid *g, double t_stop, double tlim, int nstep_stop, int *nsteps_done)
{ return run_to_time(g, "aa_run_3d", 3, t_stop, tlim, nstep_stop, nsteps_done); }

int aa_run_hst_arm(aa_grid *g, double t_next, double dt_out, int nlim)
{
  const char *who = "aa_run_hst_arm";
  if (!g) return aa_fail(-1, "[%s]: null argument", who);
  if (g->one_d) return aa_fail(-1, "[%s]: this is a 1-D Grid: aa_run_1d keeps the whole loop in one launch and would add the sums in another order; its history rows stay stop times", who);
  if (!g->slab.empty()) return aa_fail(-1, "[%s]: a Grid cut into slabs steps one at a time: aa_step, aa_history", who);
  if (g->keep_flux || g->level > 0)
    return aa_fail(-1, "[%s]: this Grid is a level of a Mesh (level %d): aa_mesh_run_hst_arm", who, g->level);
  const int cap = g->two_d ? g->batch_2d : g->batch_3d;      // rows of one batch; 0: the call steps one at a time and needs no device buffer
  if (cap > 0) {
    if (int rc = hst_grid_buffers(g, cap, who)) return rc;
    if (int rc = hst_sched_buffers(g->hst, who)) return rc;
  }
  g->hst.t_next = t_next; g->hst.dt_out = dt_out; g->hst.nlim = nlim < 0 ? -1 : nlim; g->hst.cap = cap;
  g->hst.armed = true;
  return 0;
}
int aa_run_hst_rows(aa_grid *g, int cap, double *rows, int *nrows, double *t_next)
{
  if (!g) return aa_fail(-1, "[aa_run_hst_rows]: null argument");
  const int n = (int)(g->hst_rows.size()/AA_HST_ROW);
  if (rows && cap > 0) memcpy(rows, g->hst_rows.data(), (size_t)(n < cap ? n : cap)*AA_HST_ROW*sizeof(double));
  if (nrows) *nrows = n;
  if (t_next) *t_next = g->hst.t_next;
  return 0;
}

}  // extern "C"
