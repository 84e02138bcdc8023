// api_internal.h -- state shared by the translation units that implement the C-ABI (api.hip: one
// Grid; smr.hip: the nested levels of a static-mesh-refinement Mesh).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "../../include/athena_amd.h"
#include "grid.h"
#include "hydro1d_launch.h"
#include "hydro2d_launch.h"
#include "hydro3d_launch.h"
#include "ion_subcycle.h"

int aa_fail(int code, const char *fmt, ...);   // records the message aa_last_error() returns
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
  return aa_fail(-2, "[athena_amd] HIP error %s at %s:%d: %s", #x, __FILE__, __LINE__, hipGetErrorString(e_)); } while (0)

// A history schedule of a run call (run.hip: aa_run_hst_arm for a Grid, smr.hip: aa_mesh_run_hst_arm for a Mesh -- ONE for all its
// Grids).  armed: for the next run call, which takes it over (active) and disarms it whatever it returns.  t_next: as armed, then
// the schedule's behind the call.  sched: the device's copy (only k_hst_row writes it, behind k_hst_seed); mirror / mirror_dev:
// the page-locked copy k_hst_row leaves for the host and its device address, read behind run_frame's synchronise like the clock;
// cap: rows of every Grid's ring -- the steps of one batch; drained: rows of this call already taken from the rings.
struct HstRun {
  bool armed = false, active = false;
  double t_next = 0, dt_out = 0; int nlim = -1;
  HstSched *sched = nullptr, *mirror = nullptr, *mirror_dev = nullptr;
  int cap = 0, drained = 0;
};

struct ProfEntry { std::string name; std::vector<hipEvent_t> ev; double total_ms = 0; long long launches = 0; };

struct aa_grid {
  aa_params p;
  aa::HostGrid d;
  aa::IonPar ion;
  hipStream_t st = nullptr; bool own_stream = false;
  hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;      // aa_integrate_3d_ctu: the tile-edge x1 fluxes beside the x2 sweep
  aa::Real *pool = nullptr; size_t pool_doubles = 0;
  aa::DevScalars *sc = nullptr;        // device
  aa::DevScalars *sc_host = nullptr;   // pinned (= &mb->s)
  aa::Mailbox *mb = nullptr, *mb_dev = nullptr;   // the pinned mailbox and its device address (grid.h Mailbox); mb_seq: stamps handed out
  unsigned long long mb_seq = 0;
  unsigned long long mb_prepublished = 0;   // stamp of the scalars the last fused pick already put into the mailbox (0: none): the fetch right behind it only polls
  bool ion_fuse_pick = false;          // the pass just queued left its records unfolded: aa_ion_pick folds and picks in one launch (one rank)
  long long *pin_idx = nullptr; aa::Real *pin_val = nullptr; long long npin = 0;
  double *cfl_part = nullptr; long cfl_part_n = 0;   // the blocks' CFL maxima of k_update<CFL> (van Leer integrator), 3 x update_blocks
  unsigned char *pin_mask = nullptr;   // 1 where a zone is pinned (k_flux2_update<CFL> leaves those to k_pinned_cfl)
  bool cfl_in_update = false;          // aa_cfl_in_update: the integrator also leaves new_dt's maxima behind
  double ion_spec_dt = -1.0, ion_spec_limit = 0.0;   // aa_ion_speculate: armed for the next first pass / what it was told
  bool ion_spec_armed = false;         //   ... the first pass has speculated: aa_ion_pick(first) settles it
  // the lean form of the speculating first pass (k_ion_pass<LEAN>; LaunchCfg ion_lean): what this ion step is doing ...
  bool ion_step_spec = false, ion_step_lean = false;   // its first pass speculated / did so in the lean form
  int ion_step_updates = 0;            // updating passes queued since aa_ion_begin = sub-cycles
  bool ion_lean_next = false;          // ... and what aa_ion_finish made of it: the step speculated and took ONE sub-cycle, so the next one is lean under `auto`
  // LaunchCfg ion_batch (api.hip ion_run_queued): sub-cycles of this Grid's previous ion step (0: none since aa_create, an upload or a
  // restart section -- the first visit of the next one queues 1), and host visits / sub-cycles executed / queued sub-cycles that left at once
  int ion_prev_niter = 0;
  bool ion_gather_entry = false;       // the last ion step came through aa_ion_radtransfer_3d_gather (aa_ion_batch_active)
  long long ion_batch_n[3] = {0, 0, 0};
  long long ion_lean_n[2] = {0, 0};    // speculating first passes queued so far: dense, lean (aa_ion_lean_counts)
  bool cfl_ready = false;              //   ... and has done so for the state as it is now (aa_step arms it by itself: LaunchCfg cfl_step)
  bool active_dirty = true;            // a call since the last full upload / download of U wrote ACTIVE zones on the device (aa_download_ghost_zones then moves the whole block)
  bool grav = false;
  int cool = 0;                        // aa_set_cooling: 1 = KoyInut; the integrator then launches the kernels of namespace aa_cool
  int rad_dir = 0, nradplane = 0; aa::Real flux_i = 0;
  int level = 0;                       // DomainS.Level: > 0 only as a level of an aa_mesh
  bool two_d = false;                  // Nx3 = 1: the 2-D integrators (hydro2d_kernels.hip); U 5 | LR 20 | F 10 | eta 2 | edge2d
  aa::Real *edge2d = nullptr;          //   ... what the x1 tiles of the 2-D kernels hand each other (grid.h)
  int order_2d = 2;                    //   ... its effective reconstruction order: 3 after aa_set_order_2d(g, 3) (p.order stays 2 on a 2-D Grid)
  bool stepped_2d = false;             //   ... an integrator chain of this Grid has been launched (aa_set_order_2d then refuses)
  bool one_d = false;                  // Nx2 = Nx3 = 1 in a 1-D root Domain: the 1-D integrators (hydro1d_kernels.hip); U 5 | LR 5 (the second U buffer)
  bool resident_1d = true;             //   ... AA_1D_RESIDENT=0 (read by aa_create): aa_run_1d steps one launch at a time instead of keeping the Grid in one workgroup's LDS (k1d_run)
  int batch_2d = 0;                    // a 2-D Grid: steps aa_run_2d queues between two reads of the clock (AA_2D_BATCH, read by aa_create; 0: it loops over aa_step)
  int batch_3d = 0;                    // a 3-D Grid: steps aa_run_3d queues between two reads of the clock (AA_3D_BATCH, read by aa_create; 0: it loops over aa_step)
  RunClock *clock = nullptr, *clock_dev = nullptr;   // time, dt, nstep, live of aa_run_1d / aa_run_2d / aa_run_3d (time_step.h): pinned, device-visible host memory and its device address ...
  aa::Run2D *run2d_dev = nullptr;      //   ... and the 2-D call's clock in device memory (hydro2d_launch.h); made by the first run call that reaches the device (run.hip)
  aa::Run3D *run3d_dev = nullptr;      //   ... and the 3-D call's (hydro_launch.h), likewise
  // history rows of a run call with a schedule armed (run.hip): this Grid's schedule (a level of a Mesh uses the Mesh's), the partial
  // rows of k_history_dc in device memory of their own (1024 x 9 doubles: the face-state area is the queued steps'), the page-locked
  // ring k_hst_row appends a batch's rows to with its device address, and the rows of the last armed call on the host, AA_HST_ROW
  // doubles each (aa_run_hst_rows / aa_mesh_run_hst_rows).  Made by the first arming; a Grid that is never armed allocates none.
  HstRun hst;
  aa::Real *hst_part = nullptr;
  double *hst_ring = nullptr, *hst_ring_dev = nullptr; int hst_ring_cap = 0;
  std::vector<double> hst_rows;
  bool inner_swept = false;            // aa_integrate_begin has done the first-pass x1 / x2 sweeps of the planes ks .. ke
  double inner_dt = 0.0;               //   ... with this dt
  bool ion_fused = false;              // one-kernel radiation sub-cycle with the scan sweep (ion_pass.hip): aa_params.ion_path, else LaunchCfg ion_fused; a sweep along x2 turns it off
  bool ion_begin_due = false;          // aa_ion_begin was called: the next first pass does the entry
  bool ef_stale = false;               // GridS.EdgeFlux has not been filled from the last sweep yet (done when somebody reads it)
  int ion_cur = 0; bool ion_pending = false;   // buffer of the last sweep that counts; a sweep launched but not yet relied upon
  aa::IonPart *ion_part = nullptr; aa::Real *ion_words = nullptr;   // per-block records of a pass; this Grid's folded words
  int host_syncs = 0;                  // stream synchronisations that return scalars to the host (bench: per step)
  bool fofc = false;                   // aa_set_fofc: first-order flux correction of the van Leer integrator (integrate_3d_vl.c Steps 10, 14)
  long long *fofc_list = nullptr;      //   ... candidates | sorted | pending, 3 x AA_FOFC_MAX zone indices (device)
  long long fofc_counts[3] = {0, 0, 0};   //   ... of the last step: zones with d < 0, with P < 0, second-order fluxes replaced
  bool keep_flux = false;              // a level of an aa_mesh: RestrictCorrect reads the second-pass fluxes ...
  aa::KeepPlanes keep = {0, {{0}}};        // ... on these face planes (own boundaries + the child's outline)
  double time = 0, dt = 0; int nstep = 0;
  long long bytes = 0;
  // composite (slabs.hip): this handle stands for ONE Grid of the caller cut into x3 slabs, one aa_grid per
  // device; every entry point of the C-ABI forwards to the slabs and does the neighbour exchange / reductions
  std::vector<aa_grid*> slab;
  struct SlabLink *link = nullptr;
  // data dumps (dump.hip): the page-locked bounce buffer (two halves of dump_cap floats), the stream of its copies, and the events
  // "piece staged" [0..1] / "piece on the host" [2..3] of either half; made by the first aa_dump_section
  float *dump_host = nullptr; size_t dump_cap = 0;
  hipStream_t dump_st = nullptr; hipEvent_t dump_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // ... and the snapshot slots of aa_dump_snapshot_begin: a whole payload in device memory (NOT the face-state area) and its page-locked
  // twin, `cap` floats each, made on first use; held: between begin and release; staged / done: "payload made" on st, "on the host" on dump_st
  struct DumpSlot { float *dev = nullptr, *host = nullptr; size_t cap = 0; bool held = false; int fmt = 0; hipEvent_t staged = nullptr, done = nullptr; };
  DumpSlot snap[AA_DUMP_SLOTS];
  // ... and the slot of aa_rst_snapshot_begin (restart.hip): the whole restart payload, `cap` doubles on either side, made on first use;
  // staged: "payload made and EdgeFlux copied" on st, done: "on the host" on dump_st
  struct RstSlot { aa::Real *dev = nullptr, *host = nullptr; size_t cap = 0; bool held = false; hipEvent_t staged = nullptr, done = nullptr; };
  RstSlot rst_snap[AA_RST_SLOTS];
  // single-variable outputs (outdata.hip): the blocks' minimum / maximum records of a piece with the running record behind them, and
  // its page-locked copy; made by the first aa_outdata
  aa::Real *out_part = nullptr; double *out_mm_host = nullptr;
  bool prof = false;
  std::vector<ProfEntry> pe;
  std::vector<hipEvent_t> ev_pool;     // events of drained scopes, reused (a small Grid's step is ~25 scopes: creating 50 events per step showed)
};

// ---- profiling: an event pair around every kernel-chain stage, on the launch stream ----------
struct Scope {
  aa_grid *g; int id; hipEvent_t a = nullptr, b = nullptr;
  Scope(aa_grid *g_, const char *name) : g(g_), id(-1) {
    if (!g->prof) return;
    for (size_t i = 0; i < g->pe.size(); i++) if (g->pe[i].name == name) { id = (int)i; break; }
    if (id < 0) { g->pe.push_back(ProfEntry()); id = (int)g->pe.size() - 1; g->pe[id].name = name; }
    if (g->ev_pool.size() >= 2) { a = g->ev_pool.back(); g->ev_pool.pop_back(); b = g->ev_pool.back(); g->ev_pool.pop_back(); }
    else { hipEventCreate(&a); hipEventCreate(&b); }
    hipEventRecord(a, g->st);
  }
  ~Scope() {
    if (id < 0) return;
    hipEventRecord(b, g->st);
    g->pe[id].ev.push_back(a); g->pe[id].ev.push_back(b); g->pe[id].launches++;
  }
};

// ---- composite Grids (slabs.hip) -------------------------------------------------------------
struct SlabLink {
  int n = 0;
  std::vector<int> k0, nk, dev;            // first active plane (0-based, global), planes, HIP device of every slab
  std::vector<int> lo, hi;                 // neighbour slab below / above (-1: physical boundary)
  std::vector<aa::Real*> send[2], recv[2];     // halo buffers on every slab's device
  std::vector<hipEvent_t> packed, copied;  // slab's send buffers are full / slab has pulled its neighbours' buffers
  std::vector<bool> copied_valid;
  // The peer copies run on a stream of their own beside the slab's kernels, and the unpack is left to whoever reads
  // the ghost planes next (halo_finish): the integrator first sweeps the planes that hold no neighbour data
  // (aa_integrate_begin), the ion step and new_dt never read them.
  std::vector<hipStream_t> xfer;
  std::vector<hipEvent_t> unpacked;        // slab's recv buffers have been unpacked (free for the next copy)
  std::vector<bool> unpacked_valid;
  bool halo_due = false;                   // messages posted, ghost planes not yet written
  aa::DevScalars *hsc = nullptr;               // pinned: n
  std::vector<aa::Real*> dwords_all;           // device: n x AA_ION_WORDS on every slab
  std::vector<hipEvent_t> wdone;           // slab's words of the pass just queued are complete
  hipEvent_t gathered = nullptr;           // slab 0 holds every slab's words
  // no peer access between two neighbouring devices (or AA_SLAB_NO_PEER=1): the halo goes device -> pinned host -> device
  bool staged = false;
  std::vector<aa::Real*> hstage[2];            // pinned: the slab's two send buffers on the host
  std::vector<hipStream_t> xout;           // the slab's device -> host copies
  std::vector<hipEvent_t> staged_ev;       // ... are complete
  // the radiation sub-cycle's words: slab 0 <-> every slab.  Where peer access between device 0 and ANY slab's device is missing (checked at
  // create time for every pair, not only neighbours), or the halo is staged anyway, the words go through pinned host memory instead: every
  // slab copies its words into hwords[round & 1][s] behind its pass and, once all have, reads the whole set back -- no peer copy at all.
  // Two rounds of buffers: a slab can be one pick ahead of another, never two (its next pass waits for everybody's words of this one).
  bool words_staged = false;
  aa::Real *hwords[2] = {nullptr, nullptr};    // pinned: n x AA_ION_WORDS each
  unsigned wround = 0;
  size_t halo = 0;
  int home = 0;                            // the caller's current device when the handle was made
  // a level of a cut Mesh (aa_create_cut): the root's cuts K_0 .. K_ntotal, and the first root slab that holds zones of this level
  // (slab s of the handle lies over root slab s0 + s and lives on its device; slabs without zones of the level are absent)
  std::vector<int> cuts;
  int s0 = 0, ntotal = 0;
  bool by_cuts = false;                    // made by aa_create_cut (aa_mesh_create takes such handles, and only such)
  int kdisp = 0;                           // the level's x3 displacement, zones of the level
};

// every composite entry point leaves the caller's current HIP device as it found it
struct DevGuard { int d = -1; DevGuard() { if (hipGetDevice(&d) != hipSuccess) d = -1; } ~DevGuard() { if (d >= 0) (void)hipSetDevice(d); } };
int slabs_create(const aa_params *p, int nslab, aa_grid **out);
int slabs_bvals_local(aa_grid *g);   // the boundary conditions of every slab without the exchange between them
int slabs_halo_finish(aa_grid *g);    // the ghost planes of a posted x3 exchange are written (before anything reads them)
int slabs_halo_exchange(aa_grid *g);  // the x3 exchange between the slabs alone (no boundary condition)
int slabs_cfl_queue(aa_grid *g);      // new_dt's maxima of every slab on their way to link->hsc, no wait
void slabs_destroy(aa_grid *g);
int slabs_sync(aa_grid *g);
long long slabs_device_bytes(const aa_grid *g);
int slabs_upload_cons(aa_grid *g, const double *U);
int slabs_download_cons(aa_grid *g, double *U);
int slabs_upload_edgeflux(aa_grid *g, const double *ef);
int slabs_download_edgeflux(aa_grid *g, double *ef);
int slabs_set_grav_tables(aa_grid *g, const double *pc, const double *p1, const double *p2, const double *p3);
int slabs_set_cooling(aa_grid *g, int kind);
int slabs_set_pinned_cells(aa_grid *g, long long n, const long long *index, const double *values);
int slabs_apply_pinned_cells(aa_grid *g);
int slabs_add_radplane(aa_grid *g, int dir, double flux);
int slabs_bvals_mhd(aa_grid *g);
int slabs_bvals_mhd_side(aa_grid *g, int dir, int side);
int slabs_bvals_ionrad(aa_grid *g);
int slabs_new_dt_local(aa_grid *g, double *dt_cfl);
int slabs_cfl_max_v(aa_grid *g, double *v);
int slabs_integrate(aa_grid *g, int vl);
int slabs_ion_begin(aa_grid *g);
int slabs_ion_rates(aa_grid *g, double *dt_chem, double *dt_therm);
int slabs_ion_update(aa_grid *g, double dt, long long *cellcount, double *dt_hydro);
int slabs_ion_pass(aa_grid *g, int update, int sweep);
int slabs_ion_pick(aa_grid *g, int first, double limit);
int slabs_fetch_scalars(aa_grid *g);
int slabs_ion_finish(aa_grid *g);
int slabs_history(aa_grid *g, double *sums);
int slabs_dump_section(aa_grid *g, int fmt, int prim, int section, float *host_dst);
void outdata_release(aa_grid *g);     // outdata.hip: the minimum / maximum records of a Grid that is going away
void dump_release(aa_grid *g);        // dump.hip: the bounce buffer of a Grid that is going away
int dump_prepare(aa_grid *g);         // dump.hip: the bounce buffer, its stream and events, made on first use (shared with restart.hip)
int dump_stream(aa_grid *g);          // dump.hip: the stream of the dumps' copies alone, made on first use (the snapshots need no bounce buffer)
void rst_snapshot_free(aa_grid *g);   // restart.hip: the restart snapshot's buffers and events (dump_release, behind the wait for dump_st)
void dump_copy_out(float *dst, const float *src, size_t n);    // dump.hip: bounce buffer <-> the caller's memory on a few threads
int slabs_rst_section(aa_grid *g, int section, double *host, int put);
int rst_section_grid(aa_grid *g, int section, double *host, long long n, int put);   // restart.hip: the first n doubles of a section of one Grid
void slabs_push_state(aa_grid *g);
// evaluation of a StaticGravPot callback at zone centres and lower faces of a Grid (api.hip)
void aa_eval_grav_tables(const aa_params &p, const double dx[3], int N1, int N2, int N3, aa_gravpot_fn fn, std::vector<double> t[4]);
int aa_edgeflux_ready(aa_grid *g);    // fill GridS.EdgeFlux from the buffers of the one-kernel sub-cycle if that is still due
extern "C" int aa_download_cons_planes(aa_grid *g, int k_first, int nplanes, double *dst);
extern "C" int aa_download_edgeflux_planes(aa_grid *g, int nplanes, double *dst);

// hydro2d_kernels.hip: the update kernels of a 2-D Grid that is a level of a Mesh -- k2d_step<CTU2 | VL2> instantiated to also store the
// second-pass fluxes of the faces on the lines of `kp` into F (global momentum order; smr.hip k2d_flux_correct reads them)
namespace aa {
void launch_2d_ctu_flux2_update_keep(const DevGrid &g, Real dt, Real *edge, DevScalars *sc, const KeepPlanes &kp, hipStream_t st);
void launch_2d_vl_flux2_update_keep(const DevGrid &g, Real dt, Real *edge, DevScalars *sc, const KeepPlanes &kp, hipStream_t st);
}

// run.hip: the frame the run calls share -- aa_run_1d / aa_run_2d / aa_run_3d for a Grid, aa_mesh_run_2d / aa_mesh_run_3d (smr.hip) for a Mesh: the
// refusals of span and tlim, the loop over single steps (stepwise), else begin -> { batch, synchronise `st`, read the clock } while it
// is live -> the host's time / dt / nstep from the clock -> end.
struct RunOps {
  const char *who, *owner;             // the entry's name for its messages; "Grid" / "root": whose tlim new_dt clips at
  void *self;
  double *time, *dt; int *nstep;       // the host's MeshS
  double tlim;
  bool stepwise;
  int (*step)(void *self);             // one aa_step / aa_mesh_step
  int (*begin)(void *self, const RunClock &seed, double t_stop, double tlim, int nstep_stop, RunClock **clock);   // the clock buffers, the call's clock; *clock: the page-locked one the host reads
  int (*batch)(void *self, double t_stop, double tlim, int nstep_stop);   // the launches between two reads of the clock
  void (*end)(void *self);             // (may be null) the host's clock has been set
  hipStream_t st; int *host_syncs;
  // a history schedule this call has taken over (null: none; then nothing below is called and the call does what it did without):
  // stepwise, the frame applies hst_row_due on the host behind every step and hst_row takes every Grid's row from aa_history;
  // queued, hst_begin seeds the device's schedule behind `begin`, the batch queues k_history_dc / k_hst_row behind every step
  // (hst->active), and hst_drain takes the rows a batch left from the rings behind every synchronise
  HstRun *hst = nullptr;
  int (*hst_row)(void *self) = nullptr;
  int (*hst_begin)(void *self, int nstep) = nullptr;
  void (*hst_drain)(void *self) = nullptr;
};
int run_frame(const RunOps &o, double t_stop, double tlim, int nstep_stop, int *nsteps_done);
// run.hip: the pieces of a history schedule a Grid and a Mesh share -- the buffers of one Grid (`cap` rows in its ring) and of a
// schedule, made on first use and freed by hst_free_grid / hst_free_sched; a row of aa_history appended on the host; the rows of
// rounds [h.drained, mirror->nrows) from a Grid's ring; and the two launches (run.hip k_hst_seed, k_hst_row)
int hst_grid_buffers(aa_grid *g, int cap, const char *who);
int hst_sched_buffers(HstRun &h, const char *who);
void hst_free_grid(aa_grid *g);
void hst_free_sched(HstRun &h);
int hst_row_host(aa_grid *g, double time, double dt);
void hst_drain_grid(aa_grid *g, const HstRun &h);
void launch_hst_seed(HstRun &h, int nstep, hipStream_t st);
// ... behind launch_history_dc's `nb` partial rows of `g`: the row, if one is due; commit: this launch also moves the schedule on
// (the last of a Mesh's Grids; a stand-alone Grid's only one)
void launch_hst_row(aa_grid *g, int nb, const RunClock *clock, double tlim, const HstRun &h, bool commit, hipStream_t st);
// run.hip: the integrator's chain of a 2-D Grid on the device clock `rc`, on g->st (a level of a Mesh: the flux-keeping update kernel;
// sc == nullptr: without new_dt's maxima)
void queue_chain_2d(aa_grid *g, const aa::Run2D *rc, aa::DevScalars *sc);
// run.hip: whether a 3-D Grid's step is the chain whose kernels have entries on the device clock (everything aa_run_3d asks before it
// queues, but the batch): asked of a stand-alone Grid and of every level of a Mesh ...
bool on_queued_chain_3d(const aa_grid *g);
// ... that chain on the clock `rc`, on g->st (a level of a Mesh: the flux-keeping update kernel; sc == nullptr: without new_dt's maxima),
// and the boundary pass behind it
void queue_chain_3d(aa_grid *g, const aa::Run3D *rc, aa::DevScalars *sc);
void queue_bvals_3d(aa_grid *g);

// new state from outside (an upload, a restart section): the next ion step's speculating entry is the dense one
static inline void ion_lean_forget(aa_grid *g) { g->ion_lean_next = false; g->ion_prev_niter = 0; for (aa_grid *c : g->slab) c->ion_lean_next = false; }
static inline double bits_to_double(unsigned long long b) { double x; memcpy(&x, &b, 8); return x; }
static inline unsigned long long double_to_bits(double x) { unsigned long long b; memcpy(&b, &x, 8); return b; }
// new_dt's maxima as the kernels left them, for time_step.h
static inline void max_v_of(const aa::DevScalars &s, double *v) { for (int d = 0; d < 3; d++) v[d] = bits_to_double(s.max_v[d]); }
extern "C" int aa_fetch_scalars(aa_grid *g);     // DevScalars device -> pinned host, synchronous
// ionrad_3d.c:862-1012 for the Grid of one level (api.hip; the loop itself is ion_subcycle.h): root (finegrid 0, limit = its
// dt) or refined level (limit = the time the root covered); *dt_done_out = the time the sub-cycles covered
extern "C" int aa_ion_run(aa_grid *g, int finegrid, double limit, int *niter_out, double *dt_done_out);
// :1017-1029, :1044 the root level behind that loop (tcoarse: of a Mesh, else NULL)
static inline int ion_root_close(aa_grid *g, int niter, double dt_done, double *tcoarse)
{
  if (ion_close_root(niter, g->p.maxiter, dt_done, &g->dt, tcoarse))
    return aa_fail(-4, "[ion_radtransfer_3d]: dt = %e, dt_done = %e", g->dt, dt_done);
  return 0;
}
// one radiation sub-cycle with the step chosen on the device (api.hip); the multi-rank drivers need the reductions on the
// host and use aa_ion_rates / aa_ion_update
extern "C" int aa_ion_arm(aa_grid *g);
extern "C" int aa_ion_subcycle(aa_grid *g, double dt_done, double limit, double *dt, int *limit_hit, double *dt_chem,
                               double *dt_therm, long long *cellcount, double *dt_hydro);
