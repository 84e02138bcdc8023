/* include/athena_amd.h -- C-ABI of the MI355X-native hot path of Atmospheric Athena.
 *
 * Plain C, plain pointers and sizes; no torch / HIP types in any signature (a HIP stream is
 * passed as `void*`).  One `aa_grid` = one Grid of the reference (one slab of the root
 * Domain, resident on one GPU).  Every entry point names the reference interface it
 * replaces (paths under /root/reference/src).  All functions return 0 on success and a
 * negative code on error; `aa_last_error()` returns the message the reference would have
 * passed to ath_error() (utils.c:118).  Nothing here falls back to a CPU path: if the GPU
 * or the library is missing, creation fails.
 *
 * Host-side state is exchanged in the reference's own layout: `GridS.U` is one contiguous
 * block of ConsS {d,M1,M2,M3,E[,s0]} indexed [k][j][i] over Nx+2*nghost zones per direction
 * (athena.h:81-100,:290; ath_array.c:78-120) and `GridS.EdgeFlux` is [Nx3+1][Nx2+1][Nx1+1]
 * (init_grid.c:242-250).  On the device the state is struct-of-arrays.
 */
#ifndef ATHENA_AMD_H
#define ATHENA_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

enum { AA_NGHOST = 4 };                     /* defs.h.in:129-140 */
enum { AA_BC_NONE = 0, AA_BC_REFLECT = 1, AA_BC_OUTFLOW = 2, AA_BC_PERIODIC = 4 }; /* bvals_mhd.c:560-586 */

typedef struct aa_params {
  int    Nx[3];            /* active zones of this Grid: all > 1 (3-D), or Nx[2] == 1 with
                              Nx[0], Nx[1] > 1 (2-D: no ghost zones along x3, host block
                              U[1][Nx2+8][Nx1+8], init_grid.c:144-174), or Nx[1] == Nx[2] == 1 in a
                              1-D root Domain (1-D: host block U[1][1][Nx1+8])                   */
  int    rootNx[3];        /* active zones of the root Domain                                   */
  double xmin[3], xmax[3]; /* root Domain extent; dx = (xmax-xmin)/rootNx (init_mesh.c:225)     */
  double MinX[3];          /* lower edge of this Grid (init_grid.c:104-111)                     */
  int    bc[6];            /* ix1,ox1,ix2,ox2,ix3,ox3; AA_BC_NONE = neighbour Grid fills it     */
  int    nscal;            /* NSCALARS (0 or 1; 1 whenever ion != 0)                            */
  int    ion;              /* ION_RADIATION + ION_RADPLANE                                      */
  double gamma, cour_no, tlim;   /* <problem>gamma, <time>cour_no, <time>tlim (main.c:368-378)  */
  /* <ionradiation> block, ionrad_3d.c:742-757 */
  double sigma_ph, m_H, mu, e_gamma, alpha_C, k_B, time_unit;
  double max_de_iter, max_de_therm_iter, max_dx_iter;
  double max_de_step, max_de_therm_step, max_dx_step;
  double tfloor, tceil;
  int    maxiter;
  int    device;           /* HIP device ordinal                                                */
  int    integrator;       /* 0: CTU + H-correction (configure default + --enable-h-correction);
                              1: van Leer, no H-correction (--with-integrator=vl);
                              2: CTU without H-correction (configure default, NO_H_CORRECTION)  */
  int    level;            /* DomainS.Level (static mesh refinement): dx = root dx / 2^level
                              (init_mesh.c:245); 0 for a single-level run                      */
  int    order;            /* configure --with-order: 2 (or 0) piecewise linear, lr_states_plm.c;
                              3 piecewise parabolic, lr_states_ppm.c (CTU integrator only)    */
  int    ion_path;         /* radiation sub-cycle: 0 by size (one kernel from rays of 48 zones, or as
                              AA_ION_FUSED says), 1 the one-kernel form (aa_ion_pass ...), 2 the
                              two-kernel form (aa_ion_rates / aa_ion_update)                   */
  int    nslab;            /* > 1: this ONE Grid of the caller is cut into that many x3 slabs, one per
                              GPU (devices `device`, `device`+1, ... modulo the visible ones, or
                              AA_SLAB_DEVICES=0,1,..), behind this same interface: the library does
                              what init_mesh.c:583-620, bvals_mhd.c:423-493 and the MPI_Allreduce
                              calls of new_dt.c / ionrad_3d.c do for the reference's ranks.  0: one
                              GPU unless AA_NGPU is set in the environment; 1: one GPU          */
} aa_params;

typedef struct aa_grid aa_grid;

/* ---- lifecycle: init_grid.c (U, EdgeFlux), integrate_init_3d (integrate_3d_ctu.c:3374),
 *      ion_radtransfer_init_3d (ionrad_3d.c:739), ion_radtransfer_init (ionrad.c:64)      */
/* aa_params.nslab > 1 (or AA_NGPU=N in the environment): the handle stands for the caller's ONE Grid cut into N x3 slabs, one
 * per HIP device (AA_SLAB_DEVICES=0,1,.. or p->device, +1, .. modulo the visible ones; csrc/slabs.hip).  Root level only
 * (the levels of a Mesh on several devices come from aa_create_cut), >= 4 planes per slab, <= 64 slabs; aa_pack_x3 / aa_unpack_x3 / aa_set_stream return an error
 * on it and aa_halo_doubles 0 (the slabs exchange their halos themselves); the caller's current device is left unchanged. */
int         aa_create(const aa_params *p, aa_grid **out);
/* One level of a Mesh whose levels are ALL cut at the same root x3 planes, one slab stack per HIP device, in one process.  `p`
 * describes the caller's undivided Grid of the level (its Nx, MinX, bc, level), kdisp is its <domainN> kDisp in zones of the
 * level (0 for the root), cuts[0..nslab] the root planes K_0 = 0 < .. < K_nslab = rootNx3 (NULL: AA_SLAB_CUTS=0,..,Nx3 from the
 * environment if set, else the equal division aa_create uses).  The handle is a composite like aa_create's: slab s holds the level's zones over the root planes [K_s, K_s+1) and lives
 * on the device of the root's slab s (AA_SLAB_DEVICES, or p->device + s modulo the visible ones); a slab without zones of the
 * level is absent.  Everything a composite handle forwards works on it, scattered and gathered by k-plane range; gravity and
 * pinned-zone positions are those of the undivided Grid.  A piece thinner than nghost is an error that names the level, the slab
 * and the cut; bc[4] / bc[5] become AA_BC_NONE on interior cuts; a periodic root wraps.  Refused: 2-D Grids, a refined level
 * that is periodic along x3.  aa_mesh_create takes such handles (see there); plain aa_create keeps refusing level > 0 with
 * nslab > 1.  The arithmetic is csrc/mesh_cuts.h (plain C, no device). */
int         aa_create_cut(const aa_params *p, int kdisp, int nslab, const int *cuts, aa_grid **out);
void        aa_destroy(aa_grid *g);   /* integrate_destruct_3d :3498 */
const char *aa_last_error(void);
int         aa_set_stream(aa_grid *g, void *hip_stream);   /* run on a caller-owned stream */
int         aa_sync(aa_grid *g);
long long   aa_device_bytes(const aa_grid *g);

/* ---- state transfer (host view coherence points: problem(), Userwork_*, outputs) */
int aa_upload_cons(aa_grid *g, const double *U_aos);      /* host ConsS block -> device SoA */
int aa_download_cons(aa_grid *g, double *U_aos);
/* Only the ghost zones of the block (its active zones are left alone): for a caller whose host copy of the active zones is
 * current, i.e. nothing but aa_bvals_* / aa_new_dt ran on the device since the block last travelled either way.  The library keeps
 * track itself: if any call since the last aa_upload_cons / aa_download_cons wrote active zones (integrators, ion step, pinned
 * zones, restriction / flux correction) the whole block is downloaded instead. */
int aa_download_ghost_zones(aa_grid *g, double *U_aos);
int aa_upload_edgeflux(aa_grid *g, const double *ef);
int aa_download_edgeflux(aa_grid *g, double *ef);
int aa_get_mesh_state(const aa_grid *g, double *time, double *dt, int *nstep);  /* MeshS.time/dt/nstep */
int aa_set_mesh_state(aa_grid *g, double time, double dt, int nstep);

/* ---- hooks the problem file installs */
/* globals.h:24 StaticGravPot: the callback is evaluated ONCE on the host at cell centres and
 * face centres (cc_pos.c:36-43) and kept as device tables; pass NULL to remove it.           */
typedef double (*aa_gravpot_fn)(double x1, double x2, double x3);
int aa_set_static_grav_pot(aa_grid *g, aa_gravpot_fn fn);
int aa_set_static_grav_tables(aa_grid *g, const double *phi_cc, const double *phi_f1,
                              const double *phi_f2, const double *phi_f3); /* [N3][N2][N1] each */
/* globals.h:25 CoolingFunc (optically thin cooling in integrate_3d_ctu.c: Steps 1c-3c :359-368 / :662-671 / :846-855 on the L/R
 * states, 8b :2133-2266 P^{n+1/2}, 11c :2943-2953 the energy).  The reference calls a host function pointer per state; a device
 * integrator needs the function itself, so the library carries the one the reference ships: AA_COOL_KOYINUT = KoyInut
 * (microphysics/cool.c:48, cgs units).  CTU integrator only -- the reference's integrate_3d_vl.c has no cooling terms.         */
#define AA_COOL_NONE    0
#define AA_COOL_KOYINUT 1
int aa_set_cooling(aa_grid *g, int kind);
/* configure --enable-fofc (FIRST_ORDER_FLUX_CORRECTION, integrate_3d_vl.c): a second-order flux that came out NaN is replaced by
 * the predictor flux of its face (Step 10); after the full update a zone with d < 0 (or P < 0) is repaired with the predictor
 * fluxes, and so are its neighbours across the faces they share (Step 14, FixCell) -- the reference's scan, in its order.  Off
 * by default; with it off a step is what it was.  van Leer integrator, second order, one Grid on one device: refused for the CTU
 * integrator, third-order reconstruction, the Grids of an aa_mesh and Grids cut into slabs (no reference build pins those).  More
 * than 4096 zones with d < 0 in one step fail the step.  aa_get_fofc_counts: out[0..2] = zones that had d < 0, zones that had
 * P < 0 (Cons_to_Prim floors P: stays 0), second-order fluxes replaced, of the last aa_integrate_3d_vl.                    */
int aa_set_fofc(aa_grid *g, int on);
int aa_get_fofc(const aa_grid *g);
int aa_get_fofc_counts(const aa_grid *g, long long out[3]);
/* Userwork_in_loop of prob/ioniz_sphere.c:255-306 re-imposes fixed values on a fixed set of
 * cells every step; the device-side equivalent is a list of pinned cells (linear index into
 * the [k][j][i] block incl. ghosts, nvar values each) applied after the integrator.          */
int aa_set_pinned_cells(aa_grid *g, long long n, const long long *index, const double *values);
int aa_apply_pinned_cells(aa_grid *g);
/* ionradplane_3d.c:56 add_radplane_3d (called by problem()); dir = -1 (rays along +x1) or -2 (along +x2: two-kernel
 * sub-cycle).  dir = -3 and dir > 0 are refused: the reference has no defined behaviour for them. */
int aa_add_radplane_3d(aa_grid *g, int dir, double flux);
int aa_has_radplane(const aa_grid *g);   /* main.c:546 `radplanelist[0].nradplane > 0`: whether a step includes the ion step */

/* ---- the reference's per-step call sites */
int aa_bvals_mhd(aa_grid *g);                       /* bvals_mhd.c:174 (physical BCs only)        */
int aa_bvals_mhd_side(aa_grid *g, int dir, int side); /* one (*BCFun)(pGrid) call of bvals_mhd.c:196-420:
                                                        dir 0..2, side 0 inner / 1 outer; for drivers that
                                                        interleave user boundary functions (bvals_mhd_fun :917) */
int aa_bvals_ionrad(aa_grid *g);                    /* bvals_ionrad.c:63                          */
int aa_new_dt(aa_grid *g);                          /* new_dt.c:32                                */
int aa_integrate_3d_ctu(aa_grid *g);                /* integrate_3d_ctu.c:110, dt = Grid dt       */
int aa_integrate_3d_vl(aa_grid *g);                 /* integrate_3d_vl.c:96 (NO_H_CORRECTION)     */
/* A 2-D Grid (Nx[2] == 1; integrate.c:49-58 picks these by dimension, and so do aa_start / aa_step): HYDRO, ADIABATIC, second
 * order (third order: aa_set_order_2d below), no gravity / cooling / scalars / ion radiation / fofc / Mesh / slabs (each refused with a
 * message: no reference target pins them in 2-D).  cour_no may exceed 0.5 with the CTU integrator, not with van Leer (integrate.c:55-57).  The 3-D entry points
 * return an error on a 2-D Grid and these on a 3-D one.                                                                        */
int aa_integrate_2d_ctu(aa_grid *g);                /* integrate_2d_ctu.c (integrator 0: + H-correction, 2: without) */
int aa_integrate_2d_vl(aa_grid *g);                 /* integrate_2d_vl.c (NO_H_CORRECTION)        */
/* Third-order reconstruction on a 2-D Grid (configure --with-order=3: lr_states_ppm.c under integrate_2d_ctu.c / integrate_2d_vl.c),
 * opt-in: aa_params.order = 3 stays refused by aa_create on a 2-D Grid, as it always was; a Grid created at order 2 is switched here.
 * order: 2 or 3.  Call it behind aa_create, before aa_start / aa_resume / the first step and before aa_mesh_create_2d.  Off (2) by
 * default; with it off every launch is what it was.  At 3, aa_integrate_2d_ctu / _vl, aa_step and aa_run_2d run the third-order
 * instantiations of the kernels that reconstruct (the CTU first pass; the van Leer corrector, without tracing: lr_states_ppm.c:502-507);
 * nothing is allocated: the four ghost zones are exactly what the five-zone stencil of the first pass reads.  Errors, each with a
 * message that begins "[aa_set_order_2d]": a 1-D or 3-D Grid (those take aa_params.order), a value other than 2 or 3, integrator = 2
 * (CTU without H-correction: no third-order reference build pins it), a Grid that has already stepped, a Grid that belongs to an
 * aa_mesh.  aa_get_order_2d: the effective order of a 2-D Grid, aa_params.order (0 reads as 2) of any other.                          */
int aa_set_order_2d(aa_grid *g, int order);
int aa_get_order_2d(const aa_grid *g);
/* A 1-D Grid (Nx[1] == Nx[2] == 1 and rootNx[1] == rootNx[2] == 1; integrate.c:36-47): HYDRO, ADIABATIC, second or third order,
 * no gravity / cooling / scalars / ion radiation / fofc / Mesh / slabs (each refused with a message that says 1-D).  cour_no has
 * no limit with the CTU integrator and must be <= 0.5 with van Leer (integrate.c:41-44).  Integrators 0 and 2 are the same code:
 * integrate_1d_ctu.c has no H-correction.  A one-row cut of a 2-D or 3-D root Domain is refused, and so is Nx[0] < 4.                                */
int aa_integrate_1d_ctu(aa_grid *g);                /* integrate_1d_ctu.c                         */
int aa_integrate_1d_vl(aa_grid *g);                 /* integrate_1d_vl.c                          */
/* Many steps of a 1-D Grid in ONE launch (csrc/hydro1d_kernels.hip k1d_run): whole passes of main.c:519-669 -- integrate, nstep++,
 * time += dt, bvals_mhd, new_dt with the clip at `tlim` (new_dt.c:183-185) -- until time >= t_stop, nstep == nstep_stop (the
 * Grid's absolute step count; at most 2^20 steps ahead) or dt <= 0.  The Grid must have been started (aa_start / aa_resume).  The
 * same bits as that many aa_step calls.  *nsteps_done: steps taken.  An error on a Grid that is not 1-D, has more than
 * aa_run_1d_cap() active zones (one workgroup's LDS), or has pinned zones.  AA_1D_RESIDENT=0 in the environment at aa_create:
 * the same call steps one launch at a time.  aa_run_1d, aa_run_2d and aa_run_3d are one body (csrc/run.hip) with the rule of csrc/time_step.h;
 * the first of them that reaches the device makes the Grid's clock (one page-locked time / dt / nstep / "live" record for both,
 * and the 2-D / 3-D call's copy in device memory); a Grid that never calls them allocates none.                                     */
int aa_run_1d(aa_grid *g, double t_stop, double tlim, int nstep_stop, int *nsteps_done);
/* Many steps of a 2-D Grid per host visit (csrc/hydro2d_kernels.hip k2d_advance): the same loop and the same stop rules as aa_run_1d,
 * with the time step picked on the device -- AA_2D_BATCH steps (environment at aa_create; default 32) are queued as plain launches,
 * then the host reads time / dt / nstep / "stopped" ONCE and queues again while the run is live; steps queued behind the stop store
 * nothing.  The same bits as that many aa_step calls.  An error on a Grid that is not 2-D, has pinned zones or is a level of an
 * aa_mesh, for tlim other than the Grid's, and for nstep_stop outside nstep .. nstep + 2^20.  AA_2D_BATCH=0: the same call steps
 * one aa_step at a time.                                                                                                        */
int aa_run_2d(aa_grid *g, double t_stop, double tlim, int nstep_stop, int *nsteps_done);
int aa_run_2d_batch(const aa_grid *g);              /* steps queued per read-back on this Grid (0: one aa_step at a time; not 2-D: 0) */
/* Many steps of a 3-D hydro Grid per host visit (csrc/hydro_kernels.hip k3d_advance): the signature, loop and stop rules of aa_run_2d.
 * AA_3D_BATCH steps (environment at aa_create; default 8) of the chain aa_integrate_3d_ctu launches by default -- integrators 0 and
 * 2, second or third order, NSCALARS 0 or 1, with or without a static potential -- are queued as plain launches whose kernels read
 * dt and dt/dx from a clock in device memory; the host reads that clock once per batch.  The same bits as that many aa_step calls.
 * What the chain does not cover takes those aa_step calls inside the same call (aa_run_3d_batch() == 0): the van Leer integrator and
 * fofc, a cooling function, ion radiation, AA_CORRECT_ALL off (the default below 4e5 zones), AA_X3_FUSED=0, AA_FUSED_UPDATE=0,
 * AA_CFL_FUSED=0, AA_EDGE_OVERLAP=1, a pending aa_integrate_begin, fewer than AA_NGHOST zones along a direction, AA_3D_BATCH=0.
 * An error on a Grid that is 1-D or 2-D (they have their own calls), has pinned zones, is cut into slabs or is a level of an
 * aa_mesh, for tlim other than the Grid's, and for nstep_stop outside nstep .. nstep + 2^20.                                   */
int aa_run_3d(aa_grid *g, double t_stop, double tlim, int nstep_stop, int *nsteps_done);
int aa_run_3d_batch(const aa_grid *g);              /* steps queued per read-back on this Grid (0: one aa_step at a time; not 3-D: 0) */
/* History rows of the NEXT aa_run_2d / aa_run_3d call, made without a stop: arms the schedule of one <outputN> block with out_fmt = hst
 * -- its next time `t_next`, its spacing `dt_out`, the loop's nlim (< 0: none) -- for that call alone; the call disarms it whatever it
 * returns, the caller keeps the block's state.  Behind every step the call takes, data_output(&Mesh, 0) of the following pass is
 * applied for that block (csrc/time_step.h hst_row_due: main.c:524, output.c:509-512): if the loop goes on -- time < tlim, nstep below
 * nlim -- and time >= t_next, a row {time, dt, the nine sums of aa_history} is made and t_next += dt_out ONCE.  No row behind the
 * step that ends the loop (the forced output writes that one); a step that merely ends the CALL (t_stop, the span) is not that end.
 * Queued (csrc/history_dc.hip k_history_dc, csrc/run.hip k_hst_row: two more launches per queued step, which store nothing unless a
 * row is due; the rows reach the host with the clock, once per batch) or step by step inside the call (aa_history behind aa_step):
 * the same rows, bit for bit.  An error on a 1-D Grid (aa_run_1d keeps its loop in one launch and would add in another order), a
 * Grid cut into slabs, a level of an aa_mesh.  aa_run_hst_rows: up to `cap` rows of AA_HST_ROW doubles of the last armed call into
 * `rows` (may be NULL), their number into *nrows, the schedule's next time behind them into *t_next.                           */
#define AA_HST_ROW 11
int aa_run_hst_arm(aa_grid *g, double t_next, double dt_out, int nlim);
int aa_run_hst_rows(aa_grid *g, int cap, double *rows, int *nrows, double *t_next);
int aa_run_1d_cap(void);                            /* most active zones aa_run_1d keeps resident */
int aa_step_1d_block(void);                         /* TEST HOOK: active zones per block of the per-step kernel (the fixtures'
                                                       sizes sit either side of it); nothing in the product calls it */
int aa_ion_radtransfer_3d(aa_grid *g, int *niter);  /* ionrad_3d.c:862; may shrink the Grid dt    */
int aa_start(aa_grid *g);                           /* main.c:412-451: bvals, bvals_ionrad, new_dt */
int aa_step(aa_grid *g, int *niter);                /* one pass of main.c:519-669                 */

/* ---- phases, for drivers that interleave neighbour exchange / global reductions
 *      (the places where the reference calls MPI)                          */
/* The part of integrate_3d_ctu that reads none of the x3 neighbours' planes (the first-pass x1 / x2 sweeps of the
 * planes ks..ke, integrate_3d_ctu.c:196-620): call it between posting the x3 halo (bvals_mhd.c:423-493) and waiting
 * for it; aa_integrate_3d_ctu then does the rest.  Same bits with or without; a no-op where the split does not apply. */
int aa_integrate_begin(aa_grid *g);      /* (aa_upload_cons, aa_download_cons and aa_history between the two calls are allowed:
                                           * they stage through the face-state area and make the integrator redo these sweeps) */
/* new_dt.c:72-140 inside the integrator: with on != 0 the caller promises that between aa_integrate_3d_ctu / _vl and the
 * next aa_new_dt_local / aa_cfl_max_v nothing but aa_apply_pinned_cells changes the active zones (the order of main.c:572-629
 * when Userwork_in_loop only pins zones); the update kernel then leaves max(|v_d| + a) behind while the new state is in
 * registers and new_dt reads it instead of sweeping the Grid again.  aa_step does this by itself.                     */
int aa_cfl_in_update(aa_grid *g, int on);
int aa_new_dt_local(aa_grid *g, double *dt_cfl);                /* new_dt.c:72-170 before Allreduce */
/* ionrad.h:38 MAXCELLCOUNT: the root's sub-cycle loop ends (check_range, ionrad_3d.c:982) when more cells than this, summed
 * over all ranks, have left their allowed range -- for a driver that runs the loop itself around aa_ion_rates / aa_ion_update */
#define AA_MAXCELLCOUNT 20
int aa_ion_begin(aa_grid *g);                                   /* ionrad_3d.c:896-905            */
int aa_ion_rates(aa_grid *g, double *dt_chem, double *dt_therm);/* :922-938 before Allreduce      */
int aa_ion_update(aa_grid *g, double dt, long long *cellcount, double *dt_hydro); /* :965-1002    */
/* Before the first aa_ion_pass of an ion step (after aa_ion_begin): `limit` = the value aa_ion_pick will be given.  The
 * first pass then also applies the first sub-cycle's update with that whole step (the zone is in registers); where the
 * reduction confirms the step -- a quiet radiation field, ONE sub-cycle per hydro step -- the closing update pass has nothing
 * left to do; otherwise the next pass restarts from the state the entry saved.  Same results bit for bit; optional
 * (AA_ION_SPECULATE=0 in the environment turns it off). */
int aa_ion_speculate(aa_grid *g, double limit);
/* The same loop for Grids that run the ONE-KERNEL sub-cycle (aa_ion_is_fused: rays of 48 zones or more; the two
 * calls above refuse such a Grid).  The loop is cut at its only true barrier, the reduction that yields the step:
 * pass n applies update(n-1) and runs sweep(n) + rates(n) on the updated zones; its reduction words (MIN dt_chem,
 * MIN dt_therm, MAX (|v|+a)/dx, SUM cells out of range, OR negative-dt_chem -- the operands of the reference's four
 * MPI_Allreduce calls ionrad_3d.c:275,399,554,672) land in DEVICE memory, AA_ION_WORDS doubles per rank.  aa_ion_pick
 * (a one-thread kernel) folds the words of all ranks, books the update just applied -- the time covered so far stays on
 * the device -- and picks the next step; a pass whose step was cut back to the limit skips its sweep by itself.  So a
 * multi-rank driver issues ONE all-gather per sub-cycle on the Grid's stream and the host reads back ONCE per sub-cycle:
 *   aa_ion_begin; aa_ion_pass(0,1); [all-gather]; aa_ion_pick(first=1);
 *   repeat: aa_ion_pass(1,1); [all-gather]; aa_ion_pick(first=0); aa_ion_fetch -> step, limit flag and stop criteria of
 *           the update that pass applied; the reference's stop tests (:974-1002);
 *   aa_ion_finish (GridS.EdgeFlux of the last sweep that counted; the one after a stop was speculative).       */
#define AA_ION_WORDS 8
int aa_ion_is_fused(const aa_grid *g);
int aa_ion_pass(aa_grid *g, int update, int sweep, double *dev_words);
int aa_ion_pick(aa_grid *g, const double *dev_words_all, int nranks, int first, double limit);
int aa_ion_fetch(aa_grid *g, double *dt, int *limit_hit, double *dt_chem, double *dt_therm, long long *cellcount,
                 double *dt_hydro, int *neg_dt_chem);
int aa_ion_finish(aa_grid *g);
/* The speculating first pass has two forms (AA_ION_LEAN; same results bit for bit): n[0], n[1] = first passes queued so far in the dense
 * and in the lean form, n[2] = lean ones the pick refuted, which were then redone densely.  Waits for the Grid's stream.            */
int aa_ion_lean_counts(aa_grid *g, long long *n);
/* Sub-cycles per host visit.  aa_ion_radtransfer_3d, aa_step and every level of an aa_mesh run the loop above inside the library;
 * with K = ion_batch > 1 the stop tests (:982-1012) are applied on the device by the pick itself, a visit queues up to K
 * sub-cycles whose kernels leave at once behind a stop, and the host reads back once per visit instead of once per sub-cycle.
 * Same results bit for bit.  The first visit of an ion step is as long as the Grid's previous ion step was (at most K; 1 after
 * aa_create, an upload or a restart section), so a step behind a one-sub-cycle step makes the launches it made with K = 1.
 * K: AA_ION_BATCH in the environment at aa_create, 1 .. AA_ION_BATCH_MAX, default 1 = a read-back per sub-cycle; anything else
 * is refused.  Taken by Grids that run the one-kernel sub-cycle on one device with the fused pick (aa_ion_batch_active); the
 * others -- the two-kernel sub-cycle, AA_ION_FUSE_PICK=0, a Grid cut into slabs, aa_ion_radtransfer_3d_gather -- keep the
 * per-sub-cycle loop whatever K is.  aa_ion_batch_counts: n[0] host visits, n[1] sub-cycles executed, n[2] queued sub-cycles
 * that left at once, of the queued loop since aa_create. */
#define AA_ION_BATCH_MAX 256
int aa_set_ion_batch(aa_grid *g, int k);
int aa_ion_batch(const aa_grid *g);
int aa_ion_batch_active(const aa_grid *g);
int aa_ion_batch_counts(const aa_grid *g, long long *n);
/* ion_radtransfer_3d (ionrad_3d.c:862-1047, root level) of a rank of a multi-rank run in ONE call: the loop above with the
 * driver's collective as a callback.  `gather(ctx)` must all-gather this rank's AA_ION_WORDS doubles at dev_words into
 * dev_words_all (nranks x AA_ION_WORDS, DEVICE memory) on the Grid's stream and return 0; it is called once per pass, between
 * aa_ion_pass and aa_ion_pick.  pGrid->dt (aa_get_mesh_state) is cut back as the reference does (:985-1000, :1019-1023).
 * gather == NULL: one rank (dev_words / dev_words_all may be NULL).  Needs the one-kernel sub-cycle (aa_ion_is_fused). */
typedef int (*aa_gather_fn)(void *ctx);
int aa_ion_radtransfer_3d_gather(aa_grid *g, double *dev_words, const double *dev_words_all, int nranks, aa_gather_fn gather,
                                 void *ctx, int *niter);
int aa_host_syncs(aa_grid *g, int reset);   /* stream synchronisations that returned scalars to the host so far */
/* x3 halo: pack_ix3/pack_ox3/unpack_* (bvals_mhd.c:2608-3175).  side 0 = inner (ks..ks+3),
 * side 1 = outer; buffers are DEVICE pointers of aa_halo_doubles() doubles.                */
long long aa_halo_doubles(const aa_grid *g);
int aa_pack_x3(aa_grid *g, int side, double *dev_buf);
int aa_unpack_x3(aa_grid *g, int side, const double *dev_buf);
/* x2 x x3 pencils (init_mesh.c:526-620 NGrid_x2 x NGrid_x3; x1 is never cut: the rays): the x2 halo, four rows x all i incl.
 * the x1 ghost zones x the ACTIVE k-planes (bvals_mhd.c:2462 pack_ix2 / pack_ox2, :2896 unpack_ix2 / unpack_ox2).  A bvals_mhd
 * call of such a driver: aa_bvals_mhd_side for x1; this exchange and aa_bvals_mhd_side for the physical x2 sides; then x3. */
long long aa_halo_doubles_x2(const aa_grid *g);
int aa_pack_x2(aa_grid *g, int side, double *dev_buf);
int aa_unpack_x2(aa_grid *g, int side, const double *dev_buf);
/* The same halos through HOST buffers, for a driver that moves them itself (the reference's own MPI ranks linked on the shim:
 * MPI_Isend / MPI_Irecv of bvals_mhd.c:296-493): dir 1 = x2, 2 = x3; aa_halo_doubles_dir doubles per buffer. */
long long aa_halo_doubles_dir(const aa_grid *g, int dir);
int aa_halo_get(aa_grid *g, int dir, int side, double *host_buf);        /* pack_i* (side 0) / pack_o* (side 1) -> host_buf */
int aa_halo_put(aa_grid *g, int dir, int side, const double *host_buf);  /* host_buf -> the ghost planes of that side      */
int aa_device_count(void);                                               /* visible HIP devices (0: none)                  */

/* ---- static mesh refinement (reference built with --enable-smr): nested levels, all resident on one GPU.
 *      levels[] holds one Grid per Domain in the order of the reference's loops (MeshS.Domain[nl][nd], athena.h:355-361):
 *      level by level from the root, Domains of a level in deck order (they neither overlap nor touch, init_mesh.c:398-418;
 *      up to three children per Grid).  Each was created with aa_params.level = its level, Nx = the
 *      Domain's zones, MinX = its lower edge (init_mesh.c:281-286), bc = 0 on fine/coarse sides
 *      (bvals_mhd.c:193-361 ProlongateLater); disp[3*g+d] = <domainN> iDisp/jDisp/kDisp in zones
 *      of its level.  Fill every level (problem(), hooks) before aa_mesh_start().  The Mesh takes
 *      over the levels' streams; destroy it before the levels.                               */
typedef struct aa_mesh aa_mesh;
int  aa_mesh_create(int nlevels, aa_grid **levels, const int *disp, aa_mesh **out); /* init_grid.c overlap
                                                          tables (:150-560) + SMR_init (smr.c:2931)  */
/* A Mesh on several devices in ONE process: all levels made by aa_create_cut on the same cuts and devices, one Domain per level.
 * Inside there is one local stack per device (the aa_mesh_create_local machinery, all pieces of a device on one stream) plus
 * what crosses slabs: the x3 halo of every level (peer copies ordered by events, or pinned host memory where peer access is
 * refused or AA_SLAB_NO_PEER=1; where all levels exchange in a row -- the end of aa_mesh_step, aa_mesh_start -- ONE pack launch
 * per slab, ONE copy per neighbour and ONE unpack launch per slab for all levels two slabs share; AA_MESH_HALO_BATCH=0: one
 * exchange per level), the flux correction of a parent plane across a cut, new_dt's maxima (one wait per step) and the
 * radiation sub-cycle's words per level.  Every aa_mesh_* function below works on it with the same signature, except
 * aa_mesh_set_stream (an error, as aa_set_stream on a composite).  The levels integrate one after the other (AA_MESH_OVERLAP
 * does not apply).  Refused by name: mixed plain / composite levels, composites of plain aa_create, different cuts or devices,
 * several Domains on a level, 2-D Grids, fofc, aa_mesh_create_local on composites.                                            */
int  aa_mesh_nslab(const aa_mesh *m);                                /* slabs of a cut Mesh (1: an undivided Mesh)    */
int  aa_mesh_halo_counts(const aa_mesh *m, long long out[3]);       /* all-level x3 exchanges of a cut Mesh so far: pack +
                                                          unpack launches, copies, exchanges                         */
/* The same contract for Grids that are all 2-D (Nx3 = 1; the reference's tst/2D-hydro/athinput.blast has three levels):
 * disp[3*g+2] must be 0, and the nesting rules of init_mesh.c:320-499 hold in x1 and x2.  Every aa_mesh_* function below works
 * on such a Mesh except the radiation ones, which return an error; aa_mesh_step runs aa_integrate_2d_ctu / _vl, and
 * aa_mesh_new_dt carries max_v1 and max_v2 only.  cour_no up to the reference's 0.8 with CTU, <= 0.5 with van Leer.  Refused:
 * a 3-D Grid among the levels (aa_mesh_create is the 3-D constructor, as this one refuses there), levels of mixed
 * integrators, integrator = 2 (no reference build with --enable-smr and without H-correction), a Grid with fofc on.  Third order
 * (aa_set_order_2d on every Grid BEFORE this call): accepted where ALL levels are at order 3 with integrator = 0; refused: levels of
 * mixed order, and van Leer levels at order 3 (no reference build with --enable-smr, --with-order=3 and the van Leer integrator). */
int  aa_mesh_create_2d(int nlevels, aa_grid **levels, const int *disp, aa_mesh **out);
void aa_mesh_destroy(aa_mesh *m);
int  aa_mesh_get_state(const aa_mesh *m, double *time, double *dt, int *nstep);     /* MeshS          */
int  aa_mesh_set_state(aa_mesh *m, double time, double dt, int nstep);
int  aa_mesh_set_stream(aa_mesh *m, void *hip_stream);
int  aa_mesh_restrict_correct(aa_mesh *m);        /* smr.c:1207 RestrictCorrect                      */
int  aa_mesh_restrict_correct_pair(aa_mesh *m, int l); /* its step for one pair: level l+1 -> level l  */
int  aa_mesh_ionrad_restrict_correct(aa_mesh *m); /* smr.c:85 ionradRestrictCorrect                  */
int  aa_mesh_prolongate(aa_mesh *m);              /* smr.c:2359 Prolongate                           */
int  aa_mesh_new_dt(aa_mesh *m);                  /* new_dt.c:32 over all levels                     */
int  aa_mesh_ion_radtransfer(aa_mesh *m, int level, int *niter); /* ionrad_3d.c:862 on Domain[level],
                                                     incl. ionrad_prolong_rcv/_snd (ionrad_smr.c)   */
int  aa_mesh_ionflux_prolong(aa_mesh *m, int level); /* ionrad_prolong_snd(level-1) + _rcv(level) alone    */
int  aa_mesh_start(aa_mesh *m);                   /* main.c:395-447                                  */
int  aa_mesh_step(aa_mesh *m, int *niter);        /* one pass of main.c:519-669; niter[nlevels]      */
/* Many passes of aa_mesh_step's loop per host visit for a Mesh of 2-D Grids (aa_mesh_create_2d): the semantics of aa_run_2d -- until
 * time >= t_stop, nstep == nstep_stop (the Mesh's absolute step count, 0 .. 2^20 steps ahead) or dt <= 0 -- with ONE clock in device
 * memory for all levels.  AA_2D_BATCH steps (environment when the Mesh is made; the Mesh has a default of its own,
 * csrc/hydro2d_launch.h) are queued as plain launches: the integrator chain of every level, restriction and flux correction,
 * new_dt's maxima, one wavefront that advances the clock over all levels (k2d_mesh_advance; csrc/time_step.h), bvals_mhd,
 * prolongation; then the host reads the clock ONCE and queues again while the run is live.  Steps queued behind the stop change
 * nothing.  The same bits as that many aa_mesh_step calls; afterwards the Mesh's and every level's time / dt / nstep are set as
 * aa_mesh_new_dt leaves them.  *nsteps_done: steps taken.  An error, each message beginning [aa_mesh_run_2d]: a null Mesh, a Mesh
 * of 3-D Grids, a Mesh made by aa_mesh_create_local or cut into slabs, a level with pinned zones, a tlim other than the root's,
 * nstep_stop outside nstep .. nstep + 2^20.  AA_2D_BATCH=0: the same call loops over aa_mesh_step; so it does on a Mesh with more
 * Grids than the advance kernel's argument table holds (16, the most a Mesh can have today) or with a level of fewer than four
 * zones along a direction.  aa_run_2d on a level of a Mesh stays an error.                                                        */
int  aa_mesh_run_2d(aa_mesh *m, double t_stop, double tlim, int nstep_stop, int *nsteps_done);
int  aa_mesh_run_2d_batch(const aa_mesh *m);      /* steps queued per read-back on this Mesh; 0: it steps one at a time */
/* The 3-D twin, for a Mesh of 3-D Grids (aa_mesh_create) on one device: the semantics of aa_mesh_run_2d with AA_3D_BATCH steps
 * (environment when the Mesh is made, 0 or 1..1024; the Mesh has a default of its own, csrc/hydro3d_launch.h) queued per read of
 * the clock.  A queued step is aa_mesh_step's order on the Mesh's one stream: the default CTU chain of every level with dt and the
 * ratios dt/dx of ITS zones from the device clock (every Grid has a clock record of its own in one device array; the update
 * kernel keeps the second-pass fluxes of the level boundaries), restriction and flux correction finest pair first, new_dt's
 * maxima, one wavefront that advances the clock over all levels (k3d_mesh_advance; csrc/time_step.h), bvals_mhd, prolongation.
 * The same bits as that many aa_mesh_step calls.  An error, each message beginning [aa_mesh_run_3d]: a null Mesh, a Mesh of 2-D
 * Grids, a Mesh made by aa_mesh_create_local or cut into slabs, a level with pinned zones, a tlim other than the root's,
 * nstep_stop outside nstep .. nstep + 2^20.  The same call loops over aa_mesh_step, with the same results, when any level is off
 * the chain aa_run_3d queues for a Grid: AA_3D_BATCH=0, the van Leer integrator, a cooling function, ion radiation, the tile kernels
 * of a small level (AA_CORRECT_ALL off: the default below 4e5 zones), AA_X3_FUSED=0, AA_FUSED_UPDATE=0, AA_CFL_FUSED=0,
 * AA_EDGE_OVERLAP=1, fewer than four zones along a direction, more Grids than the advance kernel's table holds (16), a kernel
 * combination this build does not instantiate.  aa_run_3d on a level of a Mesh and aa_mesh_run_2d on a 3-D Mesh stay errors.      */
int  aa_mesh_run_3d(aa_mesh *m, double t_stop, double tlim, int nstep_stop, int *nsteps_done);
int  aa_mesh_run_3d_batch(const aa_mesh *m);      /* steps queued per read-back on this Mesh; 0: it steps one at a time */
/* aa_run_hst_arm / aa_run_hst_rows for the next aa_mesh_run_2d / aa_mesh_run_3d call: ONE schedule for the Mesh (a block's time and
 * spacing are shared by its levels), the rule applied to the Mesh's clock, a row of every Grid where one is due -- `grid`: the
 * Grid's index in the Mesh's order; all Grids have the same number of rows.  An error on a Mesh cut into slabs and on one made by
 * aa_mesh_create_local.                                                                                                      */
int  aa_mesh_run_hst_arm(aa_mesh *m, double t_next, double dt_out, int nlim);
int  aa_mesh_run_hst_rows(aa_mesh *m, int grid, int cap, double *rows, int *nrows, double *t_next);

/* Multi-GPU SMR: every level is cut into x3 slabs at the SAME root planes, so that restriction, the
 * radiation hand-off and prolongation stay inside a rank.  aa_mesh_create_local builds one rank's stack
 * of slabs from explicit links (21 ints per link l: cs[3] = first parent zone under the child slab as a
 * local index incl. ghosts, n[3] parent zones, prol[6] = that side of the child slab is a fine/coarse
 * boundary of the LEVEL, corr[6] = the parent zone outside that side is on this rank, cdisp[3] = child
 * origin - 2 x parent origin).  Where a level ends exactly at a cut (prol=1, corr=0 on an x3 side) the
 * parent plane outside belongs to the neighbouring rank: the child's restricted boundary flux travels
 * as a message of (Nx1/2)(Nx2/2) x 6 doubles (smr.c:1592-1640 is the same message under MPI).        */
int  aa_mesh_create_local(int nlevels, aa_grid **levels, const int *links, aa_mesh **out);
int  aa_flux_x3_export(aa_grid *child, int side, double *dev_buf);   /* side 0 lower / 1 upper boundary */
int  aa_flux_x3_apply(aa_grid *parent, int side, int i0, int j0, int n1, int n2, const double *dev_buf);
int  aa_cfl_max_v(aa_grid *g, double v[3]);       /* new_dt.c:72-140 of one Grid (the MAX over the slabs of
                                                     a level and the carry from level to level are the driver's) */

/* ---- function-level kernels on device arrays' host mirrors (parity tests): n states of
 *      nvar = 5+nscal doubles each, same conventions as fluxes()/lr_states()              */
int aa_test_fluxes(int nscal, double gamma, int n, const double *Ul, const double *Ur,
                   const double *etah, double *F);                      /* roe.c:59        */
int aa_test_lr_states(int nscal, double gamma, int n, const double *W, double dt, double dx,
                      int il, int iu, double *Wl, double *Wr);          /* lr_states_plm.c:62 */
int aa_test_lr_states_ppm(int nscal, double gamma, int n, const double *W, double dt, double dx,
                          int il, int iu, double *Wl, double *Wr);      /* lr_states_ppm.c:91  */

int aa_test_xdiv(int n, const double *a, const double *b, double *out);  /* csrc/hydro_dev.h x_div / x_sqrt beside the compiler's
                                                                            a/b and sqrt(a): out[5][n] = x_div, a/b, x_sqrt,
                                                                            sqrt, x_div_r(a, b, 1/b) */
/* The marching kernels' zone accessors (csrc/hydro_kernels.hip: scalar base + 32-bit byte offset + immediate) at byte offsets 0,
 * 2^31 - 8, 2^31 and 2^32 - 8 of a 4 GiB field: lane l stores 1000 + l there and 2000 + l at the same offset from the base moved up by
 * stride_bytes; stored[2][4] = the eight words as hipMemcpy finds them, loaded[3][4] = as the accessors load them back (base, base +
 * stride, and the base's word again from the zone below through the immediate). */
int aa_test_zone_offsets(unsigned stride_bytes, double *stored, double *loaded);
int aa_test_explog(int n, const double *x, double *y_exp, double *y_log);  /* the exp / ln of csrc/ion_pass.hip
                                                                             (n a multiple of 4): exp(x), ln|x|  */
/* The folds and step picks of the radiation sub-cycle on scratch memory (tests/test_gpu_ion_subcycles.py): rec[n][5] = n records
 * (dt_chem, dt_therm, max_dti, cellcount, neg) as the blocks of a pass leave them; prev[AA_TEST_PICK_SCALARS] = the scalars the
 * picks find (those a previous call returned; NULL: all 0).  Launches k_ion_reduce -> words[0][8]; k_ion_reduce_pick (no mailbox)
 * -> words[1][8], out[0][]; k_ion_pick2 on words[0] (one rank) -> out[1][]; k_ion_pick, its reductions set to words[0] and handed
 * dt_done = first ? 0 : prev's dt_done + dt_sel -> out[2][].  A row of out / prev: dt_sel, limit_hit, dt_done, dt_applied,
 * hit_applied, neg_applied, spec_state, dt_chem_out, dt_therm_out, neg_out, then the reductions as the pick leaves them: max_dti,
 * cellcount, dt_chem, dt_therm (the doubles whose bits the words hold), neg_dt_chem, 0. */
#define AA_TEST_PICK_SCALARS 16
int aa_test_ion_pick(int n, const double *rec, int first, double limit, int spec_armed, const double *prev, double *words, double *out);
/* The queued sub-cycle loop (aa_set_ion_batch) over a script, on scratch memory: rec[n][5] = the record of the first pass and of
 * the pass of every further sub-cycle.  The first pick, then visits of b0, K, K, ... queued picks with one publication each and no
 * passes in between, until the device stops the loop (an error if the script runs out first).  out[5] = niter, dt_done, stop code
 * (1 stopped, 2 stopped and cut, 3 negative dt_chem), visits, queued picks that left at once; steps[n]: the applied steps in order. */
int aa_test_ion_batch(int n, const double *rec, int fine, double limit, double cour_no, int K, int b0, double *out, double *steps);

/* ---- dump_history.c:157-200: volume integrals over the active zones of this Grid, in the column
 *      order of the .hst file: mass, total E, x1/x2/x3 Mom., x1/x2/x3-KE, scalar 0 (0 if NSCALARS=0).
 *      Sums over Grids (MPI_Reduce :257) and the division by the Domain volume (:271-279) are the
 *      caller's.                                                                               */
int aa_history(aa_grid *g, double sums[9]);

/* ---- dump_vtk.c:28-327 / dump_binary.c:30-266: the single-precision payload of a data dump, made on the device from the
 *      ACTIVE zones and delivered in file order, one section at a time (zones [k][j][i], i fastest, no ghost zones):
 *        AA_DUMP_VTK  0 density | 1 momentum or velocity, 3 floats per zone | 2 total energy or pressure | 3.. scalars;
 *                     every word big-endian as the reference writes it (ath_bswap)
 *        AA_DUMP_BIN  NVAR = 5 + NSCALARS sections in ConsS / PrimS order, native byte order
 *      prim != 0: primitive variables exactly as Cons1D_to_Prim1D (convert_var.c:389-421; the same bits from the default and
 *      the strict library).  The header text / binary header around the sections is the caller's (they hold no field data).
 *      host_dst is any host memory of aa_dump_section_floats() floats: the library stages through a page-locked bounce
 *      buffer of its own (two halves of AA_DUMP_CHUNK_FLOATS floats, default 2^23).  Like aa_download_cons the call uses the
 *      face-state area (allowed between aa_integrate_begin and aa_integrate_3d_ctu) and changes no state.                 */
#define AA_DUMP_VTK 1
#define AA_DUMP_BIN 2
int       aa_dump_sections(const aa_grid *g, int fmt);                        /* sections of a dump (0: unknown format) */
long long aa_dump_section_floats(const aa_grid *g, int fmt, int section);     /* n or 3n; 0 past the last section       */
int       aa_dump_section(aa_grid *g, int fmt, int prim, int section, float *host_dst);

/* ---- the same payload without stopping the run: ONE kernel makes every section of a dump from the state as it is when the call is
 *      queued (behind everything the step launched) into a snapshot buffer in device memory -- not the face-state area -- and one
 *      copy on the stream of the dumps brings it into page-locked host memory while the Grid's stream goes on with the next step.
 *      A Grid has AA_DUMP_SLOTS snapshot slots, each a device buffer and a page-locked buffer of aa_dump_snapshot_bytes() (made on
 *      the slot's first use, sized for either format, kept until aa_destroy): two snapshots may be in flight or in the hands of a
 *      writer at a time.
 *        begin    queues kernel and copy and returns without waiting (allocation on first use apart).  It leaves the face-state
 *                 area and the sweeps of aa_integrate_begin alone: a step between begin and ready is the step it would have been.
 *                 max_bytes: the caller's cap on the payload (a larger one is refused).
 *        ready    1: the payload is on the host, 0: in flight, < 0: error; never blocks.   wait: blocks until it is.
 *        section  section s of the payload in the page-locked buffer, *nfloats = aa_dump_section_floats() (sections start 16-byte
 *                 aligned, the words are those of aa_dump_section bit for bit); NULL before the payload is on the host.  The
 *                 pointer holds until release.
 *        release  waits if the copy is still in flight and frees the slot for the next begin.
 *      ONE threading rule: every one of these calls -- like the rest of this header -- comes from the thread that drives the run.
 *      Another thread may READ the memory `section` returned (and write it to a file) between ready and release, nothing else.
 *      Composite handles (aa_params.nslab > 1) refuse begin: aa_dump_section is the path there.  aa_destroy with a snapshot in
 *      flight waits for it.                                                                                                       */
#define AA_DUMP_SLOTS 2
long long    aa_dump_snapshot_bytes(const aa_grid *g, int fmt);                 /* of the payload with its padding (0: unknown format) */
int          aa_dump_snapshot_begin(aa_grid *g, int slot, int fmt, int prim, long long max_bytes);
int          aa_dump_snapshot_ready(aa_grid *g, int slot);
int          aa_dump_snapshot_wait(aa_grid *g, int slot);
const float *aa_dump_snapshot_section(aa_grid *g, int slot, int section, long long *nfloats);
int          aa_dump_snapshot_release(aa_grid *g, int slot);

/* ---- output.c:629-1233: the payload of a single-variable output (out = d | M1 | M2 | M3 | E | V1 | V2 | V3 | P | cs2 | flux with
 *      x1 / x2 / x3 slices) from the ACTIVE zones, in double precision: OutData3 where nothing is reduced, OutData2 / OutData1 where
 *      one or two directions are.  reduce[a] != 0 sums the expression over the zones lo[a] .. hi[a] (inclusive, counted from 0 over the
 *      active zones) of direction a in the reference's order and multiplies by 1.0/count[/count]; the caller finds the indices (the
 *      search of output.c:763-780 with the face positions of fc_pos; the reference then adds the first active index a second time,
 *      :789-790, so its zones lie nghost above the slice: a range may reach into the ghost zones, which must be current), the
 *      library refuses a range outside the Grid's arrays.  The same bits from the default and the strict library.
 *        aa_outdata       dims[3] doubles ([dims[2]][dims[1]][dims[0]], a reduced direction has 1) to host_dst, with the payload's
 *                         minimum and maximum as minmax1/2/3 (utils.c:142-197) leave them
 *        aa_outdata_dims  dims alone: what host_dst has to hold
 *        aa_outdata_gray  the bytes of output_pgm.c:94-122 for the same payload scaled with dmin / dmax (the caller's: the
 *                         payload's own or the block's fixed ones), dims[0]*dims[1]*dims[2] bytes in file order
 *      AA_OUT_FLUX is GridS.EdgeFlux[k][j][i] (prob/ioniz_sphere.c:356-359) of a Grid with a radiation plane.  Refused: a Grid cut
 *      into slabs, a level of an aa_mesh, a 1-D Grid.  Like aa_dump_section the calls stage through the face-state area and the
 *      bounce buffer and change no state.                                                                                          */
#define AA_OUT_D    0
#define AA_OUT_M1   1
#define AA_OUT_M2   2
#define AA_OUT_M3   3
#define AA_OUT_E    4
#define AA_OUT_V1   5
#define AA_OUT_V2   6
#define AA_OUT_V3   7
#define AA_OUT_P    8
#define AA_OUT_CS2  9
#define AA_OUT_FLUX 10
int aa_outdata_dims(aa_grid *g, int expr, const int reduce[3], const int lo[3], const int hi[3], int dims[3]);
int aa_outdata(aa_grid *g, int expr, const int reduce[3], const int lo[3], const int hi[3], double *host_dst, int dims[3],
               double *dmin, double *dmax);
int aa_outdata_gray(aa_grid *g, int expr, const int reduce[3], const int lo[3], const int hi[3], double dmin, double dmax,
                    unsigned char *host_dst, int dims[3]);

/* ---- restart.c:463-983 / restart_grids :52-456: the double-precision payload of a restart dump to and from the resident state,
 *      one labelled section at a time, ACTIVE zones [k][j][i] only:
 *        DENSITY | 1-MOMENTUM | 2-MOMENTUM | 3-MOMENTUM | ENERGY | EDGEFLUX (ion radiation; (Nx1+1)(Nx2+1)(Nx3+1)) | SCALAR n
 *      `host` is any host memory of aa_rst_section_doubles() doubles; the data travels through the bounce buffer of the data
 *      dumps (AA_DUMP_CHUNK_FLOATS: two floats per double).  get uses the face-state area like aa_dump_section and changes no
 *      state.  put writes the active zones and NO ghost zone; afterwards the device holds what no host block does (the next
 *      aa_download_ghost_zones moves the whole block) and new_dt's maxima are due again; EDGEFLUX counts as filled.  Composite
 *      handles (aa_params.nslab > 1) take both calls.
 *      aa_resume / aa_mesh_resume: the start sequence of a restarted run (main.c:398-451) -- aa_start / aa_mesh_start without
 *      new_dt: the dt of the file (aa_set_mesh_state / aa_mesh_set_state) is the next step's.                              */
int       aa_rst_sections(const aa_grid *g);
int       aa_rst_section_label(const aa_grid *g, int section, char *buf, int n);
long long aa_rst_section_doubles(const aa_grid *g, int section);          /* 0 past the last section */
int       aa_rst_section_get(aa_grid *g, int section, double *host);
int       aa_rst_section_put(aa_grid *g, int section, const double *host);
/*      Boxes: the part [lo, lo + n) of a section, `lo` and `n` in the section's own index space (active zones; the (Nx+1)^3 face
 *      indices for EDGEFLUX), `host` the box, contiguous [k][j][i].  Any sequence of put_box calls that tiles a section leaves
 *      what one aa_rst_section_put of the joined data leaves; put_box writes nothing outside its box; get_box returns the
 *      slice of aa_rst_section_get.  -1 for a box that is not wholly inside the section, and for composite handles
 *      (aa_params.nslab > 1): those take whole sections only.                                                             */
int       aa_rst_section_get_box(aa_grid *g, int section, const int lo[3], const int n[3], double *host);
int       aa_rst_section_put_box(aa_grid *g, int section, const int lo[3], const int n[3], const double *host);
int       aa_resume(aa_grid *g);
int       aa_mesh_resume(aa_mesh *m);

/* ---- the restart payload without stopping the run -- the route of aa_dump_snapshot_* above, in double precision: ONE kernel makes
 *      every section but EDGEFLUX from the state as it is when the call is queued (behind everything the step launched), one copy on
 *      the Grid's stream puts EDGEFLUX beside them (filled first where the one-kernel sub-cycle left that to the reader, as
 *      aa_rst_section_get does), both into a snapshot buffer in device memory -- not the face-state area --, and one copy on the
 *      stream of the dumps brings the whole payload into page-locked host memory while the Grid's stream goes on with the next step.
 *      A Grid has AA_RST_SLOTS = 1 slot: a device buffer and a page-locked buffer of aa_rst_snapshot_bytes(), made on first use and
 *      kept until aa_destroy (restart blocks fire rarely; at 512^3 with scalar and EdgeFlux the payload is 7.52 GB on either side).
 *        begin    queues kernel and copies and returns without waiting (allocation on first use apart).  It leaves the face-state
 *                 area, the sweeps of aa_integrate_begin, new_dt's maxima and the host block's bookkeeping alone: a step between
 *                 begin and ready is the step it would have been.  max_bytes: the caller's cap on the payload (a larger one is
 *                 refused before the slot is taken); a held slot is refused too.  Profile scopes: rst_snapshot (the kernel),
 *                 rst_snapshot_ef (the EDGEFLUX copy).
 *        ready    1: the payload is on the host, 0: in flight, < 0: error; never blocks.   wait: blocks until it is.
 *        section  section s (those of aa_rst_sections / aa_rst_section_label) in the page-locked buffer, *ndoubles =
 *                 aa_rst_section_doubles(); sections start 16-byte aligned, the doubles are those of aa_rst_section_get bit for
 *                 bit; NULL before the payload is on the host.  The pointer holds until release.
 *        release  waits if the copy is still in flight and frees the slot for the next begin.
 *      The threading rule is that of the dump snapshots: every call from the thread that drives the run; another thread may READ the
 *      memory `section` returned between ready and release, nothing else.  Composite handles (aa_params.nslab > 1) refuse begin:
 *      aa_rst_section_get is the path there.  aa_destroy with a snapshot in flight waits for it.                              */
#define AA_RST_SLOTS 1
long long     aa_rst_snapshot_bytes(const aa_grid *g);                /* payload with its padding */
int           aa_rst_snapshot_begin(aa_grid *g, int slot, long long max_bytes);
int           aa_rst_snapshot_ready(aa_grid *g, int slot);
int           aa_rst_snapshot_wait(aa_grid *g, int slot);
const double *aa_rst_snapshot_section(aa_grid *g, int slot, int section, long long *ndoubles);  /* NULL before the payload is on the host */
int           aa_rst_snapshot_release(aa_grid *g, int slot);

/* ---- measurement: per-kernel accumulated device time (hipEvent pairs on the stream) */
int         aa_profile_enable(aa_grid *g, int on);
int         aa_profile_reset(aa_grid *g);
int         aa_profile_count(const aa_grid *g);
const char *aa_profile_name(const aa_grid *g, int i);
int         aa_profile_get(aa_grid *g, int i, double *total_ms, long long *launches);

#ifdef __cplusplus
}
#endif
#endif
