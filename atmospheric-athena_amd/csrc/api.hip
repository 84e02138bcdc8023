// api.hip -- the C-ABI of include/athena_amd.h: owns the device mirror of one Grid, sequences
// the kernel chains in the order of the reference's main loop (main.c:519-669) and of
// ion_radtransfer_3d (ionrad_3d.c:862-1047), and carries the scalar control flow (dt, sub-cycle
// termination) on the host exactly as the reference does.  No CPU arithmetic path exists here.
#include <hip/hip_runtime.h>
#include <math.h>
#include <float.h>
#include <limits.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "field_offsets.h"
#include <string>
#include <thread>
#include <vector>
#include "api_internal.h"

using namespace aa;

static thread_local char g_err[1024] = "";
int aa_fail(int code, const char *fmt, ...)
{
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
  return code;
}
#define fail aa_fail

static void prof_drain(aa_grid *g)
{
  hipStreamSynchronize(g->st);
  for (auto &e : g->pe) {
    for (size_t i = 0; i + 1 < e.ev.size(); i += 2) {
      float ms = 0; hipEventElapsedTime(&ms, e.ev[i], e.ev[i + 1]); e.total_ms += ms;
      g->ev_pool.push_back(e.ev[i]); g->ev_pool.push_back(e.ev[i + 1]);
    }
    e.ev.clear();
  }
}

void aa_eval_grav_tables(const aa_params &p, const double dx[3], int N1, int N2, int N3, aa_gravpot_fn fn, std::vector<double> t[4])
{
  for (int w = 0; w < 4; w++) t[w].resize((size_t)N1*N2*N3);
  // the callback is a pure function of position (as in the reference, which calls it ~52 times
  // per cell per step): evaluate k-planes on all host cores
  unsigned nth = std::thread::hardware_concurrency(); if (nth < 1) nth = 1; if (nth > 64) nth = 64;
  if ((int)nth > N3) nth = N3;
  std::vector<std::thread> pool;
  for (unsigned w = 0; w < nth; w++) pool.emplace_back([&, w]() {
    for (int k = (int)w; k < N3; k += (int)nth) for (int j = 0; j < N2; j++) for (int i = 0; i < N1; i++) {
      // cc_pos.c:36-43
      const double x1 = p.MinX[0] + ((double)(i - AA_NGHOST) + 0.5)*dx[0];
      const double x2 = p.MinX[1] + ((double)(j - AA_NGHOST) + 0.5)*dx[1];
      const double x3 = p.MinX[2] + ((double)(k - AA_NGHOST) + 0.5)*dx[2];
      const size_t m = ((size_t)k*N2 + j)*N1 + i;
      t[0][m] = fn(x1, x2, x3);
      t[1][m] = fn(x1 - 0.5*dx[0], x2, x3);
      t[2][m] = fn(x1, x2 - 0.5*dx[1], x3);
      t[3][m] = fn(x1, x2, x3 - 0.5*dx[2]);
    }
  });
  for (auto &th : pool) th.join();
}

// Every launch choice of one Grid (grid.h LaunchCfg): read from the environment here, once per Grid, never again.  One line per
// knob: its name, its default or the size from which the default is on, its range.  Returns fail()'s code for a value out of range.
static int launch_cfg_read(const aa_params &p, LaunchCfg &c)
{
  auto env = [](const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; };
  constexpr int UNSET = INT_MIN;                                                     // (no knob takes it as a value)
  auto on = [](int v, bool dflt) { return v == UNSET ? dflt : v != 0; };             // an on / off knob: forced by any number, else by default
  const long long zones = (long long)p.Nx[0]*p.Nx[1]*p.Nx[2], rays = (long long)p.Nx[1]*p.Nx[2];
  // ---- launch geometry
  c.strip = env("AA_STRIP", 64); c.xcd = env("AA_XCD", 1);
  c.x1_flat = env("AA_X1_FLAT", 1); c.slopes_march = env("AA_SLOPES_MARCH", 1);
  c.ca_kc = env("AA_CA_KC", 0); c.fu_kc = env("AA_FU_KC", 0);
  c.ion_pass_cap = env("AA_ION_PASS_BLOCKS", 4096); if (c.ion_pass_cap < 1) c.ion_pass_cap = 1;
  c.pitch_align = env("AA_PITCH_ALIGN", 1);
  c.mailbox = env("AA_MAILBOX", 1); c.mailbox_spin_us = env("AA_MAILBOX_SPIN_US", 300);
  c.bc_one = env("AA_BC_ONE", 1); c.fuse_pick = env("AA_ION_FUSE_PICK", 1); c.pin_one = env("AA_PIN_ONE", 1);
  c.edge_overlap = env("AA_EDGE_OVERLAP", 0);
  c.sw_chunk = env("AA_SW_CHUNK", 0); c.vp_kc = env("AA_VP_KC", 0);
  if (c.sw_chunk < 0 || c.sw_chunk > 4096 || c.vp_kc < 0 || c.vp_kc > 4096)
    return fail(-1, "[aa_create]: AA_SW_CHUNK=%d AA_VP_KC=%d: each must be 0 (by size) or 1..4096", c.sw_chunk, c.vp_kc);
  // ---- which kernels carry a stage
  // the one-kernel correct pass (with both first passes on board since round 4) wins from about 70^3 zones on, the tile kernels
  // below (profiles/microbench/ca_threshold_r04.sh: 64^3 -11 %, 80^3 +20 %, 96^3 +21 %, 112^3 +21 %; until round 4 the
  // limit was 2^21 zones): same results bit for bit, so the choice follows the size unless AA_CORRECT_ALL forces it
  c.correct_all = on(env("AA_CORRECT_ALL", UNSET), zones >= 400000LL);
  { const int v = env("AA_X3_FUSED", UNSET); c.x3_fused_mode = v == UNSET ? -1 : (v != 0); }      // (the potential arrives after aa_create: x3_fused below decides)
  c.fused_update = on(env("AA_FUSED_UPDATE", UNSET), true);
  c.cfl_step = on(env("AA_CFL_FUSED", UNSET), true);                 // aa_step: new_dt's maxima from the update kernel (=2: as 1, kept for the tests)
  c.vl_predict = on(env("AA_VL_PREDICT", UNSET), zones >= (1LL << 18));
  // rates inside the ray sweep: one block per 64 rays, so it needs many rays to fill the chip (512^2 rays:
  // -2.9 ms per step; 80^2 rays: +6 %); same results either way
  c.fused_rates = on(env("AA_FUSED_RATES", UNSET), rays >= (1LL << 17));
  // the one-kernel sub-cycle wants whole wavefronts along the rays (rays of 48 zones or more: the 52^3 level of the reference's own deck
  // takes 6 sub-cycles of 4 launches + a read-back the other way, 3 + a read-back this way -- there the launches count, not the 12 idle
  // lanes of a wavefront; round 3: 64); AA_ION_FUSED forces either path
  c.ion_fused = on(env("AA_ION_FUSED", UNSET), p.Nx[0] >= 48);
  c.ion_begin_fused = on(env("AA_ION_BEGIN_FUSED", UNSET), true);
  c.ion_spec_on = on(env("AA_ION_SPECULATE", UNSET), true);
  // the speculating first pass without the entry's dense saves (k_ion_pass<LEAN>): auto = behind a step whose speculation stood
  // after one sub-cycle (the stationary regime); same results bit for bit either way
  { const char *e = getenv("AA_ION_LEAN");
    c.ion_lean = (!e || !strcmp(e, "auto")) ? -1 : (!strcmp(e, "0") ? 0 : (!strcmp(e, "1") ? 1 : 2));
    if (c.ion_lean == 2) return fail(-1, "[aa_create]: AA_ION_LEAN=%s: must be auto, 0 or 1", e); }
  // radiation sub-cycles queued per host visit (ion_run_fused): 1 = one read-back per sub-cycle, the launches as they were; same bits
  c.ion_batch = env("AA_ION_BATCH", 1);
  if (c.ion_batch < 1 || c.ion_batch > AA_ION_BATCH_MAX)
    return fail(-1, "[aa_create]: AA_ION_BATCH=%d: must be 1 (a read-back per sub-cycle) or 2..%d", c.ion_batch, AA_ION_BATCH_MAX);
  // ---- not a launch choice of a kernel of the step, kept here all the same: floats per half of the dumps' bounce buffer
  c.dump_chunk = env("AA_DUMP_CHUNK_FLOATS", 1 << 23); if (c.dump_chunk < 4) c.dump_chunk = 4; if (c.dump_chunk > (1 << 28)) c.dump_chunk = 1 << 28;
  return 0;
}
// slabs asked for: aa_params.nslab, or AA_NGPU in the environment (drop-in executables)
static int slabs_wanted(const aa_params *p)
{ int ns = p->nslab; if (ns == 0) { const char *e = getenv("AA_NGPU"); if (e) ns = atoi(e); } return ns; }

extern "C" {

const char *aa_last_error(void) { return g_err; }

int aa_create(const aa_params *p, aa_grid **out)
{
  if (!p || !out) return fail(-1, "[aa_create]: null argument");
  // integrate.c:30-84: the integrator follows the number of directions with more than one zone
  int dim = 0;
  for (int d = 0; d < 3; d++) {
    if (p->Nx[d] < 1) return fail(-1, "[aa_create]: Nx%d=%d", d + 1, p->Nx[d]);
    if (p->Nx[d] > 1) dim++;
  }
  if (dim == 2 && p->Nx[2] > 1)
    return fail(-1, "[integrate_init]: 2D problem must have Nx1 and Nx2 > 1: Nx1=%d, Nx2=%d, Nx3=%d", p->Nx[0], p->Nx[1], p->Nx[2]);
  if (dim == 1 && p->Nx[0] <= 1)
    return fail(-1, "[integrate_init]: 1D problem must have Nx1 > 1: Nx1=%d, Nx2=%d, Nx3=%d", p->Nx[0], p->Nx[1], p->Nx[2]);
  // (integrate.c:30-88 has no text for dim = 0: no case of its switch, and neither message behind it, takes it)
  if (dim == 0) return fail(-1, "[aa_create]: a Grid of a single zone (Nx1=%d, Nx2=%d, Nx3=%d): no integrator takes it; a 1-D Grid has Nx1 > 1", p->Nx[0], p->Nx[1], p->Nx[2]);
  const bool two_d = dim == 2, one_d = dim == 1;
  if (one_d) {
    // integrate.c:30 counts the ROOT Domain's directions: a row of a 2-D or 3-D Domain would take that Domain's integrator, and
    // the library does not cut Domains along x2 (nor 2-D ones at all)
    if (p->rootNx[1] != 1 || p->rootNx[2] != 1)
      return fail(-1, "[aa_create]: Nx2 = Nx3 = 1 in a root Domain of %d x %d x %d zones: a 1-D Grid takes a 1-D root Domain",
                  p->rootNx[0], p->rootNx[1], p->rootNx[2]);
    // bvals_mhd.c fills the ghost zones of a side one after the other, and one side after the other; with fewer active zones
    // than ghost zones a boundary function reads ghost zones, and the order decides what it finds.  k_bc and k1d_run fill the
    // eight ghost zones at once, which is the same thing only where every source is an active zone
    if (p->Nx[0] < AA_NGHOST)
      return fail(-1, "[aa_create]: a 1-D Grid of %d zones: fewer than the %d ghost zones of a side is not supported", p->Nx[0], AA_NGHOST);
    if (p->integrator == 1 && p->cour_no > 0.5)   // integrate.c:41-44; integrate_1d_ctu has no such limit (:38-39)
      return fail(-1, "<time>cour_no=%e, must be <= 0.5 with 1D VL integrator", p->cour_no);
    // what no reference target pins on a 1-D Grid is refused
    if (p->ion) return fail(-1, "[aa_create]: ion radiation on a 1-D Grid: the reference has ionrad_3d only");
    if (p->nscal != 0) return fail(-1, "[aa_create]: passive scalars on a 1-D Grid: no reference target pins them (NSCALARS must be 0)");
    if (p->level != 0) return fail(-1, "[aa_create]: a refined level (level %d) as a 1-D Grid: static mesh refinement is not available in 1-D", p->level);
    const int ns = slabs_wanted(p);
    if (ns > 1) return fail(-1, "[aa_create]: a 1-D Grid cannot be cut into x3 slabs (nslab / AA_NGPU = %d)", ns);
  }
  if (!two_d && !one_d && p->cour_no > 0.5)   // integrate.c:66-68
    return fail(-1, "<time>cour_no was set to %g: must be <= 0.5 with 3D integrator", p->cour_no);
  if (two_d) {
    if (p->integrator == 1 && p->cour_no > 0.5)   // integrate.c:55-57; integrate_2d_ctu has no such limit
      return fail(-1, "<time>cour_no=%e, must be <= 0.5 with 2D VL integrator", p->cour_no);
    // what no reference target pins on a 2-D Grid is refused
    if (p->ion) return fail(-1, "[aa_create]: ion radiation on a 2-D Grid: the reference has ionrad_3d only");
    if (p->nscal != 0) return fail(-1, "[aa_create]: passive scalars on a 2-D Grid: no reference target pins them (NSCALARS must be 0)");
    if (p->order == 3) return fail(-1, "[aa_create]: third-order reconstruction on a 2-D Grid: no reference target pins it");
    const int ns = slabs_wanted(p);
    if (ns > 1) return fail(-1, "[aa_create]: a 2-D Grid cannot be cut into x3 slabs (nslab / AA_NGPU = %d)", ns);
  }
  if (p->ion && p->nscal != 1) return fail(-1, "[aa_create]: ion radiation needs NSCALARS=1");
  if (p->nscal != 0 && p->nscal != 1) return fail(-1, "[aa_create]: NSCALARS must be 0 or 1");
  { // one Grid of the caller on several GPUs
    const int ns = slabs_wanted(p);
    if (ns > 1) return slabs_create(p, ns, out);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(-3, "[aa_create]: no HIP device visible -- this library has no CPU path");
  HIPCHK(hipSetDevice(p->device));
  aa_grid *g = new aa_grid();
  g->p = *p;
  HostGrid &d = g->d;
  d = HostGrid();
  if (int rc = launch_cfg_read(*p, d.cfg)) { delete g; return rc; }
  d.Nx1 = p->Nx[0]; d.Nx2 = p->Nx[1]; d.Nx3 = p->Nx[2];
  d.N1 = d.Nx1 + 2*AA_NGHOST; d.N2 = d.Nx2 + 2*AA_NGHOST; d.N3 = d.Nx3 + 2*AA_NGHOST;
  d.is = d.js = d.ks = AA_NGHOST;
  d.ie = d.is + d.Nx1 - 1; d.je = d.js + d.Nx2 - 1; d.ke = d.ks + d.Nx3 - 1;
  g->two_d = two_d; g->one_d = one_d;
  if (two_d || one_d) { d.N3 = 1; d.ks = d.ke = 0; }      // init_grid.c:144-174: no ghost zones along a direction with one zone
  if (two_d) {
    // AA_2D_BATCH: steps aa_run_2d queues between two reads of the device clock (1 .. 1024); 0: it loops over aa_step; same bits
    const char *e = getenv("AA_2D_BATCH");
    g->batch_2d = e ? atoi(e) : AA_2D_BATCH_DEFAULT;
    if (g->batch_2d < 0 || g->batch_2d > 1024) { const int v = g->batch_2d; delete g; return fail(-1, "[aa_create]: AA_2D_BATCH=%d: must be 0 (step by step) or 1..1024", v); }
  }
  if (!two_d && !one_d) {
    // AA_3D_BATCH: steps aa_run_3d queues between two reads of the device clock (1 .. 1024); 0: it loops over aa_step; same bits
    const char *e = getenv("AA_3D_BATCH");
    g->batch_3d = e ? atoi(e) : AA_3D_BATCH_DEFAULT;
    if (g->batch_3d < 0 || g->batch_3d > 1024) { const int v = g->batch_3d; delete g; return fail(-1, "[aa_create]: AA_3D_BATCH=%d: must be 0 (step by step) or 1..1024", v); }
  }
  if (one_d) {
    d.N2 = 1; d.js = d.je = 0;
    // AA_1D_RESIDENT=0: aa_run_1d steps one launch at a time (k1d_step) instead of many steps in one launch (k1d_run); same bits
    const char *e = getenv("AA_1D_RESIDENT");
    g->resident_1d = e ? atoi(e) != 0 : true;
  }
  // rows padded to a multiple of 16 doubles and every field shifted by 12 doubles: the first active zone of
  // every row (i = 4) then sits on a 128-byte line, and so does every wavefront of the kernels that walk the
  // active zones 64 at a time (-2.9 % of a 512^3 step; AA_PITCH_ALIGN=0: dense rows)
  const int pitch_align = d.cfg.pitch_align;
  d.sJ = pitch_align ? ((d.N1 + 15)/16)*16 : d.N1; d.sK = (long)d.sJ*d.N2; d.nc = d.sK*d.N3;
  // the marching 3-D kernels reach a zone by a 32-bit byte offset from its field's base (field_offsets.h): one code path, no fallback
  if (!one_d && !two_d && !field_offsets_fit(d.nc, d.sJ, d.sK)) {
    const long nc = d.nc; delete g;
    return fail(-1, "[aa_create]: a Grid of %ld zones (ghost zones and row padding included): a field of more than 2^32 bytes is beyond the kernels' 32-bit zone offsets", nc);
  }
  if (p->level < 0 || p->level > 7) { delete g; return fail(-1, "[aa_create]: level %d out of range", p->level); }
  g->level = p->level;
  Real rootdx[3];
  for (int a = 0; a < 3; a++) {
    rootdx[a] = (p->xmax[a] - p->xmin[a])/(Real)(p->rootNx[a]);   // init_mesh.c:225
    d.dx[a] = rootdx[a]/(Real)(1 << p->level);                    // :245
    if ((two_d && a == 2) || (one_d && a >= 1)) d.dx[a] = rootdx[a];                     // :331-337: a direction with one zone keeps the root's extent
  }
  d.Gamma = p->gamma; d.Gamma_1 = p->gamma - 1.0; d.rGamma_1 = 1.0/d.Gamma_1;
  // one pool: U 6 | LR 36 | F 18 | eta 3 | dhalf 1 | phi 4 | ion 5 + sign(1) | edgeflux
  const size_t nc = (size_t)d.nc;
  const size_t nef = (size_t)(d.Nx1 + 1)*(d.Nx2 + 1)*(d.Nx3 + 1);
  size_t n = nc*(6 + 36 + 18 + 5 + 1 + 4);       // eta: 3 + the two edge arrays of k_correct_all
  // a 2-D Grid: U 5 | LR 2 x 2 x 5 | F 2 x 5 | eta 2 | edge (hydro2d_kernels.hip), nothing of the 3-D set
  const size_t nedge2 = two_d ? (size_t)5*ntiles_2d(d)*d.N2 : 0;
  if (two_d) n = nc*(5 + 20 + 10 + 2) + nedge2;
  // a 1-D Grid: U 5 | the second U buffer 5 (hydro1d_kernels.hip; k1d_step writes it, then the two change places), nothing else
  if (one_d) n = nc*(5 + 5);
  g->ion_fused = p->ion && (p->ion_path ? p->ion_path == 1 : d.cfg.ion_fused);      // (the caller's choice goes before the knob and the size)
  const size_t nrays = (size_t)d.Nx2*d.Nx3;
  if (p->ion) n += nc*6 + nef;
  const size_t nlean = nrays*(size_t)((d.Nx1 + 63)/64);      // one ballot word per ray and 64-zone tile (k_ion_pass<LEAN>)
  if (g->ion_fused) n += 2*nc + 2*nrays + nlean;
  if (p->order != 0 && p->order != 2 && p->order != 3) { delete g; return fail(-1, "[aa_create]: order %d (2: PLM, 3: PPM)", p->order); }
  if (p->order == 3 && !one_d) n += nc*18;      // (the 1-D kernels keep the slopes in LDS)
  g->pool_doubles = n;
  n += 16;
  hipError_t e = hipMalloc(&g->pool, n*sizeof(Real));
  if (e != hipSuccess) { delete g; return fail(-2, "[aa_create]: hipMalloc of %.2f GB failed: %s", n*8e-9, hipGetErrorString(e)); }
  g->bytes = (long long)(n*sizeof(Real));
  hipMemset(g->pool, 0, n*sizeof(Real));
  Real *q = g->pool + (pitch_align ? 12 : 0);
  if (one_d) { d.U = q; q += 5*nc; d.LR = q; q += 5*nc; }
  else if (two_d) { d.U = q; q += 5*nc; d.LR = q; q += 20*nc; d.F = q; q += 10*nc; d.eta = q; q += 2*nc; g->edge2d = q; q += nedge2; }
  else {
  d.U = q; q += 6*nc; d.LR = q; q += 36*nc; d.F = q; q += 18*nc; d.eta = q; q += 5*nc; d.dhalf = q; q += nc;
  d.phi = q; q += 4*nc;
  }
  if (p->order == 3 && !one_d) { d.slope = q; q += 18*nc; }
  if (p->ion) {
    d.ph_rate = q; q += nc; d.kin = q; q += nc; d.vmax = q; q += nc;
    d.e_init = q; q += nc; d.x_init = q; q += nc;
    d.sign = (int2*)q; q += nc; d.edgeflux = q; q += nef;
    d.sg16 = (unsigned short*)d.sign;                  // the fused path keeps its 2-byte sign words in the same storage
    d.fin[0] = d.ph_rate; d.fin[1] = d.ph_rate;
    if (g->ion_fused) { d.fin[1] = q; q += nc; d.s_init = q; q += nc; d.raylast = q; q += 2*nrays; d.lean_mask = (unsigned long long*)q; q += nlean; }
    IonPar &ip = g->ion;
    ip.sigma_ph = p->sigma_ph; ip.m_H = p->m_H; ip.mu = p->mu; ip.e_gamma = p->e_gamma; ip.alpha_C = p->alpha_C;
    ip.k_B = p->k_B; ip.time_unit = p->time_unit;
    ip.max_de_iter = p->max_de_iter; ip.max_de_therm_iter = p->max_de_therm_iter; ip.max_dx_iter = p->max_dx_iter;
    ip.max_de_step = p->max_de_step; ip.max_de_therm_step = p->max_de_therm_step; ip.max_dx_step = p->max_dx_step;
    ip.tfloor = p->tfloor; ip.tceil = p->tceil; ip.cour_no = p->cour_no;
    // ionrad.c:112-131: smallest face area and the "low" neutral density, from the ROOT dx
    // (the reference's fallback at :129 is dx[1], reproduced as is)
    Real a1 = rootdx[0]*rootdx[1], a2 = rootdx[0]*rootdx[2], a3 = rootdx[1]*rootdx[2];
    if (a1 < a2) ip.min_area = (a1 < a3) ? a1 : a3; else ip.min_area = (a2 < a3) ? a2 : a3;
    Real maxdx = rootdx[0] > rootdx[1] ? rootdx[0] : rootdx[1];
    maxdx = maxdx > rootdx[2] ? maxdx : rootdx[1];
    ip.d_nlo = 1.0e-4 * p->m_H / (p->sigma_ph * maxdx);      // MINOPTDEPTH, ionrad.h:29
    ip.inv_mH = 1.0/p->m_H; ip.inv_kB = 1.0/p->k_B; ip.aC14 = p->alpha_C/(14.0*p->m_H);
    ip.rec_floor = 2.59e-13*pow(p->tfloor/1.0e4, -0.7);      // recomb_rate_coef(tfloor), ionrad_chemistry.c:111
    ip.cx1 = p->max_dx_iter/(1 + p->max_dx_iter);
    ip.ce1 = p->max_de_therm_iter/(1 + p->max_de_therm_iter); ip.ce2 = p->max_de_iter/(1 + p->max_de_iter);
    ip.ie1 = 1.0/(1.0 + p->max_de_therm_iter); ip.ie2 = 1.0/(1.0 + p->max_de_iter);
    for (int a = 0; a < 3; a++) ip.inv_dx[a] = 1.0/d.dx[a];
    ip.iso = (d.dx[0] == d.dx[1] && d.dx[1] == d.dx[2]);
  }
  if (hipMalloc(&g->sc, sizeof(DevScalars)) != hipSuccess ||
      hipHostMalloc(&g->mb, sizeof(Mailbox), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
    hipFree(g->pool); delete g; return fail(-2, "[aa_create]: scalar buffers");
  }
  memset(g->mb, 0, sizeof(Mailbox));
  g->sc_host = &g->mb->s;
  if (hipHostGetDevicePointer((void**)&g->mb_dev, g->mb, 0) != hipSuccess) { (void)hipGetLastError(); g->mb_dev = nullptr; d.cfg.mailbox = 0; }
  if (g->ion_fused) {
    // (records of a pass | a second set nobody folds: k_ion_pass<LEAN>'s way back)
    if (hipMalloc(&g->ion_part, (size_t)2*ion_pass_blocks(d)*sizeof(IonPart)) != hipSuccess ||
        hipMalloc(&g->ion_words, AA_ION_WORDS*sizeof(Real)) != hipSuccess) {
      hipFree(g->pool); hipFree(g->sc); hipHostFree(g->mb); delete g; return fail(-2, "[aa_create]: ion reduction buffers");
    }
  }
  // (every word of these is written before it is read; zeroed all the same, so that no run ever depends on what a freed
  //  allocation of an earlier Grid left behind)
  (void)hipMemset(g->sc, 0, sizeof(DevScalars));
  if (g->ion_part) (void)hipMemset(g->ion_part, 0, (size_t)2*ion_pass_blocks(d)*sizeof(IonPart));
  if (g->ion_words) (void)hipMemset(g->ion_words, 0, AA_ION_WORDS*sizeof(Real));
  hipStreamCreate(&g->st); g->own_stream = true;
  *out = g;
  return 0;
}

void aa_destroy(aa_grid *g)
{
  if (!g) return;
  if (g->link) { slabs_destroy(g); return; }          // a composite handle, whether or not it has slabs yet
  hipStreamSynchronize(g->st);
  prof_drain(g);
  dump_release(g);
  outdata_release(g);
  hipFree(g->pool); hipFree(g->sc); hipHostFree(g->mb);
  for (hipEvent_t ev : g->ev_pool) hipEventDestroy(ev);
  if (g->ion_part) hipFree(g->ion_part);
  if (g->ion_words) hipFree(g->ion_words);
  if (g->pin_idx) hipFree(g->pin_idx);
  if (g->pin_val) hipFree(g->pin_val);
  if (g->pin_mask) hipFree(g->pin_mask);
  if (g->cfl_part) hipFree(g->cfl_part);
  if (g->fofc_list) hipFree(g->fofc_list);
  if (g->clock) { hipHostFree(g->clock); hipFree(g->run2d_dev); hipFree(g->run3d_dev); }      // (run.hip run_buffers; run2d_dev / run3d_dev: null on Grids of the other shapes)
  hst_free_grid(g); hst_free_sched(g->hst);      // (run.hip: the buffers of an armed history schedule, if one was ever armed)
  if (g->d.phalf) hipFree(g->d.phalf);
  if (g->side) hipStreamDestroy(g->side);
  if (g->ev_fork) hipEventDestroy(g->ev_fork);
  if (g->ev_join) hipEventDestroy(g->ev_join);
  if (g->own_stream) hipStreamDestroy(g->st);
  delete g;
}

int aa_set_stream(aa_grid *g, void *s)
{
  if (!g->slab.empty()) return fail(-1, "[aa_set_stream]: a Grid cut into slabs runs on its slabs' own streams");
  hipStreamSynchronize(g->st);
  if (g->own_stream) { hipStreamDestroy(g->st); g->own_stream = false; }
  g->st = (hipStream_t)s;
  return 0;
}
int aa_sync(aa_grid *g) { if (!g->slab.empty()) return slabs_sync(g); HIPCHK(hipStreamSynchronize(g->st)); return 0; }
long long aa_device_bytes(const aa_grid *g) { return g->slab.empty() ? g->bytes : slabs_device_bytes(g); }

// ---- state transfer: staging through the (idle) face-state area ---------------------------
int aa_upload_cons(aa_grid *g, const double *U)
{
  g->cfl_ready = false; g->active_dirty = false;      // (host and device agree on the active zones from here on)
  g->inner_swept = false;          // the state changes under a pending aa_integrate_begin: its sweeps are redone
  ion_lean_forget(g);
  if (!g->slab.empty()) return slabs_upload_cons(g, U);
  const int nvar = 5 + g->p.nscal; const size_t n = (size_t)g->d.N1*g->d.N2*g->d.N3*nvar;
  HIPCHK(hipMemcpyAsync(g->d.LR, U, n*sizeof(Real), hipMemcpyHostToDevice, g->st));
  launch_aos_to_soa(g->d, nvar, g->d.LR, g->st);
  HIPCHK(hipStreamSynchronize(g->st));
  return 0;
}
int aa_download_cons(aa_grid *g, double *U)
{
  if (!g->slab.empty()) return slabs_download_cons(g, U);
  g->inner_swept = false;          // the face-state area is the staging buffer (see aa_integrate_begin in athena_amd.h)
  const int nvar = 5 + g->p.nscal; const size_t n = (size_t)g->d.N1*g->d.N2*g->d.N3*nvar;
  launch_soa_to_aos(g->d, nvar, g->d.LR, g->st);
  HIPCHK(hipMemcpyAsync(U, g->d.LR, n*sizeof(Real), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  g->active_dirty = false;
  return 0;
}
// Only the GHOST zones of the host block [N3][N2][N1][nvar] (the caller knows its active zones are current: nothing but
// boundary calls ran on the device since the block last travelled).  The shell is 9 % of a 256^3 block: six strided copies
// out of the staging area instead of the whole block over PCIe.
int aa_download_ghost_zones(aa_grid *g, double *U)
{
  if (!g->slab.empty()) return slabs_download_cons(g, U);
  // the caller says its active zones are current; the library knows whether any call since the last full transfer wrote active zones
  // (the integrators, the ion step, pinned zones, restriction / flux correction): then the whole block travels
  if (g->active_dirty || g->one_d) return aa_download_cons(g, U);      // (a 1-D block is one row: it travels whole)
  g->inner_swept = false;
  const int nvar = 5 + g->p.nscal, N1 = g->d.N1, N2 = g->d.N2, N3 = g->d.N3, ng = AA_NGHOST;
  const size_t row = (size_t)N1*nvar*sizeof(Real), plane = row*N2;
  launch_soa_to_aos(g->d, nvar, g->d.LR, g->st);
  const char *S = (const char*)g->d.LR; char *D = (char*)U;
  if (g->two_d) {      // one plane: four rows at either end, four zones at either end of the rows in between
    const size_t w2 = (size_t)ng*nvar*sizeof(Real), mid2 = (size_t)ng*row;
    HIPCHK(hipMemcpyAsync(D, S, ng*row, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipMemcpyAsync(D + (size_t)(N2 - ng)*row, S + (size_t)(N2 - ng)*row, ng*row, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipMemcpy2DAsync(D + mid2, row, S + mid2, row, w2, (size_t)(N2 - 2*ng), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipMemcpy2DAsync(D + mid2 + row - w2, row, S + mid2 + row - w2, row, w2, (size_t)(N2 - 2*ng), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    return 0;
  }
  // x3: the four planes at either end, whole
  HIPCHK(hipMemcpyAsync(D, S, ng*plane, hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpyAsync(D + (size_t)(N3 - ng)*plane, S + (size_t)(N3 - ng)*plane, ng*plane, hipMemcpyDeviceToHost, g->st));
  const size_t mid = (size_t)ng*plane;      // the planes in between
  // x2: four rows at either end of every such plane
  HIPCHK(hipMemcpy2DAsync(D + mid, plane, S + mid, plane, ng*row, N3 - 2*ng, hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpy2DAsync(D + mid + (size_t)(N2 - ng)*row, plane, S + mid + (size_t)(N2 - ng)*row, plane, ng*row, N3 - 2*ng, hipMemcpyDeviceToHost, g->st));
  // x1: four zones at either end of every row of those planes (the rows are one constant stride apart across j and k)
  const size_t w = (size_t)ng*nvar*sizeof(Real), nrows = (size_t)(N3 - 2*ng)*N2;
  HIPCHK(hipMemcpy2DAsync(D + mid, row, S + mid, row, w, nrows, hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpy2DAsync(D + mid + row - w, row, S + mid + row - w, row, w, nrows, hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  return 0;
}
// planes [k_first, k_first + nplanes) of the host block [N3][N2][N1][nvar]
int aa_download_cons_planes(aa_grid *g, int k_first, int nplanes, double *dst)
{
  if (!g->slab.empty()) return fail(-1, "[aa_download_cons_planes]: one slab at a time");
  if (k_first < 0 || nplanes < 0 || k_first + nplanes > g->d.N3) return fail(-1, "[aa_download_cons_planes]: planes %d..%d", k_first, k_first + nplanes);
  g->inner_swept = false;
  const int nvar = 5 + g->p.nscal; const size_t pl = (size_t)g->d.N1*g->d.N2*nvar;
  launch_soa_to_aos(g->d, nvar, g->d.LR, g->st);
  HIPCHK(hipMemcpyAsync(dst, g->d.LR + (size_t)k_first*pl, (size_t)nplanes*pl*sizeof(Real), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  return 0;
}
int aa_download_edgeflux_planes(aa_grid *g, int nplanes, double *dst)
{
  if (!g->slab.empty()) return fail(-1, "[aa_download_edgeflux_planes]: one slab at a time");
  if (!g->p.ion) return fail(-1, "[aa_download_edgeflux]: ion radiation is off");
  if (nplanes < 0 || nplanes > g->d.Nx3 + 1) return fail(-1, "[aa_download_edgeflux_planes]: %d planes of %d", nplanes, g->d.Nx3 + 1);
  { int rc = aa_edgeflux_ready(g); if (rc) return rc; }
  const size_t n = (size_t)(g->d.Nx1 + 1)*(g->d.Nx2 + 1)*(size_t)nplanes;
  HIPCHK(hipMemcpyAsync(dst, g->d.edgeflux, n*sizeof(Real), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  return 0;
}
int aa_upload_edgeflux(aa_grid *g, const double *ef)
{
  if (!g->slab.empty()) return slabs_upload_edgeflux(g, ef);
  if (!g->p.ion) return fail(-1, "[aa_upload_edgeflux]: ion radiation is off");
  g->ef_stale = false;
  const size_t n = (size_t)(g->d.Nx1 + 1)*(g->d.Nx2 + 1)*(g->d.Nx3 + 1);
  HIPCHK(hipMemcpyAsync(g->d.edgeflux, ef, n*sizeof(Real), hipMemcpyHostToDevice, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  return 0;
}
int aa_download_edgeflux(aa_grid *g, double *ef)
{
  if (!g->slab.empty()) return slabs_download_edgeflux(g, ef);
  if (!g->p.ion) return fail(-1, "[aa_download_edgeflux]: ion radiation is off");
  { int rc = aa_edgeflux_ready(g); if (rc) return rc; }
  const size_t n = (size_t)(g->d.Nx1 + 1)*(g->d.Nx2 + 1)*(g->d.Nx3 + 1);
  HIPCHK(hipMemcpyAsync(ef, g->d.edgeflux, n*sizeof(Real), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  return 0;
}
int aa_get_mesh_state(const aa_grid *g, double *time, double *dt, int *nstep)
{ if (time) *time = g->time; if (dt) *dt = g->dt; if (nstep) *nstep = g->nstep; return 0; }
int aa_set_mesh_state(aa_grid *g, double time, double dt, int nstep)
{ g->time = time; g->dt = dt; g->nstep = nstep; if (!g->slab.empty()) slabs_push_state(g); return 0; }

// ---- hooks --------------------------------------------------------------------------------
int aa_set_static_grav_tables(aa_grid *g, const double *pc, const double *p1, const double *p2, const double *p3)
{
  if (!g->slab.empty()) return slabs_set_grav_tables(g, pc, p1, p2, p3);
  if (!pc) { g->grav = false; return 0; }
  if (g->one_d) return fail(-1, "[aa_set_static_grav_tables]: static gravity on a 1-D Grid: no reference run pins it");
  if (g->two_d) return fail(-1, "[aa_set_static_grav_tables]: static gravity on a 2-D Grid: no reference run pins it (prob/ioniz_sphere.c:113 writes past a 2-D Grid)");
  // host tables are dense [N3][N2][N1]; device rows are sJ apart
  const double *src[4] = {pc, p1, p2, p3};
  for (int w = 0; w < 4; w++)
    HIPCHK(hipMemcpy2DAsync(g->d.phi + (size_t)w*g->d.nc, (size_t)g->d.sJ*sizeof(Real), src[w], (size_t)g->d.N1*sizeof(Real),
                            (size_t)g->d.N1*sizeof(Real), (size_t)g->d.N2*g->d.N3, hipMemcpyHostToDevice, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  g->grav = true;
  return 0;
}

int aa_set_static_grav_pot(aa_grid *g, aa_gravpot_fn fn)
{
  if (!fn) return aa_set_static_grav_tables(g, nullptr, nullptr, nullptr, nullptr);
  if (g->one_d) return fail(-1, "[aa_set_static_grav_pot]: static gravity on a 1-D Grid: no reference run pins it");
  if (g->two_d) return fail(-1, "[aa_set_static_grav_pot]: static gravity on a 2-D Grid: no reference run pins it (prob/ioniz_sphere.c:113 writes past a 2-D Grid)");
  // (a Grid cut into slabs evaluates the callback at the positions of the caller's ONE Grid: the slabs then hold
  //  the very numbers the undivided Grid would)
  const int N1 = g->p.Nx[0] + 2*AA_NGHOST, N2 = g->p.Nx[1] + 2*AA_NGHOST, N3 = g->p.Nx[2] + 2*AA_NGHOST;
  double dx[3];
  for (int a = 0; a < 3; a++) dx[a] = ((g->p.xmax[a] - g->p.xmin[a])/(Real)(g->p.rootNx[a]))/(Real)(1 << g->p.level);
  std::vector<double> t[4];
  aa_eval_grav_tables(g->p, dx, N1, N2, N3, fn, t);
  return aa_set_static_grav_tables(g, t[0].data(), t[1].data(), t[2].data(), t[3].data());
}

// globals.h:25 CoolingFunc.  The reference calls the enrolled function per state on the host; on the device the function has to
// be one the library carries: AA_COOL_KOYINUT = KoyInut (microphysics/cool.c:48), the one the reference ships.  The CTU
// integrator then runs the second compilation of its kernels (namespace aa_cool: hydro_kernels.hip with -DAA_COOLING=1) and
// keeps P^{n+1/2} beside d^{n+1/2}.  The van Leer integrator of the reference has no cooling terms (integrate_3d_vl.c).
int aa_set_cooling(aa_grid *g, int kind)
{
  if (kind != AA_COOL_NONE && kind != AA_COOL_KOYINUT) return fail(-1, "[aa_set_cooling]: kind=%d: only AA_COOL_NONE and AA_COOL_KOYINUT", kind);
  if (kind && g->p.integrator == 1) return fail(-1, "[aa_set_cooling]: the van Leer integrator has no cooling terms in the reference (integrate_3d_vl.c)");
  if (kind && g->one_d) return fail(-1, "[aa_set_cooling]: cooling on a 1-D Grid: no reference target pins it");
  if (kind && g->two_d) return fail(-1, "[aa_set_cooling]: cooling on a 2-D Grid: no reference target pins it");
  if (!g->slab.empty() || g->link) return slabs_set_cooling(g, kind);
  g->inner_swept = false;
  if (kind && !g->d.phalf) {
    HIPCHK(hipMalloc(&g->d.phalf, (size_t)g->d.nc*sizeof(Real)));
    HIPCHK(hipMemsetAsync(g->d.phalf, 0, (size_t)g->d.nc*sizeof(Real), g->st));
    g->bytes += (long long)g->d.nc*sizeof(Real);
  }
  g->cool = kind;
  return 0;
}

// First-order flux correction of the van Leer integrator (the reference's --enable-fofc: integrate_3d_vl.c Step 10, a second-order
// flux that came out NaN becomes the predictor flux of its face; Step 14 + FixCell, a zone the full update left with d < 0 or P < 0
// takes the predictor fluxes instead, and so do its neighbours for the faces they share).  Off by default; with it off the step
// launches what it always did.  Accepted where a reference build pins the behaviour, refused elsewhere.
int aa_set_fofc(aa_grid *g, int on)
{
  if (!on) { if (g->slab.empty() && !g->link) { g->fofc = false; g->fofc_counts[0] = g->fofc_counts[1] = g->fofc_counts[2] = 0; } return 0; }
  if (!g->slab.empty() || g->link) return fail(-1, "[aa_set_fofc]: not available on a Grid cut into slabs (FixCell's bounds are per Grid; no reference build pins a cut one)");
  if (g->one_d) return fail(-1, "[aa_set_fofc]: first-order flux correction on a 1-D Grid: no reference target pins it (integrate_3d_vl.c only here)");
  if (g->two_d) return fail(-1, "[aa_set_fofc]: first-order flux correction on a 2-D Grid: no reference target pins it (integrate_3d_vl.c only here)");
  if (g->p.integrator != 1) return fail(-1, "[aa_set_fofc]: the CTU integrator has no first-order flux correction in the reference (integrate_3d_vl.c only)");
  if (g->p.order == 3) return fail(-1, "[aa_set_fofc]: no reference build pins first-order flux correction with third-order reconstruction");
  if (g->level > 0 || g->keep_flux) return fail(-1, "[aa_set_fofc]: not available on a level of a refined Mesh (FixCell would also have to replace the fluxes RestrictCorrect reads)");
  if (!g->fofc_list) {
    HIPCHK(hipMalloc(&g->fofc_list, (size_t)3*AA_FOFC_MAX*sizeof(long long)));
    HIPCHK(hipMemsetAsync(g->fofc_list, 0, (size_t)3*AA_FOFC_MAX*sizeof(long long), g->st));
    g->bytes += (long long)(3*AA_FOFC_MAX*sizeof(long long));
  }
  g->fofc = true;
  return 0;
}
int aa_get_fofc(const aa_grid *g) { return g->fofc ? 1 : 0; }
int aa_get_fofc_counts(const aa_grid *g, long long out[3])
{
  for (int n = 0; n < 3; n++) out[n] = g->fofc_counts[n];
  return 0;
}

int aa_set_pinned_cells(aa_grid *g, long long n, const long long *index, const double *values)
{
  if (!g->slab.empty()) return slabs_set_pinned_cells(g, n, index, values);
  if (g->pin_idx) { hipFree(g->pin_idx); g->pin_idx = nullptr; }
  if (g->pin_val) { hipFree(g->pin_val); g->pin_val = nullptr; }
  if (g->pin_mask) { hipFree(g->pin_mask); g->pin_mask = nullptr; }
  g->npin = 0;
  g->cfl_ready = false; g->active_dirty = true;
  if (n <= 0) return 0;
  const int nvar = 5 + g->p.nscal;
  HIPCHK(hipMalloc(&g->pin_idx, (size_t)n*sizeof(long long)));
  HIPCHK(hipMalloc(&g->pin_val, (size_t)n*nvar*sizeof(Real)));
  HIPCHK(hipMemcpy(g->pin_idx, index, (size_t)n*sizeof(long long), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g->pin_val, values, (size_t)n*nvar*sizeof(Real), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&g->pin_mask, (size_t)g->d.nc));
  HIPCHK(hipMemsetAsync(g->pin_mask, 0, (size_t)g->d.nc, g->st));
  launch_pin_mask(g->d, n, g->pin_idx, g->pin_mask, g->st);
  g->npin = n;
  return 0;
}
int aa_apply_pinned_cells(aa_grid *g)
{
  if (!g->slab.empty()) return slabs_apply_pinned_cells(g);
  Scope s(g, "pinned_cells");
  // (cfl_ready: the zones were left out of the integrator's maxima and join them here, from the values written -- one launch;
  //  AA_PIN_ONE=0: k_pinned + k_pinned_cfl, which reads them back)
  if (g->cfl_ready && g->d.cfg.pin_one) launch_pinned(g->d, 5 + g->p.nscal, g->npin, g->pin_idx, g->pin_val, g->st, g->sc);
  else {
    launch_pinned(g->d, 5 + g->p.nscal, g->npin, g->pin_idx, g->pin_val, g->st);
    if (g->cfl_ready) launch_pinned_cfl(g->d, g->npin, g->pin_idx, g->sc, g->st);
  }
  if (g->npin > 0) g->active_dirty = true;      // active zones written: aa_download_ghost_zones must move the whole block
  return 0;
}

int aa_add_radplane_3d(aa_grid *g, int dir, double flux)
{
  if (g->one_d) return fail(-1, "[add_radplane_3d]: ion radiation on a 1-D Grid: the reference has ionrad_3d only");
  if (g->two_d) return fail(-1, "[add_radplane_3d]: ion radiation on a 2-D Grid: the reference has ionrad_3d only");
  if (!g->p.ion) return fail(-1, "[add_radplane_3d]: ion radiation is off");
  // Rays along +x1 (dir = -1) and along +x2 (dir = -2).  The reference has no working behaviour for the others:
  // right-to-left rays (dir > 0) never enter the loop `for (i=s; i<=e; i+=lr)` with s > e (ionradplane_3d.c:275, :335,
  // :367), and dir = -3 divides by a cell_len that is only assigned in the right-to-left branch (:136-145).
  if (dir != -1 && dir != -2)
    return fail(-1, "[add_radplane_3d]: dir=%d: only -1 (rays along +x1) and -2 (along +x2) have defined behaviour in the reference", dir);
  if (dir == -2) {
    if (g->p.level > 0) return fail(-1, "[add_radplane_3d]: rays along +x2 on a refined level are not supported");
    g->ion_fused = false;          // the two-kernel sub-cycle carries this sweep
  }
  if (!g->slab.empty()) { int rc = slabs_add_radplane(g, dir, flux); if (rc) return rc; }
  g->rad_dir = dir; g->flux_i = flux; g->nradplane = 1;
  return 0;
}

int aa_has_radplane(const aa_grid *g) { return (g->p.ion && g->nradplane > 0) ? 1 : 0; }   // main.c:546: the ion step runs iff nradplane > 0

// ---- per-step call sites ------------------------------------------------------------------
int aa_bvals_mhd(aa_grid *g)
{
  if (!g->slab.empty()) return slabs_bvals_mhd(g);
  Scope s(g, "bvals_mhd");
  if (g->one_d) {      // bvals_mhd.c:187-193, :542: the x1 pass only
    launch_bc_dir(g->d, 0, 0, g->p.bc[0], g->p.bc[1], g->st);
    return 0;
  }
  if (g->two_d) {      // bvals_mhd.c:170: x1 then x2, so the corners fill; a direction with one zone has no boundary functions
    for (int d = 0; d < 2; d++) launch_bc_dir(g->d, g->p.nscal, d, g->p.bc[2*d], g->p.bc[2*d + 1], g->st);
    return 0;
  }
  if (g->d.cfg.bc_one) { launch_bc_shell(g->d, g->p.nscal, g->p.bc, g->st); return 0; }      // the three passes as one launch: same bits
  for (int d = 0; d < 3; d++)            // x1, x2, x3 so the corners fill (bvals_mhd.c:170)
    launch_bc_dir(g->d, g->p.nscal, d, g->p.bc[2*d], g->p.bc[2*d + 1], g->st);
  return 0;
}

int aa_bvals_mhd_side(aa_grid *g, int dir, int side)
{
  if (dir < 0 || dir > 2 || side < 0 || side > 1) return fail(-1, "[aa_bvals_mhd_side]: dir=%d side=%d", dir, side);
  if (!g->slab.empty()) return slabs_bvals_mhd_side(g, dir, side);
  if ((g->two_d && dir == 2) || (g->one_d && dir >= 1)) return 0;      // (no ghost zones along a direction with one zone)
  const int flag = g->p.bc[2*dir + side];
  if (flag) { Scope s(g, "bvals_mhd"); launch_bc(g->d, g->p.nscal, dir, side, flag, g->st); }
  return 0;
}

int aa_bvals_ionrad(aa_grid *g)
{
  if (!g->slab.empty()) return slabs_bvals_ionrad(g);
  if (!g->p.ion) return 0;
  if (g->rad_dir == -1) launch_edgeflux_bc(g->d, g->flux_i, g->st);
  else if (g->rad_dir == -2) launch_edgeflux_bc_x2(g->d, g->flux_i, g->st);
  return 0;
}

// DevScalars device -> host.  The mailbox way (grid.h Mailbox; AA_MAILBOX=0: a copy + a stream wait): a one-wave kernel behind the
// producers writes the scalars into pinned host memory and stamps them; the host polls the stamp -- for a while: a wait that
// outlasts AA_MAILBOX_SPIN_US (a long kernel in front) ends in hipStreamSynchronize like the other way, so no core spins for
// milliseconds.  On the small Grids of the reference's own decks a step is a few dozen launches and 2 + N_sub read-backs, and a
// copy + wait costs ~25 us against ~8 for a launch + poll.
int aa_fetch_scalars(aa_grid *g)
{
  if (!g->slab.empty()) return fail(-1, "[aa_fetch_scalars]: not available on a Grid cut into slabs");
  g->host_syncs++;
  if (g->d.cfg.mailbox && g->mb_dev) {
    unsigned long long seq;
    if (g->mb_prepublished && g->mb_prepublished == g->mb_seq) { seq = g->mb_seq; g->mb_prepublished = 0; }      // (k_ion_reduce_pick has published them)
    else { seq = ++g->mb_seq; launch_publish(g->sc, g->mb_dev, seq, g->st); }
    volatile unsigned long long *stamp = &g->mb->seq;
    struct timespec t0; clock_gettime(CLOCK_MONOTONIC, &t0);
    for (unsigned spins = 1;; spins++) {
      if (__atomic_load_n(stamp, __ATOMIC_ACQUIRE) == seq) return 0;
      if ((spins & 127u) == 0) {
        struct timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);
        if ((t1.tv_sec - t0.tv_sec)*1000000L + (t1.tv_nsec - t0.tv_nsec)/1000L > g->d.cfg.mailbox_spin_us) break;
      }
      __builtin_ia32_pause();
    }
    HIPCHK(hipStreamSynchronize(g->st));          // (also where a kernel in front failed: the error comes out here)
    if (__atomic_load_n(stamp, __ATOMIC_ACQUIRE) != seq) return fail(-2, "[aa_fetch_scalars]: the mailbox kernel finished without its stamp");
    return 0;
  }
  HIPCHK(hipMemcpyAsync(g->sc_host, g->sc, sizeof(DevScalars), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  return 0;
}
#define fetch_scalars aa_fetch_scalars

int aa_new_dt_local(aa_grid *g, double *dt_cfl)
{
  if (!g->slab.empty()) return slabs_new_dt_local(g, dt_cfl);
  if (g->cfl_ready) g->cfl_ready = false;        // the integrator (+ aa_apply_pinned_cells) has left the maxima in g->sc
  else { Scope s(g, "new_dt");
    HIPCHK(hipMemsetAsync(g->sc->max_v, 0, 3*sizeof(unsigned long long), g->st));
    launch_cfl(g->d, g->sc, g->st); }
  int rc = fetch_scalars(g); if (rc) return rc;
  const int ndir = g->one_d ? 1 : g->two_d ? 2 : 3;     // new_dt.c:156-161: only the directions with more than one zone
  double v[3]; max_v_of(*g->sc_host, v);
  *dt_cfl = dt_courant(g->p.cour_no, dt_fold(0.0, v, g->d.dx, ndir));
  return 0;
}

int aa_cfl_max_v(aa_grid *g, double *v)      // new_dt.c:72-140 of this Grid: max(|v_d| + a) per direction
{
  if (!g->slab.empty()) return slabs_cfl_max_v(g, v);
  if (g->cfl_ready) g->cfl_ready = false;        // the integrator (+ aa_apply_pinned_cells) has left the maxima in g->sc
  else { Scope s(g, "new_dt");
    HIPCHK(hipMemsetAsync(g->sc->max_v, 0, 3*sizeof(unsigned long long), g->st));
    launch_cfl(g->d, g->sc, g->st); }
  int rc = fetch_scalars(g); if (rc) return rc;
  max_v_of(*g->sc_host, v);
  if (g->two_d || g->one_d) v[2] = 0.0;  // new_dt.c:135: max_v3 only where Nx3 > 1
  if (g->one_d) v[1] = 0.0;              // :128: max_v2 only where Nx2 > 1
  return 0;
}

int aa_new_dt(aa_grid *g)
{
  double dtc; int rc = aa_new_dt_local(g, &dtc); if (rc) return rc;
  g->dt = dt_pick(g->nstep, g->dt, dtc, g->time, g->p.tlim);       // new_dt.c:167-185
  if (!g->slab.empty()) slabs_push_state(g);
  return 0;
}

// k_correct_all also does the x3 first pass (no k_sweep_march<2> launch, those fluxes never in HBM): -3.1 ms of a 512^3
// blast step, -4.2 ms ifront, -4.4 / -2.0 ms third order without / with gravity.  Second order + passive scalar + gravity
// (ioniz_sphere: 249 VGPRs at 2 waves per SIMD) was a draw in round 2 and left to the sweep kernel; with the hardware
// min / max in the reconstruction (default build, hydro_dev.h: 12 % fewer instructions in this kernel) it is ahead there too --
// 19.5 against 17.2 + 4.55 ms, hydro chain 45.5 -> 43.3 (round 3, same-box ABAB) -- and is the default everywhere.
// Same bits either way.
// aa_cfl_in_update: zero the maxima and let k_flux2_update fill them
static void cfl_arm(aa_grid *g)
{
  g->cfl_ready = g->cfl_in_update && (g->npin == 0 || g->pin_mask);
  if (g->cfl_ready) (void)hipMemsetAsync(g->sc->max_v, 0, 3*sizeof(unsigned long long), g->st);
}
int aa_cfl_in_update(aa_grid *g, int on)
{
  if (!g->slab.empty()) return 0;      // (composite Grids keep k_cfl)
  // (until round 4 the strict build kept k_cfl: with -ffp-contract=off its 6-variable update kernel spilled 15 registers with the
  //  CFL epilogue; with the lower x3 flux parked in LDS and dt/dx in scalar registers it holds 250 without scratch, and the strict
  //  step is 48.1 -> 47.1 ms at 512^3 with the maxima from the update kernel.  AA_CFL_FUSED=0: k_cfl; =2: as 1, kept for the tests)
  g->cfl_in_update = on != 0; g->cfl_ready = false;
  return 0;
}

static bool x3_fused(const aa_grid *g)      // default: always (round 3; until then not for second order + scalar + gravity)
{ return g->d.cfg.x3_fused_mode >= 0 ? g->d.cfg.x3_fused_mode != 0 : true; }

// The part of the step that needs none of the x3 neighbours' planes: the first-pass x1 and x2 sweeps of the k-planes
// ks .. ke (a pencil along x1 or x2 lies in one plane).  A multi-GPU caller posts the x3 halo, calls this, waits for the
// halo, unpacks it and calls aa_integrate_3d_ctu, which then sweeps only the four ghost planes in x1 / x2: the messages
// travel under ~10 ms of kernels at 512^3.  Same bits as without the call.  Does nothing (returns 0) where the split
// does not apply: composite Grids, third order (the slope arrays come first), the unfused correct / update chains, VL.
// the kernels of a run with a cooling function are the second compilation of hydro_kernels.hip (namespace aa_cool)
#define HL(f) (g->cool ? aa_cool::f : aa::f)
// ... and with it the x1 first pass (round 4: k_correct_all<X3F>): no k_sweep_x1_flat launch before k_correct_all
static bool x1_fused(const aa_grid *g) { return g->d.cfg.correct_all && x3_fused(g); }
int aa_integrate_begin(aa_grid *g)
{
  if (g->two_d || g->one_d) return 0;
  if (!g->slab.empty() || g->p.integrator != 0 || g->d.slope || !g->d.cfg.correct_all || !g->d.cfg.fused_update || g->inner_swept) return 0;
  const HostGrid &d = g->d; const int ns = g->p.nscal; const Real dt = g->dt;
  const int nk = d.ke - d.ks + 1;
  { Scope s(g, "sweep_x2"); HL(launch_sweep)(d, ns, 1, dt, g->grav, g->st, 2, nk); }
  if (!x1_fused(g)) { Scope s(g, "sweep_x1"); HL(launch_sweep)(d, ns, 0, dt, g->grav, g->st, 2, nk); }
  g->inner_swept = true;
  g->inner_dt = dt;
  HIPCHK(hipGetLastError());
  return 0;
}

// aa_params.integrator 2: the CTU integrator of a reference built WITHOUT --enable-h-correction (its configure default).  Such a
// build has no eta arrays and roe.c uses |ev| where the H_CORRECTION build uses MAX(|ev|, etah) (roe.c:282-290): the numbers of
// etah = 0.  The correct kernels have just filled the etas; zero them before the second-pass fluxes read them (three fields:
// ~1 ms at 512^3 in this mode only; the kernels of the default mode carry no flag for it).
static void no_h_correction(aa_grid *g)
{
  if (g->p.integrator != 2) return;
  Scope s(g, "no_h_correction");
  (void)hipMemsetAsync(g->d.eta, 0, (size_t)3*g->d.nc*sizeof(Real), g->st);
}

int aa_integrate_3d_ctu(aa_grid *g)
{
  if (!g->slab.empty()) return slabs_integrate(g, 0);
  if (g->one_d) return fail(-1, "[aa_integrate_3d_ctu]: this is a 1-D Grid (Nx2 = Nx3 = 1): aa_integrate_1d_ctu");
  if (g->two_d) return fail(-1, "[aa_integrate_3d_ctu]: this is a 2-D Grid (Nx3 = 1): aa_integrate_2d_ctu");
  g->cfl_ready = false; g->active_dirty = true;
  const HostGrid &d = g->d; const int ns = g->p.nscal; const Real dt = g->dt;
  if (g->inner_swept) {      // aa_integrate_begin did the planes ks .. ke: the two ghost planes either side remain
    if (g->inner_dt != dt) return fail(-1, "[aa_integrate_3d_ctu]: dt changed after aa_integrate_begin");
    g->inner_swept = false;
    const int nk = d.ke - d.ks + 1;
    { Scope s(g, "sweep_x2"); HL(launch_sweep)(d, ns, 1, dt, g->grav, g->st, 0, 2); HL(launch_sweep)(d, ns, 1, dt, g->grav, g->st, 2 + nk, 2); }
    if (!x1_fused(g)) { Scope s(g, "sweep_x1"); HL(launch_sweep)(d, ns, 0, dt, g->grav, g->st, 0, 2); HL(launch_sweep)(d, ns, 0, dt, g->grav, g->st, 2 + nk, 2); }
    if (!x3_fused(g)) { Scope s(g, "sweep_x3"); HL(launch_sweep)(d, ns, 2, dt, g->grav, g->st, 0, -1); }
    { Scope s(g, "correct_all"); HL(launch_correct_all)(d, ns, dt, g->grav, x3_fused(g), g->st, false); }
    no_h_correction(g);
    Scope s(g, "flux2_update");
    cfl_arm(g);
    HL(launch_flux2_update)(d, ns, dt, g->grav, g->keep_flux ? &g->keep : nullptr, g->st, g->cfl_ready ? g->sc : nullptr, g->pin_mask);
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (d.slope) { Scope s(g, "ppm_slopes"); for (int dir = 0; dir < 3; dir++) HL(launch_slopes)(d, ns, dir, g->st, nullptr); }
  // AA_EDGE_OVERLAP=1: the tile-edge x1 fluxes k_correct_all needs (k_x1_edge_flux: a few bytes per zone, bound by its strided loads)
  // beside the x2 sweep (bound by its arithmetic) on a stream of their own; both read U only.  -0.27 ms of a 41.4 ms step at 512^3
  // (profiles/r04_x1f_ab.txt item 11) -- off by default: it is inside the box-to-box spread, and with two kernels in flight at once the
  // per-kernel durations a profiler reports are no longer each kernel's own
  bool edges_aside = false;
  if (x1_fused(g) && d.cfg.edge_overlap) {
    if (!g->side) {
      HIPCHK(hipStreamCreateWithFlags(&g->side, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&g->ev_fork, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&g->ev_join, hipEventDisableTiming));
    }
    HIPCHK(hipEventRecord(g->ev_fork, g->st));
    HIPCHK(hipStreamWaitEvent(g->side, g->ev_fork, 0));
    HL(launch_x1_edges)(d, ns, dt, g->grav, g->side);
    HIPCHK(hipEventRecord(g->ev_join, g->side));
    edges_aside = true;
  }
  // x2 and x3 first, so that the x1 sweep can do its first pass and its correct pass in one go
  { Scope s(g, "sweep_x2"); HL(launch_sweep)(d, ns, 1, dt, g->grav, g->st, 0, -1); }
  if (edges_aside) HIPCHK(hipStreamWaitEvent(g->st, g->ev_join, 0));
  if (!(g->d.cfg.correct_all && x3_fused(g))) { Scope s(g, "sweep_x3"); HL(launch_sweep)(d, ns, 2, dt, g->grav, g->st, 0, -1); }
  if (g->d.cfg.correct_all) {
    if (!x1_fused(g)) { Scope s(g, "sweep_x1"); HL(launch_sweep)(d, ns, 0, dt, g->grav, g->st, 0, -1); }
    { Scope s(g, "correct_all"); HL(launch_correct_all)(d, ns, dt, g->grav, x3_fused(g), g->st, edges_aside); }
  } else {
    { Scope s(g, "sweep_correct_x1"); HL(launch_sweep_correct_x1)(d, ns, dt, g->grav, g->st); }
    { Scope s(g, "correct_x2"); HL(launch_correct)(d, ns, 1, dt, g->grav, g->st); }
    { Scope s(g, "correct_x3"); HL(launch_correct)(d, ns, 2, dt, g->grav, g->st); }
  }
  no_h_correction(g);
  if (g->d.cfg.fused_update) {
    Scope s(g, "flux2_update");
    cfl_arm(g);
    HL(launch_flux2_update)(d, ns, dt, g->grav, g->keep_flux ? &g->keep : nullptr, g->st, g->cfl_ready ? g->sc : nullptr, g->pin_mask);
  } else {
    { Scope s(g, "flux2_x1"); HL(launch_flux2)(d, ns, 0, g->st); }
    { Scope s(g, "flux2_x2"); HL(launch_flux2)(d, ns, 1, g->st); }
    { Scope s(g, "flux2_x3"); HL(launch_flux2)(d, ns, 2, g->st); }
    { Scope s(g, "update");   HL(launch_update)(d, ns, d.dhalf, dt, g->grav, g->st, nullptr, nullptr, nullptr); }
  }
  HIPCHK(hipGetLastError());
  return 0;
}

#undef HL
// U^n of the first-order flux correction: the second face-state family, idle in the van Leer integrator (grid.h)
static Real *fofc_un(const aa_grid *g) { return g->d.LR + 6*g->d.nc; }
static int fofc_zero(aa_grid *g, int first_field_off, int nfields)
{
  HIPCHK(hipMemsetAsync((char*)g->sc + first_field_off, 0, (size_t)nfields*sizeof(int), g->st));
  return 0;
}
static void vl_update(aa_grid *g)
{
  const HostGrid &d = g->d; const int ns = g->p.nscal;
  if (g->fofc) launch_update_fofc(d, ns, d.LR, g->dt, g->grav, g->st, g->cfl_ready ? g->sc : nullptr, g->cfl_part, g->pin_mask, g->sc, g->fofc_list);
  else launch_update(d, ns, d.LR, g->dt, g->grav, g->st, g->cfl_ready ? g->sc : nullptr, g->cfl_part, g->pin_mask);   // d^{n+1/2} = Uhalf.d
}
// What is left of Steps 10 and 14 once the update has run: the counts come back with the step's other scalars (one read-back;
// zero candidates, the common case, launches nothing more).
static int fofc_finish(aa_grid *g)
{
  const HostGrid &d = g->d; const int ns = g->p.nscal;
  const size_t ubytes = (size_t)(5 + ns)*d.nc*sizeof(Real);
  int rc = aa_fetch_scalars(g); if (rc) return rc;
  long long nan = 0;
  if (g->sc_host->fofc_nanseen) {
    // Step 10, made up for: the reference tests every second-order flux as it is computed; here the update notices a NaN among
    // the fluxes it reads (no pass over the flux arrays in the steps that have none: all of them, on every deck tried), and then
    // U^n goes back, the fluxes are repaired over the reference's ranges and the update runs again.
    HIPCHK(hipMemcpyAsync(d.U, fofc_un(g), ubytes, hipMemcpyDeviceToDevice, g->st));
    for (int dir = 0; dir < 3; dir++) launch_fofc_nanfix(d, ns, dir, fofc_un(g), g->sc, g->st);
    if ((rc = fofc_zero(g, offsetof(DevScalars, fofc_n), 2))) return rc;
    if (g->cfl_ready) HIPCHK(hipMemsetAsync(g->sc->max_v, 0, 3*sizeof(unsigned long long), g->st));
    vl_update(g);
    if ((rc = aa_fetch_scalars(g))) return rc;
    nan = g->sc_host->fofc_nan;
  }
  const int ncand = g->sc_host->fofc_n;
  long long negd = 0, negP = 0;
  if (ncand > AA_FOFC_MAX)
    return fail(-4, "[aa_integrate_3d_vl]: first-order flux correction: %d zones with d < 0 in one step, more than the %d the fix handles", ncand, AA_FOFC_MAX);
  if (ncand > 0) {
    launch_fofc_fix(d, ns, fofc_un(g), g->dt, g->sc, g->fofc_list, g->st);
    if ((rc = aa_fetch_scalars(g))) return rc;
    if (g->sc_host->fofc_ovf)
      return fail(-4, "[aa_integrate_3d_vl]: first-order flux correction: the zones changed ahead of the scan outgrew the list of %d", AA_FOFC_MAX);
    negd = g->sc_host->fofc_negd; negP = g->sc_host->fofc_negP;
    if (negd + negP > 0) g->cfl_ready = false;       // zones changed behind the update: its CFL maxima are stale, new_dt takes them with k_cfl
  }
  g->fofc_counts[0] = negd; g->fofc_counts[1] = negP; g->fofc_counts[2] = nan;
  return 0;
}

int aa_integrate_3d_vl(aa_grid *g)
{
  if (!g->slab.empty()) return slabs_integrate(g, 1);
  if (g->one_d) return fail(-1, "[aa_integrate_3d_vl]: this is a 1-D Grid (Nx2 = Nx3 = 1): aa_integrate_1d_vl");
  if (g->two_d) return fail(-1, "[aa_integrate_3d_vl]: this is a 2-D Grid (Nx3 = 1): aa_integrate_2d_vl");
  g->cfl_ready = false; g->active_dirty = true;
  // integrate_3d_vl.c:96-: donor-cell fluxes -> U^{n+1/2} -> PLM or PPM (no tracing) + Roe -> update
  const HostGrid &d = g->d; const int ns = g->p.nscal; const Real dt = g->dt;
  if (g->fofc) {      // Step 5d, restated: keep U^n (ghost zones included) instead of the predictor fluxes
    // (outside the profiler's stages, like the fix: their cost is the difference profiles/fofc_rate.py measures on whole steps)
    HIPCHK(hipMemcpyAsync(fofc_un(g), d.U, (size_t)(5 + ns)*d.nc*sizeof(Real), hipMemcpyDeviceToDevice, g->st));
    int rc = fofc_zero(g, offsetof(DevScalars, fofc_n), 6); if (rc) return rc;
  }
  // donor-cell fluxes + U^{n+1/2} in one marching kernel from 2^18 zones (512^3: 16.8 -> 9.7 ms; same at 80^3;
  // 10 % slower at 32^3); AA_VL_PREDICT forces either, the results are the same bit for bit
  if (g->d.cfg.vl_predict) { Scope s(g, "vl_predict"); launch_vl_predict(d, ns, dt, g->grav, g->st); }
  else {
    { Scope s(g, "vl_flux1"); for (int dir = 0; dir < 3; dir++) launch_vl_flux1(d, ns, dir, g->st); }
    { Scope s(g, "vl_uhalf"); launch_vl_uhalf(d, ns, dt, g->grav, g->st); }
  }
  // --with-order=3: the corrector reconstructs U^{n+1/2} with parabolae (no tracing, lr_states_ppm.c:502-507): their slopes first
  if (d.slope) { Scope s(g, "ppm_slopes"); for (int dir = 0; dir < 3; dir++) launch_slopes(d, ns, dir, g->st, d.LR); }
  { Scope s(g, "vl_flux2_x1"); launch_vl_flux2(d, ns, 0, dt, g->st); }
  { Scope s(g, "vl_flux2_x2"); launch_vl_flux2(d, ns, 1, dt, g->st); }
  { Scope s(g, "vl_flux2_x3"); launch_vl_flux2(d, ns, 2, dt, g->st); }
  {
    Scope s(g, "update");
    cfl_arm(g);                      // aa_cfl_in_update: new_dt's maxima ride on the update, as in k_flux2_update
    if (g->cfl_ready) {
      const long nb = update_blocks(d);
      if (g->cfl_part_n < 3*nb) {
        if (g->cfl_part) { (void)hipFree(g->cfl_part); g->cfl_part = nullptr; g->cfl_part_n = 0; }
        if (hipMalloc(&g->cfl_part, (size_t)3*nb*sizeof(Real)) == hipSuccess) g->cfl_part_n = 3*nb; else g->cfl_ready = false; g->active_dirty = true;
      }
    }
    vl_update(g);
  }
  HIPCHK(hipGetLastError());
  if (g->fofc) return fofc_finish(g);
  return 0;
}

int aa_ion_begin(aa_grid *g)
{
  g->cfl_ready = false; g->active_dirty = true;
  if (!g->p.ion) return fail(-1, "[ion_radtransfer]: ion radiation is off");
  if (!g->slab.empty()) return slabs_ion_begin(g);
  if (g->ion_fused) {
    // (a sweep of the previous ion step that nobody asked for is dropped here: its buffers are about to be reused)
    g->ion_cur = 0; g->ion_pending = false; g->ef_stale = false;
    g->ion_spec_dt = -1.0; g->ion_spec_armed = false;
    g->ion_step_spec = g->ion_step_lean = false; g->ion_step_updates = 0;
    if (g->d.cfg.ion_begin_fused) { g->ion_begin_due = true; return 0; }       // rides on the first pass
    Scope s(g, "ion_begin");
    launch_ion_begin16(g->d, g->ion, g->st);
    return 0;
  }
  Scope s(g, "ion_begin");
  launch_ion_begin(g->d, g->ion, g->st);
  return 0;
}

// ionradplane_3d.c:265: the hard-coded time ramp of the incident flux, evaluated once on the host (it is the same for
// every ray of the root level)
static Real ion_flux0(const aa_grid *g) { return g->flux_i*(5.*(erf((g->time - 1.2e5)/8e4)+1)+0.1); }

// ionrad_3d.c:922-938 of the two-kernel sub-cycle, queued: ph_rate_init, the ray sweep, the rates and their reductions
static int ion_sweep_and_rates(aa_grid *g)
{
  if (g->nradplane > 0) {
    const Real flux0 = ion_flux0(g);
    // :264-271: a refined level starts every ray from the flux its parent left in EdgeFlux[..][..][0]
    if (g->rad_dir == -2) { Scope s(g, "ray_sweep"); launch_ray_sweep_x2(g->d, g->ion, g->flux_i, g->st); }
    else if (g->d.cfg.fused_rates) { Scope s(g, "ray_sweep_rates"); launch_ray_sweep_rates(g->d, g->ion, flux0, g->level > 0, g->sc, g->st); }
    else { Scope s(g, "ray_sweep"); launch_ray_sweep(g->d, g->ion, flux0, g->level > 0, g->st); }
  } else {
    HIPCHK(hipMemsetAsync(g->d.ph_rate, 0, (size_t)g->d.nc*sizeof(Real), g->st));
  }
  if (!(g->d.cfg.fused_rates && g->nradplane > 0 && g->rad_dir == -1)) { Scope s(g, "ion_rates"); launch_ion_rates(g->d, g->ion, g->sc, g->st); }
  return 0;
}

int aa_ion_rates(aa_grid *g, double *dt_chem, double *dt_therm)
{
  int rc;
  if (!g->slab.empty()) return slabs_ion_rates(g, dt_chem, dt_therm);
  if (g->ion_fused) return fail(-1, "[aa_ion_rates]: this Grid runs the one-kernel sub-cycle (aa_ion_pass / aa_ion_pick / aa_ion_fetch)");
  if ((rc = aa_ion_arm(g))) return rc;
  if ((rc = ion_sweep_and_rates(g))) return rc;
  if ((rc = fetch_scalars(g))) return rc;
  if (g->sc_host->neg_dt_chem) return fail(-4, "[compute_chem_rates]: negative dt_chem");   // ionrad_3d.c:389-391
  *dt_chem = bits_to_double(g->sc_host->dt_chem);
  *dt_therm = bits_to_double(g->sc_host->dt_therm);
  return 0;
}

int aa_ion_update(aa_grid *g, double dt, long long *cellcount, double *dt_hydro)
{
  g->cfl_ready = false; g->active_dirty = true;
  if (!g->slab.empty()) return slabs_ion_update(g, dt, cellcount, dt_hydro);
  if (g->ion_fused) return fail(-1, "[aa_ion_update]: this Grid runs the one-kernel sub-cycle (aa_ion_pass / aa_ion_pick / aa_ion_fetch)");
  HIPCHK(hipMemsetAsync(&g->sc->max_dti, 0, 2*sizeof(unsigned long long), g->st));
  { Scope s(g, "ion_update"); launch_ion_update(g->d, g->ion, dt, g->sc, g->st); }
  int rc = fetch_scalars(g); if (rc) return rc;
  if (cellcount) *cellcount = (long long)g->sc_host->cellcount;
  if (dt_hydro) *dt_hydro = g->p.cour_no/bits_to_double(g->sc_host->max_dti);
  return 0;
}

// One sub-cycle of ion_radtransfer_3d with the step chosen on the device (ionrad_3d.c:919-971): ray
// sweep, rates, k_ion_pick, update -- and ONE read-back.  `limit` is the hydro dt (root) or the coarse
// time (refined level).  The first call of an ion step must find the reductions armed (aa_ion_arm).
int aa_ion_arm(aa_grid *g)
{
  if (!g->slab.empty()) return fail(-1, "[aa_ion_arm]: not available on a Grid cut into slabs (aa_ion_run / aa_ion_rates + aa_ion_update)");
  DevScalars init; memset(&init, 0, sizeof init);
  init.dt_chem = double_to_bits(DBL_MAX); init.dt_therm = double_to_bits(DBL_MAX);
  *g->sc_host = init;
  HIPCHK(hipMemcpyAsync(g->sc, g->sc_host, sizeof(DevScalars), hipMemcpyHostToDevice, g->st));
  return 0;
}
int aa_ion_subcycle(aa_grid *g, double dt_done, double limit, double *dt, int *limit_hit, double *dt_chem,
                    double *dt_therm, long long *cellcount, double *dt_hydro)
{
  g->cfl_ready = false; g->active_dirty = true;
  if (!g->slab.empty()) return fail(-1, "[aa_ion_subcycle]: not available on a Grid cut into slabs (aa_ion_run / aa_ion_rates + aa_ion_update)");
  if (g->ion_fused) return fail(-1, "[aa_ion_subcycle]: this Grid runs the one-kernel sub-cycle");
  int rc;
  if ((rc = ion_sweep_and_rates(g))) return rc;
  launch_ion_pick(g->sc, dt_done, limit, g->st);
  { Scope s(g, "ion_update"); launch_ion_update_sel(g->d, g->ion, g->sc, g->st); }
  if ((rc = fetch_scalars(g))) return rc;
  if (g->sc_host->neg_out) return fail(-4, "[compute_chem_rates]: negative dt_chem");   // ionrad_3d.c:389-391
  *dt = g->sc_host->dt_sel; *limit_hit = g->sc_host->limit_hit;
  *dt_chem = g->sc_host->dt_chem_out; *dt_therm = g->sc_host->dt_therm_out;
  *cellcount = (long long)g->sc_host->cellcount;
  *dt_hydro = g->p.cour_no/bits_to_double(g->sc_host->max_dti);
  return 0;
}

// ---- the one-kernel sub-cycle (ion_pass.hip), as phases: a driver that reduces over ranks puts ONE collective
// (an all-gather of AA_ION_WORDS doubles per rank, on this Grid's stream) between aa_ion_pass and aa_ion_pick
int aa_ion_is_fused(const aa_grid *g) { return g->ion_fused ? 1 : 0; }

// pass n: update(n-1) with the dt aa_ion_pick chose (if `update`), then sweep(n) + rates(n) (if `sweep`); this
// Grid's words of the reduction go to dev_words (DEVICE, AA_ION_WORDS doubles; NULL: kept in the Grid)
int aa_ion_pass(aa_grid *g, int update, int sweep, double *dev_words)
{
  g->cfl_ready = false; g->active_dirty = true;
  if (!g->ion_fused) return fail(-1, "[aa_ion_pass]: this Grid runs the two-kernel sub-cycle (aa_ion_rates / aa_ion_update)");
  if (!g->slab.empty()) {
    if (dev_words) return fail(-1, "[aa_ion_pass]: a Grid cut into slabs reduces over its slabs itself");
    return slabs_ion_pass(g, update, sweep);
  }
  if (!update && !sweep) return fail(-1, "[aa_ion_pass]: nothing to do");
  g->mb_prepublished = 0;
  if (update) {
    // relying on the rates of the previous sweep makes that sweep the one that counts
    if (!g->ion_pending) return fail(-1, "[aa_ion_pass]: update without a preceding sweep");
    g->ion_cur ^= 1; g->ion_pending = false;
  }
  // :264-271: a refined level starts every ray from the flux its parent left in EdgeFlux[..][..][0]; no radiation plane:
  // flux 0 (every zone's ph_rate stays 0, as after ph_rate_init)
  const Real flux0 = (g->nradplane > 0) ? ion_flux0(g) : 0.0;
  const bool begin = g->ion_begin_due;
  if (begin && update) return fail(-1, "[aa_ion_pass]: the first pass of an ion step cannot apply an update");
  g->ion_begin_due = false;
  // aa_ion_speculate: the first pass also applies the first sub-cycle's update with the whole step (k_ion_pass)
  const Real spec_dt = (begin && g->ion_spec_dt >= 0.0) ? g->ion_spec_dt : -1.0;
  if (!update) g->ion_spec_armed = spec_dt >= 0.0;
  g->ion_spec_dt = -1.0;
  // which form a speculating first pass takes (LaunchCfg ion_lean) ...
  const bool lean = spec_dt >= 0.0 && (g->d.cfg.ion_lean == 1 || (g->d.cfg.ion_lean < 0 && g->ion_lean_next));
  if (!update && begin) { g->ion_step_spec = spec_dt >= 0.0; g->ion_step_lean = lean; if (spec_dt >= 0.0) g->ion_lean_n[lean ? 1 : 0]++; }
  if (update) g->ion_step_updates++;
  // ... and the lean form's way back, in front of the first updating pass (ion_spec_armed: until the pick behind it): one launch that
  // leaves at once unless the pick refuted the speculation (spec_state 2); it sweeps into the buffer the first pass filled (ion_cur
  // has just moved on) and counts with the updating pass's stage
  const bool redo = update && g->ion_spec_armed && g->ion_step_lean;
  { Scope s(g, update ? (sweep ? "ion_pass" : "ion_pass_last") : (begin ? "ion_pass_begin" : "ion_pass_first"));
    if (redo) launch_ion_lean_redo(g->d, g->ion, flux0, g->level > 0 && g->nradplane > 0, g->sc, g->ion_cur ^ 1, g->ion_part + ion_pass_blocks(g->d), g->st);
    launch_ion_pass(g->d, g->ion, update != 0, sweep != 0, begin, flux0, g->level > 0 && g->nradplane > 0, g->sc, g->ion_cur,
                    g->ion_part, dev_words ? dev_words : g->ion_words, g->st, spec_dt, !g->ion_fuse_pick, lean); }
  if (sweep) g->ion_pending = true;
  HIPCHK(hipGetLastError());
  return 0;
}

// Before the first pass of an ion step (after aa_ion_begin): `limit` is the step the sub-cycles have to cover (the hydro
// step, or what is left of the coarse time on a refined level -- the value aa_ion_pick will be given).  The first pass then
// also applies the first sub-cycle's update with that whole step; where the reduction confirms it -- the stationary regime,
// ONE sub-cycle per step -- the closing update pass has nothing left to do (k_ion_pass).  Results are the same bit for bit.
int aa_ion_speculate(aa_grid *g, double limit)
{
  if (!g->ion_fused || !g->d.cfg.ion_spec_on) return 0;
  if (!g->slab.empty()) { for (aa_grid *c : g->slab) { c->ion_spec_dt = c->ion_begin_due ? limit : -1.0; c->ion_spec_limit = limit; } return 0; }
  g->ion_spec_dt = g->ion_begin_due ? limit : -1.0;      // (only the pass that also does the step's entry can speculate)
  g->ion_spec_limit = limit;
  return 0;
}

// ionrad_3d.c:941-967 from the words of all ranks (DEVICE, nranks x AA_ION_WORDS doubles; NULL: this Grid's own): books
// the update the pass just applied (its step, the time covered so far -- kept on the device) and picks the step of the
// next one, cut back to `limit`; `first` = the pass was the first of the ion step (no update applied yet)
int aa_ion_pick(aa_grid *g, const double *dev_words_all, int nranks, int first, double limit)
{
  if (!g->ion_fused) return fail(-1, "[aa_ion_pick]: this Grid runs the two-kernel sub-cycle");
  if (!g->slab.empty()) return slabs_ion_pick(g, first, limit);
  if (first && g->ion_spec_armed && limit != g->ion_spec_limit)
    return fail(-1, "[aa_ion_pick]: limit %.17g, but aa_ion_speculate was told %.17g", limit, g->ion_spec_limit);
  if (g->ion_fuse_pick) {      // (ion_run_fused, one rank: the pass left its records unfolded)
    if (dev_words_all) return fail(-1, "[aa_ion_pick]: internal: a fused pick with gathered words");
    // (not the first pick of an ion step: aa_ion_fetch follows at once -- the kernel publishes the scalars itself)
    const bool pub = !first && g->d.cfg.mailbox && g->mb_dev;
    if (pub) g->mb_prepublished = ++g->mb_seq;
    launch_ion_reduce_pick(g->d, g->ion_part, g->ion_words, g->sc, first, limit, g->st, first ? (g->ion_spec_armed ? 1 : 0) : 0,
                           pub ? g->mb_dev : nullptr, pub ? g->mb_seq : 0ULL);
  } else
  launch_ion_pick2(dev_words_all ? dev_words_all : g->ion_words, dev_words_all ? nranks : 1, g->sc, first, limit, g->st,
                   first ? (g->ion_spec_armed ? 1 : 0) : 0);
  if (!first) g->ion_spec_armed = false;
  HIPCHK(hipGetLastError());
  return 0;
}

// the ONE read-back of a sub-cycle, after pass + pick: of the update that pass applied its step `dt`, whether that step
// was cut back to the limit, the stop criteria's operands (cells out of range, dt_hydro) and `neg` = compute_chem_rates'
// negative-dt_chem flag of the rates the step came from; dt_chem / dt_therm are those of the NEXT step (diagnostics)
int aa_ion_fetch(aa_grid *g, double *dt, int *limit_hit, double *dt_chem, double *dt_therm, long long *cellcount, double *dt_hydro, int *neg)
{
  // (a Grid cut into slabs: every slab has picked from the gathered words; slab 0's scalars come back)
  { int rc = g->slab.empty() ? fetch_scalars(g) : slabs_fetch_scalars(g); if (rc) return rc; }
  *dt = g->sc_host->dt_applied; *limit_hit = g->sc_host->hit_applied;
  if (dt_chem) *dt_chem = g->sc_host->dt_chem_out;
  if (dt_therm) *dt_therm = g->sc_host->dt_therm_out;
  if (cellcount) *cellcount = (long long)g->sc_host->cellcount;
  if (dt_hydro) *dt_hydro = g->p.cour_no/bits_to_double(g->sc_host->max_dti);
  if (neg) *neg = g->sc_host->neg_applied;
  return 0;
}

// GridS.EdgeFlux <- the last sweep that counted (outputs, restart dumps, ionrad_prolong_snd read it).  Only marked here:
// the array is filled when somebody reads it (aa_download_edgeflux, the hand-off to a refined level) -- 16 B/zone that a
// step without output does not have to move
int aa_ion_finish(aa_grid *g)
{
  if (!g->ion_fused) return 0;
  if (!g->slab.empty()) return slabs_ion_finish(g);
  g->ion_pending = false;
  g->ion_lean_next = g->ion_step_spec && g->ion_step_updates == 1;      // (a guess at the next step's regime, not a condition of anything)
  g->ef_stale = true;
  return 0;
}
// speculating first passes queued so far in the dense and in the lean form, and lean ones that were refuted and redone densely
// (counted on the device: this call waits for the stream); a Grid cut into slabs: slab 0's, every slab counts the same
int aa_ion_lean_counts(aa_grid *g, long long *n)
{
  if (!g->ion_fused) { n[0] = n[1] = n[2] = 0; return 0; }
  aa_grid *c = g->slab.empty() ? g : g->slab[0];
  DevGuard keep;
  HIPCHK(hipSetDevice(c->p.device));
  DevScalars s;
  HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipMemcpy(&s, c->sc, sizeof(DevScalars), hipMemcpyDeviceToHost));
  n[0] = c->ion_lean_n[0]; n[1] = c->ion_lean_n[1]; n[2] = s.lean_redone;
  return 0;
}
} // extern "C"
int aa_edgeflux_ready(aa_grid *g)
{
  if (!g->ef_stale) return 0;
  { Scope s(g, "ion_finish"); launch_ion_finish(g->d, g->ion_cur, g->st); }
  g->ef_stale = false;
  HIPCHK(hipGetLastError());
  return 0;
}
extern "C" {

// the words of the pass just queued to all ranks (the driver's collective, on the Grid's stream): nothing to do with one rank
struct IonGather { double *words = nullptr; const double *all = nullptr; int nranks = 1; aa_gather_fn fn = nullptr; void *ctx = nullptr; };
static int ion_gather(const IonGather &G)
{
  if (!G.fn) return 0;
  const int rc = G.fn(G.ctx);
  return rc ? aa_fail(-5, "[ion_radtransfer_3d]: the driver's all-gather of the sub-cycle's words failed (%d)", rc) : 0;
}
// what a level's loop leaves behind: :983, :1000, :1009 pGrid->dt = dt_done where the loop says so
static int ion_ran(aa_grid *g, const IonSubcycles &r, int *niter_out, double *dt_done_out)
{
  if (r.rc) return r.rc;
  if (r.cut) g->dt = r.dt_done;
  *niter_out = r.niter; *dt_done_out = r.dt_done;
  return 0;
}

// ---- LaunchCfg ion_batch: K sub-cycles per host visit.  Which Grids take it: one rank reducing alone with the fused pick, no slabs
static bool ion_batch_on(const aa_grid *g)
{ return g->p.ion && g->ion_fused && g->slab.empty() && g->d.cfg.ion_batch > 1 && g->d.cfg.fuse_pick != 0; }
int aa_set_ion_batch(aa_grid *g, int k)
{
  if (k < 1 || k > AA_ION_BATCH_MAX) return fail(-1, "[aa_set_ion_batch]: ion_batch=%d: must be 1 (a read-back per sub-cycle) or 2..%d", k, AA_ION_BATCH_MAX);
  g->d.cfg.ion_batch = k;
  for (aa_grid *c : g->slab) c->d.cfg.ion_batch = k;
  return 0;
}
int aa_ion_batch(const aa_grid *g) { return g->slab.empty() ? g->d.cfg.ion_batch : g->slab[0]->d.cfg.ion_batch; }      // (the slabs read the environment)
// (a Grid whose ion step last came through aa_ion_radtransfer_3d_gather -- a rank of several -- reduces over the ranks every sub-cycle)
int aa_ion_batch_active(const aa_grid *g) { return (ion_batch_on(g) && !g->ion_gather_entry) ? 1 : 0; }
int aa_ion_batch_counts(const aa_grid *g, long long *n) { for (int k = 0; k < 3; k++) n[k] = g->ion_batch_n[k]; return 0; }

// The loop behind the first pass and the first pick with the stop rule on the device (k_ion_reduce_pick_q): a visit queues `b`
// sub-cycles -- each the launches aa_ion_pass(1, 1) + aa_ion_pick(0) would make, in their queued entries -- and reads back once,
// behind the last pick's publication.  The kernels take cur, flux0 and limit by value: ion_cur moves per QUEUED sub-cycle here and
// is set to what the EXECUTED ones leave behind the read-back, as are the other words the per-sub-cycle loop keeps.  The first
// visit is as long as the Grid's previous ion step was (at most K, at least 1: a step behind a one-sub-cycle step is launch for
// launch the per-sub-cycle loop's), later ones K.
static int ion_run_queued(aa_grid *g, bool fine, double limit, IonSubcycles *r)
{
  const int K = g->d.cfg.ion_batch;
  const Real flux0 = (g->nradplane > 0) ? ion_flux0(g) : 0.0;
  const bool fe = g->level > 0 && g->nradplane > 0;
  const bool pub = g->d.cfg.mailbox && g->mb_dev;
  int b = g->ion_prev_niter < 1 ? 1 : (g->ion_prev_niter < K ? g->ion_prev_niter : K), queued = 0, rc;
  const int cur0 = g->ion_cur;
  for (;;) {
    { Scope s(g, "ion_pass");
    for (int i = 0; i < b; i++, queued++) {
      const bool redo = queued == 0 && g->ion_spec_armed && g->ion_step_lean, last = i == b - 1;
      g->ion_cur ^= 1;
      g->mb_prepublished = (last && pub) ? ++g->mb_seq : 0;
      launch_ion_subcycle_q(g->d, g->ion, redo, flux0, fe, g->sc, g->ion_cur, g->ion_part, g->ion_words, fine ? 1 : 0, limit, g->p.cour_no, g->st,
                            (last && pub) ? g->mb_dev : nullptr, (last && pub) ? g->mb_seq : 0ULL);
    } }
    HIPCHK(hipGetLastError());
    g->ion_spec_armed = false;
    if ((rc = fetch_scalars(g))) return rc;
    g->ion_batch_n[0]++;
    if (g->sc_host->ion_stop != 0) break;
    b = K;
  }
  const DevScalars &h = *g->sc_host;
  const int ran = h.ion_niter + (h.ion_stop == ION_STOP_NEG ? 1 : 0);      // sub-cycles whose passes ran
  g->ion_cur = cur0 ^ (ran & 1); g->ion_pending = true; g->ion_step_updates = ran;
  g->ion_batch_n[1] += ran; g->ion_batch_n[2] += queued - ran;
  g->ion_prev_niter = h.ion_niter;
  if (h.ion_stop == ION_STOP_NEG) { r->rc = fail(-4, "[compute_chem_rates]: negative dt_chem"); return 0; }      // ionrad_3d.c:389-391
  r->rc = 0; r->niter = h.ion_niter; r->dt_done = h.dt_done; r->cut = h.ion_stop == ION_STOP_CUT;
  return 0;
}

// the one-kernel sub-cycle: pass / gather / pick / fetch
static int ion_run_fused(aa_grid *g, bool fine, double limit, int *niter_out, double *dt_done_out, const IonGather &G = IonGather())
{
  int rc;
  const double *all = G.fn ? G.all : nullptr;
  const int nr = G.fn ? G.nranks : 1;
  // one rank: every pass of this loop is followed by its pick with nothing in between -- fold and pick in one launch
  struct FuseGuard { aa_grid *g; ~FuseGuard() { g->ion_fuse_pick = false; } } fuse_guard{g};
  g->ion_fuse_pick = !G.fn && g->d.cfg.fuse_pick != 0;
  if ((rc = aa_ion_begin(g))) return rc;
  if ((rc = aa_ion_speculate(g, limit))) return rc;                          // (the first pass may already apply update(0) with the whole step)
  if ((rc = aa_ion_pass(g, 0, 1, G.fn ? G.words : nullptr))) return rc;      // sweep(0) + rates(0)
  if ((rc = ion_gather(G))) return rc;
  if ((rc = aa_ion_pick(g, all, nr, 1, limit))) return rc;                   // -> dt_0 (stays on the device)
  if (!G.fn && !g->ion_gather_entry && ion_batch_on(g)) {
    IonSubcycles q = {0, 0, 0.0, false};
    if ((rc = ion_run_queued(g, fine, limit, &q))) return rc;
    if (q.rc) return q.rc;
    if ((rc = aa_ion_finish(g))) return rc;
    return ion_ran(g, q, niter_out, dt_done_out);
  }
  const IonSubcycles r = ion_subcycles(fine, [&](double, double *dt, int *hit, long long *cellcount, double *dt_hydro) -> int {
    // update(n) with the step picked on the device, then -- unless that step was cut back to the limit -- sweep(n+1) and
    // rates(n+1), speculatively: whether the loop goes on is only known from this pass's own reductions
    int rc, neg;
    if ((rc = aa_ion_pass(g, 1, 1, G.fn ? G.words : nullptr))) return rc;
    if ((rc = ion_gather(G))) return rc;
    if ((rc = aa_ion_pick(g, all, nr, 0, limit))) return rc;
    if ((rc = aa_ion_fetch(g, dt, hit, nullptr, nullptr, cellcount, dt_hydro, &neg))) return rc;   // the one read-back
    if (neg) return fail(-4, "[compute_chem_rates]: negative dt_chem");      // ionrad_3d.c:389-391 (of the rates behind dt)
    return 0;
  });
  if (r.rc) return r.rc;
  g->ion_prev_niter = r.niter;
  if ((rc = aa_ion_finish(g))) return rc;
  return ion_ran(g, r, niter_out, dt_done_out);
}

// the two-kernel sub-cycle, the step picked on the device: ONE read-back per sub-cycle
static int ion_run_phased(aa_grid *g, bool fine, double limit, int *niter_out, double *dt_done_out)
{
  int rc;
  if ((rc = aa_ion_begin(g))) return rc;
  if ((rc = aa_ion_arm(g))) return rc;
  return ion_ran(g, ion_subcycles(fine, [&](double dt_done, double *dt, int *hit, long long *cellcount, double *dt_hydro) -> int {
    double dt_chem, dt_therm;
    return aa_ion_subcycle(g, dt_done, limit, dt, hit, &dt_chem, &dt_therm, cellcount, dt_hydro);
  }), niter_out, dt_done_out);
}

// the two-kernel sub-cycle on a Grid cut into slabs (short rays): rates and update reduce over the slabs on the host, which
// picks the step in between -- two read-backs per slab and sub-cycle, as under MPI
static int ion_run_host_picked(aa_grid *g, bool fine, double limit, int *niter_out, double *dt_done_out)
{
  int rc;
  if ((rc = aa_ion_begin(g))) return rc;
  return ion_ran(g, ion_subcycles(fine, [&](double dt_done, double *dt, int *hit, long long *cellcount, double *dt_hydro) -> int {
    double dt_chem, dt_therm;
    int rc;
    if ((rc = aa_ion_rates(g, &dt_chem, &dt_therm))) return rc;
    *dt = ion_pick_step(dt_chem, dt_therm, dt_done, limit, hit);
    return aa_ion_update(g, *dt, cellcount, dt_hydro);
  }), niter_out, dt_done_out);
}

int aa_ion_run(aa_grid *g, int finegrid, double limit, int *niter_out, double *dt_done_out)
{
  g->cfl_ready = false; g->active_dirty = true;
  g->ion_gather_entry = false;
  if (g->ion_fused) return ion_run_fused(g, finegrid != 0, limit, niter_out, dt_done_out);
  return g->slab.empty() ? ion_run_phased(g, finegrid != 0, limit, niter_out, dt_done_out)
                         : ion_run_host_picked(g, finegrid != 0, limit, niter_out, dt_done_out);
}

int aa_ion_radtransfer_3d(aa_grid *g, int *niter_out)
{
  // ionrad_3d.c:862-1047, root level
  int niter = 0, rc; double dt_done = 0.0;
  if ((rc = aa_ion_run(g, 0, g->dt, &niter, &dt_done))) return rc;
  if ((rc = ion_root_close(g, niter, dt_done, nullptr))) return rc;
  if (niter_out) *niter_out = niter;
  return 0;
}

int aa_ion_radtransfer_3d_gather(aa_grid *g, double *dev_words, const double *dev_words_all, int nranks, aa_gather_fn gather,
                                 void *ctx, int *niter_out)
{
  g->cfl_ready = false; g->active_dirty = true;
  if (!g->slab.empty()) return fail(-1, "[aa_ion_radtransfer_3d_gather]: a Grid cut into slabs reduces over its slabs itself (aa_ion_radtransfer_3d)");
  if (!g->ion_fused) return fail(-1, "[aa_ion_radtransfer_3d_gather]: this Grid runs the two-kernel sub-cycle (aa_ion_rates / aa_ion_update)");
  if (gather && (!dev_words || !dev_words_all || nranks < 1)) return fail(-1, "[aa_ion_radtransfer_3d_gather]: word buffers");
  g->ion_gather_entry = true;
  IonGather G; G.words = dev_words; G.all = dev_words_all; G.nranks = nranks; G.fn = gather; G.ctx = ctx;
  int niter = 0, rc; double dt_done = 0.0;
  if ((rc = ion_run_fused(g, false, g->dt, &niter, &dt_done, G))) return rc;
  if ((rc = ion_root_close(g, niter, dt_done, nullptr))) return rc;
  if (niter_out) *niter_out = niter;
  return 0;
}

int aa_host_syncs(aa_grid *g, int reset)
{
  int n = g->host_syncs; if (reset) g->host_syncs = 0;
  for (aa_grid *c : g->slab) { n += c->host_syncs; if (reset) c->host_syncs = 0; }
  return n;
}

int aa_start(aa_grid *g)
{
  int rc;
  if ((rc = aa_bvals_mhd(g))) return rc;
  if ((rc = aa_bvals_ionrad(g))) return rc;
  return aa_new_dt(g);
}

int aa_step(aa_grid *g, int *niter_out)
{
  int rc, niter = 0;
  if (g->p.ion && g->nradplane > 0) {                       // main.c:546-556
    if ((rc = aa_ion_radtransfer_3d(g, &niter))) return rc;
    if ((rc = aa_bvals_mhd(g))) return rc;
  }
  // (between the integrator and new_dt this loop only pins zones: the integrator may leave new_dt's maxima behind)
  const bool keep_opt = g->cfl_in_update;
  if (g->slab.empty() && g->d.cfg.cfl_step) g->cfl_in_update = true;      // (both builds since round 4: aa_cfl_in_update)
  if (g->one_d) rc = (g->p.integrator == 1 ? aa_integrate_1d_vl(g) : aa_integrate_1d_ctu(g));     // integrate.c:36-47
  else if (g->two_d) rc = (g->p.integrator == 1 ? aa_integrate_2d_vl(g) : aa_integrate_2d_ctu(g));     // integrate.c:49-58
  else
  rc = (g->p.integrator == 1 ? aa_integrate_3d_vl(g) : aa_integrate_3d_ctu(g));                    // :572-585
  g->cfl_in_update = keep_opt;
  if (rc) return rc;
  if (g->npin > 0 && (rc = aa_apply_pinned_cells(g))) return rc;   // Userwork_in_loop :597
  g->nstep++; g->time += g->dt;                              // :618-626
  if ((rc = aa_new_dt(g))) return rc;                        // :629
  if ((rc = aa_bvals_mhd(g))) return rc;                     // :635-644
  if (niter_out) *niter_out = niter;
  return 0;
}

// ---- x3 halo ------------------------------------------------------------------------------
#define NO_SLABS(name) if (!g->slab.empty()) return fail(-1, "[" name "]: not available on a Grid cut into slabs"); \
  if (g->one_d) return fail(-1, "[" name "]: not available on a 1-D Grid (one Grid, no halo exchange)"); \
  if (g->two_d) return fail(-1, "[" name "]: not available on a 2-D Grid (one Grid, no halo exchange)")
long long aa_halo_doubles(const aa_grid *g)      // (a Grid cut into slabs exchanges its halos itself: 0)
{ return g->slab.empty() ? (long long)g->d.N1*g->d.N2*AA_NGHOST*(5 + g->p.nscal) : 0LL; }
int aa_pack_x3(aa_grid *g, int side, double *buf)
{
  NO_SLABS("aa_pack_x3");
  Scope s(g, "halo_pack");
  const int k0 = side == 0 ? g->d.ks : g->d.ke - AA_NGHOST + 1;    // pack_ix3 / pack_ox3
  launch_pack_x3(g->d, 5 + g->p.nscal, k0, buf, g->st);
  return 0;
}
int aa_unpack_x3(aa_grid *g, int side, const double *buf)
{
  NO_SLABS("aa_unpack_x3");
  Scope s(g, "halo_unpack");
  const int k0 = side == 0 ? g->d.ks - AA_NGHOST : g->d.ke + 1;    // unpack_ix3 / unpack_ox3
  launch_unpack_x3(g->d, 5 + g->p.nscal, k0, buf, g->st);
  return 0;
}

// x2 halo of an x2 x x3 pencil decomposition (init_mesh.c:526-620 allows any NGrid_x2 x NGrid_x3; never x1: the rays):
// bvals_mhd.c:2462-2560 pack_ix2 / pack_ox2, :2896-3000 unpack.  Order of a bvals_mhd call with pencils: x1 sides
// (aa_bvals_mhd_side), then the x2 exchange / the physical x2 sides, then x3 -- so that the corners travel (:170).
long long aa_halo_doubles_x2(const aa_grid *g)
{ return g->slab.empty() ? (long long)g->d.N1*AA_NGHOST*(g->d.ke - g->d.ks + 1)*(5 + g->p.nscal) : 0LL; }
int aa_pack_x2(aa_grid *g, int side, double *buf)
{
  NO_SLABS("aa_pack_x2");
  Scope s(g, "halo_pack");
  const int j0 = side == 0 ? g->d.js : g->d.je - AA_NGHOST + 1;    // pack_ix2 / pack_ox2
  launch_pack_x2(g->d, 5 + g->p.nscal, j0, buf, g->st);
  return 0;
}
int aa_unpack_x2(aa_grid *g, int side, const double *buf)
{
  NO_SLABS("aa_unpack_x2");
  g->inner_swept = false; g->cfl_ready = false;      // (ghost zones only: the host's active zones stay current)
  Scope s(g, "halo_unpack");
  const int j0 = side == 0 ? g->d.js - AA_NGHOST : g->d.je + 1;    // unpack_ix2 / unpack_ox2
  launch_unpack_x2(g->d, 5 + g->p.nscal, j0, buf, g->st);
  return 0;
}

// The same halos for a driver that moves them itself through HOST buffers (the reference's own MPI ranks on the shim,
// bvals_mhd.c:296-493 with MPI_Isend / MPI_Irecv): dir 1 = x2, 2 = x3; get = pack_i* / pack_o* into host_buf, put = the
// ghost planes from host_buf.  The packed block is staged in the face-state area (idle outside the integrator).
long long aa_halo_doubles_dir(const aa_grid *g, int dir) { return dir == 1 ? aa_halo_doubles_x2(g) : (dir == 2 ? aa_halo_doubles(g) : 0LL); }
int aa_halo_get(aa_grid *g, int dir, int side, double *host_buf)
{
  NO_SLABS("aa_halo_get");
  if ((dir != 1 && dir != 2) || side < 0 || side > 1 || !host_buf) return fail(-1, "[aa_halo_get]: dir=%d side=%d", dir, side);
  g->inner_swept = false;
  int rc = dir == 1 ? aa_pack_x2(g, side, g->d.LR) : aa_pack_x3(g, side, g->d.LR); if (rc) return rc;
  HIPCHK(hipMemcpyAsync(host_buf, g->d.LR, (size_t)aa_halo_doubles_dir(g, dir)*sizeof(Real), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  return 0;
}
int aa_halo_put(aa_grid *g, int dir, int side, const double *host_buf)
{
  NO_SLABS("aa_halo_put");
  if ((dir != 1 && dir != 2) || side < 0 || side > 1 || !host_buf) return fail(-1, "[aa_halo_put]: dir=%d side=%d", dir, side);
  g->inner_swept = false; g->cfl_ready = false;      // (ghost zones only: the host's active zones stay current)
  HIPCHK(hipMemcpyAsync(g->d.LR, host_buf, (size_t)aa_halo_doubles_dir(g, dir)*sizeof(Real), hipMemcpyHostToDevice, g->st));
  int rc = dir == 1 ? aa_unpack_x2(g, side, g->d.LR) : aa_unpack_x3(g, side, g->d.LR); if (rc) return rc;
  HIPCHK(hipStreamSynchronize(g->st));      // (host_buf and the staging area are the caller's again)
  return 0;
}
int aa_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; } return n; }

// ---- function-level tests -------------------------------------------------------------------
int aa_test_fluxes(int nscal, double gamma, int n, const double *Ul, const double *Ur, const double *etah, double *F)
{
  const size_t nv = 5 + nscal, nb = (size_t)n*nv*sizeof(Real);
  Real *d = nullptr;
  HIPCHK(hipMalloc(&d, 3*nb + (size_t)n*sizeof(Real)));
  Real *dUl = d, *dUr = d + (size_t)n*nv, *dF = d + 2*(size_t)n*nv, *de = d + 3*(size_t)n*nv;
  HIPCHK(hipMemcpy(dUl, Ul, nb, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dUr, Ur, nb, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(de, etah, (size_t)n*sizeof(Real), hipMemcpyHostToDevice));
  launch_test_fluxes(nscal, gamma, n, dUl, dUr, de, dF, 0);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(F, dF, nb, hipMemcpyDeviceToHost));
  hipFree(d);
  return 0;
}
static int test_lr_any(int order, int nscal, double gamma, int n, const double *W, double dt, double dx, int il, int iu, double *Wl, double *Wr)
{
  const size_t nv = 5 + nscal, nb = (size_t)n*nv*sizeof(Real);
  const int h = (order == 3) ? 3 : 2;
  if (il < h || iu > n - 1 - h) return fail(-1, "[aa_test_lr_states]: W must cover [il-%d, iu+%d]", h, h);
  Real *d = nullptr;
  HIPCHK(hipMalloc(&d, 3*nb));
  Real *dW = d, *dWl = d + (size_t)n*nv, *dWr = d + 2*(size_t)n*nv;
  HIPCHK(hipMemcpy(dW, W, nb, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dWl, Wl, nb, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dWr, Wr, nb, hipMemcpyHostToDevice));
  if (order == 3) launch_test_lr_ppm(nscal, gamma, n, dW, dt, dx, il, iu, dWl, dWr, 0);
  else launch_test_lr(nscal, gamma, n, dW, dt, dx, il, iu, dWl, dWr, 0);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(Wl, dWl, nb, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(Wr, dWr, nb, hipMemcpyDeviceToHost));
  hipFree(d);
  return 0;
}
int aa_test_lr_states(int nscal, double gamma, int n, const double *W, double dt, double dx, int il, int iu, double *Wl, double *Wr)
{ return test_lr_any(2, nscal, gamma, n, W, dt, dx, il, iu, Wl, Wr); }
int aa_test_lr_states_ppm(int nscal, double gamma, int n, const double *W, double dt, double dx, int il, int iu, double *Wl, double *Wr)
{ return test_lr_any(3, nscal, gamma, n, W, dt, dx, il, iu, Wl, Wr); }

// the scaling-free quotient / square root of hydro_dev.h beside hipcc's own: out[5][n] = x_div(a,b), a/b, x_sqrt(a), sqrt(a),
// x_div_r(a, b, 1/b)
int aa_test_xdiv(int n, const double *a, const double *b, double *out)
{
  if (n <= 0) return fail(-1, "[aa_test_xdiv]: n = %d", n);
  Real *d = nullptr;
  HIPCHK(hipMalloc(&d, 7*(size_t)n*sizeof(Real)));
  HIPCHK(hipMemcpy(d, a, (size_t)n*sizeof(Real), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d + n, b, (size_t)n*sizeof(Real), hipMemcpyHostToDevice));
  launch_test_xdiv(n, d, d + n, d + 2*(size_t)n, 0);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, d + 2*(size_t)n, 5*(size_t)n*sizeof(Real), hipMemcpyDeviceToHost));
  hipFree(d);
  return 0;
}

// exp / log of the one-kernel sub-cycle (ion_pass.hip) on n values (n a multiple of 4): ye = exp(x), yl = ln|x|
// the marching kernels' zone accessors at byte offsets 0, 2^31 - 8, 2^31 and 2^32 - 8 of a field of 4 GiB (k_test_zone_offsets).
// The field lies 2^31 bytes inside its allocation: an offset that a faulty accessor sign-extended (or cut to 31 bits) still lands in
// memory this call owns, and shows as a word missing where the host looks for it.
int aa_test_zone_offsets(unsigned stride_bytes, double *stored, double *loaded)
{
  if (!stored || !loaded) return fail(-1, "[aa_test_zone_offsets]: null argument");
  if (stride_bytes % 8u || stride_bytes > (1u << 30)) return fail(-1, "[aa_test_zone_offsets]: stride of %u bytes: a multiple of 8 up to 2^30", stride_bytes);
  const unsigned off[4] = {0u, 0x7ffffff8u, 0x80000000u, 0xfffffff8u};
  const size_t front = (size_t)1 << 31, field = (size_t)1 << 32;
  char *pool = nullptr;
  Real *out = nullptr;
  hipError_t e = hipMalloc(&pool, front + field + (size_t)stride_bytes + 64);
  if (e != hipSuccess) return fail(-2, "[aa_test_zone_offsets]: hipMalloc of 6.5 GB failed: %s", hipGetErrorString(e));
  if (hipMalloc(&out, 12*sizeof(Real)) != hipSuccess) { hipFree(pool); return fail(-2, "[aa_test_zone_offsets]: hipMalloc"); }
  char *base = pool + front;
  int rc = 0;
  for (int l = 0; l < 4 && !rc; l++)
    for (int s = 0; s < 2 && !rc; s++)
      if (hipMemset(base + (size_t)off[l] + (s ? (size_t)stride_bytes : 0), 0, sizeof(Real)) != hipSuccess) rc = -2;
  if (!rc && hipMemset(out, 0, 12*sizeof(Real)) != hipSuccess) rc = -2;
  if (!rc) {
    launch_test_zone_offsets((Real *)base, off, stride_bytes, 0, out, 0);
    launch_test_zone_offsets((Real *)base, off, stride_bytes, 1, out, 0);
    if (hipDeviceSynchronize() != hipSuccess) rc = -2;
  }
  for (int l = 0; l < 4 && !rc; l++)
    for (int s = 0; s < 2 && !rc; s++)
      if (hipMemcpy(stored + 4*s + l, base + (size_t)off[l] + (s ? (size_t)stride_bytes : 0), sizeof(Real), hipMemcpyDeviceToHost) != hipSuccess) rc = -2;
  if (!rc && hipMemcpy(loaded, out, 12*sizeof(Real), hipMemcpyDeviceToHost) != hipSuccess) rc = -2;
  hipFree(out); hipFree(pool);
  return rc ? fail(rc, "[aa_test_zone_offsets]: %s", hipGetErrorString(hipGetLastError())) : 0;
}

int aa_test_explog(int n, const double *x, double *ye, double *yl)
{
  if (n <= 0 || n % 4) return fail(-1, "[aa_test_explog]: n must be a positive multiple of 4");
  Real *d = nullptr;
  HIPCHK(hipMalloc(&d, 3*(size_t)n*sizeof(Real)));
  HIPCHK(hipMemcpy(d, x, (size_t)n*sizeof(Real), hipMemcpyHostToDevice));
  launch_test_explog(n, d, d + n, d + 2*(size_t)n, 0);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(ye, d + n, (size_t)n*sizeof(Real), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(yl, d + 2*(size_t)n, (size_t)n*sizeof(Real), hipMemcpyDeviceToHost));
  hipFree(d);
  return 0;
}

// the folds and step picks of the radiation sub-cycle (k_ion_reduce, k_ion_reduce_pick, k_ion_pick2 of ion_pass.hip; k_ion_pick of
// ion_kernels.hip) over n records and the scalars of a previous call: see include/athena_amd.h for the layout of a row
static void pick_row_to_scalars(const double *v, DevScalars *s)
{
  memset(s, 0, sizeof *s);
  if (!v) return;
  s->dt_sel = v[0]; s->limit_hit = (int)v[1]; s->dt_done = v[2]; s->dt_applied = v[3]; s->hit_applied = (int)v[4]; s->neg_applied = (int)v[5];
  s->spec_state = (int)v[6]; s->dt_chem_out = v[7]; s->dt_therm_out = v[8]; s->neg_out = (int)v[9];
  s->max_dti = double_to_bits(v[10]); s->cellcount = (unsigned long long)v[11];
  s->dt_chem = double_to_bits(v[12]); s->dt_therm = double_to_bits(v[13]); s->neg_dt_chem = (int)v[14];
}
static void pick_scalars_to_row(const DevScalars &s, double *v)
{
  v[0] = s.dt_sel; v[1] = s.limit_hit; v[2] = s.dt_done; v[3] = s.dt_applied; v[4] = s.hit_applied; v[5] = s.neg_applied;
  v[6] = s.spec_state; v[7] = s.dt_chem_out; v[8] = s.dt_therm_out; v[9] = s.neg_out;
  v[10] = bits_to_double(s.max_dti); v[11] = (double)s.cellcount;
  v[12] = bits_to_double(s.dt_chem); v[13] = bits_to_double(s.dt_therm); v[14] = s.neg_dt_chem; v[15] = 0.0;
}
int aa_test_ion_pick(int n, const double *rec, int first, double limit, int spec_armed, const double *prev, double *words, double *out)
{
  if (n < 1 || n > (1 << 20)) return fail(-1, "[aa_test_ion_pick]: n = %d", n);
  static_assert(sizeof(IonPart) == 5*sizeof(Real), "a record is five doubles");
  const size_t nrec = (size_t)n*sizeof(IonPart), nw = 2*AA_ION_WORDS*sizeof(Real);
  char *d = nullptr;
  HIPCHK(hipMalloc(&d, nrec + nw + 3*sizeof(DevScalars)));
  IonPart *part = (IonPart*)d;
  Real *w = (Real*)(d + nrec);
  DevScalars *sc = (DevScalars*)(d + nrec + nw);
  DevScalars h[3];
  pick_row_to_scalars(prev, &h[0]); h[1] = h[0]; h[2] = h[0];
  HIPCHK(hipMemcpy(part, rec, nrec, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(w, 0xff, nw));            // (NaNs: a word a fold does not write shows)
  HIPCHK(hipMemcpy(sc, h, 2*sizeof(DevScalars), hipMemcpyHostToDevice));
  launch_test_ion_reduce(part, n, w, 0);
  launch_test_ion_reduce_pick(part, n, w + AA_ION_WORDS, sc, first, limit, spec_armed, 0);
  launch_ion_pick2(w, 1, sc + 1, first, limit, 0, spec_armed);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(words, w, nw, hipMemcpyDeviceToHost));
  // the two-kernel form keeps its reductions in the scalars (k_ion_rates' atomics): here the fold of the records
  h[2].dt_chem = double_to_bits(words[0]); h[2].dt_therm = double_to_bits(words[1]); h[2].max_dti = double_to_bits(words[2]);
  h[2].cellcount = (unsigned long long)words[3]; h[2].neg_dt_chem = words[4] != 0.0;
  HIPCHK(hipMemcpy(sc + 2, &h[2], sizeof(DevScalars), hipMemcpyHostToDevice));
  launch_ion_pick(sc + 2, first ? 0.0 : h[0].dt_done + h[0].dt_sel, limit, 0);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(h, sc, 3*sizeof(DevScalars), hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; k++) pick_scalars_to_row(h[k], out + (size_t)k*AA_TEST_PICK_SCALARS);
  hipFree(d);
  return 0;
}

// the sub-cycle loop with the stop rule on the device (ion_run_queued's visits) over a script: row 0 of `rec` is the record of the first
// pass, row r that of the pass of sub-cycle r.  The first pick, then visits of b0, K, K ... queued picks (k_ion_reduce_pick_q over one
// record each) with a publication behind the last pick of each and no passes in between, until the device says stop.  out: niter, dt_done,
// stop code, visits, queued picks that left at once; steps: the applied steps in order (n doubles).
int aa_test_ion_batch(int n, const double *rec, int fine, double limit, double cour_no, int K, int b0, double *out, double *steps)
{
  if (n < 2 || n > 4096) return fail(-1, "[aa_test_ion_batch]: n = %d", n);
  if (K < 1 || K > AA_ION_BATCH_MAX || b0 < 1 || b0 > K) return fail(-1, "[aa_test_ion_batch]: K = %d, first visit %d", K, b0);
  const size_t nrec = (size_t)n*sizeof(IonPart), nw = AA_ION_WORDS*sizeof(Real), nst = (size_t)(n + AA_ION_BATCH_MAX)*sizeof(Real);      // (a visit may book up to K - 1 sub-cycles past the script before the host sees it has run out)
  char *d = nullptr;
  Mailbox *mb = nullptr, *mb_dev = nullptr;
  HIPCHK(hipMalloc(&d, nrec + nw + nst + sizeof(DevScalars)));
  if (hipHostMalloc(&mb, sizeof(Mailbox), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&mb_dev, mb, 0) != hipSuccess) { hipFree(d); return fail(-2, "[aa_test_ion_batch]: no mailbox"); }
  memset(mb, 0, sizeof(Mailbox));
  IonPart *part = (IonPart*)d;
  Real *w = (Real*)(d + nrec), *st = (Real*)(d + nrec + nw);
  DevScalars *sc = (DevScalars*)(d + nrec + nw + nst);
  int rc = 0, visits = 0, queued = 0, b = b0;
  unsigned long long seq = 0;
  auto chk = [&](hipError_t e) { if (e != hipSuccess && !rc) rc = fail(-2, "[aa_test_ion_batch]: HIP error %s", hipGetErrorString(e)); return e == hipSuccess; };
  if (chk(hipMemcpy(part, rec, nrec, hipMemcpyHostToDevice)) && chk(hipMemset(w, 0, nw + nst + sizeof(DevScalars)))) {
    launch_test_ion_reduce_pick(part, 1, w, sc, 1, limit, 0, 0);
    for (;;) {
      for (int i = 0; i < b; i++, queued++) {
        const int row = (1 + queued < n) ? 1 + queued : n - 1;
        launch_test_ion_reduce_pick_q(part + row, 1, w, sc, fine, limit, cour_no, st, i == b - 1 ? mb_dev : nullptr, i == b - 1 ? ++seq : 0ULL, 0);
      }
      if (!chk(hipDeviceSynchronize())) break;
      visits++;
      if (mb->seq != seq) { rc = fail(-2, "[aa_test_ion_batch]: visit %d ended without its stamp", visits); break; }
      if (mb->s.ion_stop != 0) break;
      if (1 + queued >= n) { rc = fail(-1, "[aa_test_ion_batch]: the script of %d rows ran out with the loop open", n); break; }
      b = K;
    }
  }
  if (!rc) {
    const DevScalars &h = mb->s;
    const int ran = h.ion_niter + (h.ion_stop == ION_STOP_NEG ? 1 : 0);
    out[0] = h.ion_niter; out[1] = h.dt_done; out[2] = h.ion_stop; out[3] = visits; out[4] = queued - ran;
    chk(hipMemcpy(steps, st, (size_t)n*sizeof(Real), hipMemcpyDeviceToHost));
  }
  hipHostFree(mb); hipFree(d);
  return rc;
}

// ---- history sums (dump_history.c:157-200) ---------------------------------------------------
int aa_history(aa_grid *g, double *sums)
{
  if (!g->slab.empty()) return slabs_history(g, sums);
  g->inner_swept = false;
  // partial rows go through the face-state area, idle outside the integrator
  const int nb = launch_history(g->d, g->p.nscal, g->d.LR, g->st);
  std::vector<double> part((size_t)nb*9);
  HIPCHK(hipMemcpyAsync(part.data(), g->d.LR, part.size()*sizeof(double), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  const double dVol = g->d.dx[0]*g->d.dx[1]*g->d.dx[2];
  for (int q = 0; q < 9; q++) {
    double s = 0.0;
    for (int b = 0; b < nb; b++) s += part[(size_t)b*9 + q];
    sums[q] = dVol*s;
  }
  return 0;
}

// ---- measurement -----------------------------------------------------------------------------
// (a Grid cut into slabs reports its first slab's kernels)
int aa_profile_enable(aa_grid *g, int on)
{
  if (!g->slab.empty()) return aa_profile_enable(g->slab[0], on);
  prof_drain(g); g->prof = on != 0;
  // events for a few dozen steps ahead: a timed region then creates none (hipEventCreate showed on the small Grids of the reference's decks)
  if (on) while (g->ev_pool.size() < 4096) { hipEvent_t ev; if (hipEventCreate(&ev) != hipSuccess) break; g->ev_pool.push_back(ev); }
  return 0;
}
int aa_profile_reset(aa_grid *g)
{ if (!g->slab.empty()) return aa_profile_reset(g->slab[0]); prof_drain(g); for (auto &e : g->pe) { e.total_ms = 0; e.launches = 0; } return 0; }
int aa_profile_count(const aa_grid *g) { if (!g->slab.empty()) return aa_profile_count(g->slab[0]); return (int)g->pe.size(); }
const char *aa_profile_name(const aa_grid *g, int i)
{ if (!g->slab.empty()) return aa_profile_name(g->slab[0], i); return (i >= 0 && i < (int)g->pe.size()) ? g->pe[i].name.c_str() : ""; }
int aa_profile_get(aa_grid *g, int i, double *total_ms, long long *launches)
{
  if (!g->slab.empty()) return aa_profile_get(g->slab[0], i, total_ms, launches);
  if (i < 0 || i >= (int)g->pe.size()) return fail(-1, "[aa_profile_get]: bad index");
  prof_drain(g);
  if (total_ms) *total_ms = g->pe[i].total_ms;
  if (launches) *launches = g->pe[i].launches;
  return 0;
}

}  // extern "C"
