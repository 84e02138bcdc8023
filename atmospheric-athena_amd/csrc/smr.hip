// smr.hip -- static mesh refinement: the nested levels of a Mesh resident on one GPU.
//
// Every level is an ordinary aa_grid (its own SoA pool, dx = root dx / 2^level).  This unit adds
// what the reference adds between the levels, as kernels that read one level's arrays and write
// the other's directly in HBM -- there are no send/receive buffers (smr.c packs them only to
// feed MPI):
//   restriction + flux correction   smr.c:1207  RestrictCorrect
//   restriction of E and s[0]       smr.c:85    ionradRestrictCorrect
//   prolongation into ghost zones   smr.c:2359  Prolongate, :3068 ProCon, :3478 mcd_slope
//   radiation hand-off to the child ionrad_smr.c:345/:34  ionrad_prolong_snd / _rcv
// and the host control flow of the SMR branches of main.c:519-669, new_dt.c:32 and
// ionrad_3d.c:862.  The fluxes the reference copies into CGrid/PGrid.myFlx in Step 12e of the
// integrator (integrate_3d_ctu.c:3072) are read straight from each level's flux arrays, which
// keep the second-pass fluxes until the next integrator call.
//
// Summation orders follow the reference term by term, so the strict (-ffp-contract=off) build
// reproduces the CPU results bit for bit.
//
// A Mesh of 2-D Grids (Nx3 = 1 on every level; aa_mesh_create_2d) runs the same host control flow on kernels of its own --
// k2d_restrict, k2d_flux_correct, k2d_box_copy, k2d_prolong: the nDim == 2 branches of smr.c -- and the 2-D integrators, whose
// update kernel leaves the fluxes of the level-boundary lines in F (hydro2d_kernels.hip k2d_step_keep; integrate_2d_ctu.c:1722-1877).
//
// A Mesh whose levels are composite handles cut at the same root x3 planes (aa_create_cut) runs one such stack per device in ONE
// process: the last part of this file (one local stack per slab + what crosses slabs; the cut arithmetic is mesh_cuts.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "api_internal.h"
#include "mesh_cuts.h"

using namespace aa;

#define NG AA_NGHOST
#define AA_MAXLEV 16     /* Grids of a Mesh (one per Domain) */

namespace {

struct Link {                 // level l+1 seen from level l (init_grid.c: CGrid.ijks/ijke, myFlx != NULL)
  int cs[3], ce[3];           // overlap on the parent, parent indices incl. ghost offset
  int n[3];                   // overlap size in parent zones
  int prol[6];                // the child has a fine/coarse boundary on this side: ghost zones prolonged
  int corr[6];                // ... and the parent zone outside is on this Grid: flux-corrected here
  int cdisp[3];               // child origin minus 2 x parent origin, zones of the child's level
};

__device__ __forceinline__ Real *fld(const DevGrid &g, Real *base, int v) { return base + (long)v*g.nc; }

// ---- restriction, flux correction and the snapshot for the prolongation: smr_coupling_kernels.h, compiled twice -- as it stands
// (k_restrict, k_flux_correct, k_box_copy: dt a kernel argument) and with AA_CLOCK_ENTRY (k_restrict_dc, k_flux_correct_dc,
// k_box_copy_dc: the entries of a step queued by aa_mesh_run_3d, which read the device clock at the top).  One text, two entries:
// a body shared through an inlined function moved the by-value kernels' code (k_flux_correct's index tables went to LDS).
#include "smr_coupling_kernels.h"
#define AA_CLOCK_ENTRY 1
#include "smr_coupling_kernels.h"
#undef AA_CLOCK_ENTRY

// ---- prolongation ----------------------------------------------------------------------------
// (the snapshot of the parent zones around the child, k_box_copy, is in smr_coupling_kernels.h)
__device__ __forceinline__ Real mcd_slope(const Real vl, const Real vc, const Real vr)   // smr.c:3478
{
  const Real dvl = (vc - vl), dvr = (vr - vc);
  if (dvl > 0.0 && dvr > 0.0) {
    const Real dv = 2.0*(dvl < dvr ? dvl : dvr), dvm = 0.5*(dvl + dvr);
    return (dvm < dv ? dvm : dv);
  } else if (dvl < 0.0 && dvr < 0.0) {
    const Real dv = 2.0*(dvl > dvr ? dvl : dvr), dvm = 0.5*(dvl + dvr);
    return (dvm > dv ? dvm : dv);
  }
  return 0.0;
}

// one thread = one parent zone under 2x2x2 ghost zones of the child (ProCon, smr.c:3068); one
// launch per boundary side, in the reference's order of sides (regions overlap at edges and
// corners with identical values)
__global__ void __launch_bounds__(128)
k_prolong(DevGrid f, Link L, const Real *box, int dim_arg, int nvar)
{
  // dim_arg < 0: all sides in one launch, side = blockIdx.y (where two sides' regions overlap, at edges and corners, both write the
  // same values: every ghost zone is a function of the snapshot `box` alone)
  const int dim = (dim_arg >= 0) ? dim_arg : (int)blockIdx.y;
  if (dim_arg < 0 && !L.prol[dim]) return;
  const int lo[3] = {f.is, f.js, f.ks}, hi[3] = {f.ie, f.je, f.ke};
  int ps[3], cnt[3];
  for (int d = 0; d < 3; d++) { ps[d] = lo[d] - NG; cnt[d] = (hi[d] - lo[d] + 1 + 2*NG)/2; }
  if (dim & 1) ps[dim >> 1] = hi[dim >> 1] + 1;
  cnt[dim >> 1] = NG/2;
  const long n = (long)cnt[0]*cnt[1]*cnt[2];
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= n) return;
  const int a = (int)(lin % cnt[0]), b = (int)((lin / cnt[0]) % cnt[1]), cc = (int)(lin / ((long)cnt[0]*cnt[1]));
  const int i = ps[0] + 2*a, j = ps[1] + 2*b, k = ps[2] + 2*cc;              // lower fine zone of the 2x2x2 block
  const int b0 = L.n[0] + 6, b1 = L.n[1] + 6;
  const long nb = (long)b0*b1*(L.n[2] + 6);
  const long sb1 = b0, sb2 = (long)b0*b1;
  // parent zone in box coordinates: fine lo-4 lies in parent cs-2 = box index 1
  const long mb = (long)((k - (lo[2] - NG))/2 + 1)*sb2 + (long)((j - (lo[1] - NG))/2 + 1)*sb1 + ((i - (lo[0] - NG))/2 + 1);
  Real P[6][8];
  // d, M1, M2, M3, s0: conserved variable + limited slopes
  for (int v = 0; v < 6; v++) {
    if (v == 4 || v >= nvar) continue;
    const Real *q = box + (long)v*nb + mb;
    const Real uc = q[0];
    const Real dq1 = mcd_slope(q[-1], uc, q[1]);
    const Real dq2 = mcd_slope(q[-sb1], uc, q[sb1]);
    const Real dq3 = mcd_slope(q[-sb2], uc, q[sb2]);
    for (int kk = 0; kk < 2; kk++) for (int jj = 0; jj < 2; jj++) for (int ii = 0; ii < 2; ii++)
      P[v][kk*4 + jj*2 + ii] = uc + (0.5*ii - 0.25)*dq1 + (0.5*jj - 0.25)*dq2 + (0.5*kk - 0.25)*dq3;
  }
  {  // the internal energy, not E, is interpolated (:3146-3168)
    const Real *qd = box + mb, *q1 = box + nb + mb, *q2 = box + 2*nb + mb, *q3 = box + 3*nb + mb, *qe = box + 4*nb + mb;
#define EINT(o) (qe[o] - 0.5*(q1[o]*q1[o] + q2[o]*q2[o] + q3[o]*q3[o])/qd[o])
    const Real Pi = EINT(0);
    const Real dq1 = mcd_slope(EINT(-1), Pi, EINT(1));
    const Real dq2 = mcd_slope(EINT(-sb1), Pi, EINT(sb1));
    const Real dq3 = mcd_slope(EINT(-sb2), Pi, EINT(sb2));
#undef EINT
    for (int kk = 0; kk < 2; kk++) for (int jj = 0; jj < 2; jj++) for (int ii = 0; ii < 2; ii++) {
      const int o = kk*4 + jj*2 + ii;
      Real e = Pi + (0.5*ii - 0.25)*dq1 + (0.5*jj - 0.25)*dq2 + (0.5*kk - 0.25)*dq3;
      e += 0.5*(P[1][o]*P[1][o] + P[2][o]*P[2][o] + P[3][o]*P[3][o])/P[0][o];
      P[4][o] = e;
    }
  }
  for (int v = 0; v < nvar; v++) {
    Real *u = fld(f, f.U, v);
    for (int kk = 0; kk < 2; kk++) for (int jj = 0; jj < 2; jj++) for (int ii = 0; ii < 2; ii++)
      u[(long)(k + kk)*f.sK + (long)(j + jj)*f.sJ + (i + ii)] = P[v][kk*4 + jj*2 + ii];
  }
}

// ---- radiation hand-off (ionrad_smr.c:345 + :34, rays along +x1): the flux the parent left at
// the upstream face of the child, copied piecewise-constant onto the child's 2x2 rays.  The
// reference moves it through CGrid.ionFlx; nothing touches the parent's EdgeFlux in between. ----
__global__ void __launch_bounds__(256)
k_ionflux_prolong(DevGrid f, DevGrid c, Link L)
{
  const int w = L.n[1] + 1, h = L.n[2] + 1;
  const int lin = blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= w*h) return;
  const int jj = lin % w, kk = lin / w;
  const int j = L.cs[1] - NG + jj, k = L.cs[2] - NG + kk;                 // parent active indices
  const long cfp = (long)(c.Nx1 + 1), cfrow = (long)(c.Nx2 + 1)*cfp;
  const long ffp = (long)(f.Nx1 + 1), ffrow = (long)(f.Nx2 + 1)*ffp;
  const Real v = c.edgeflux[(long)k*cfrow + (long)j*cfp + (L.cs[0] - NG)];
  const int ks = k*2 - L.cdisp[2], js = j*2 - L.cdisp[1];                 // :97-98
#define EF(a,b) f.edgeflux[(long)(a)*ffrow + (long)(b)*ffp]
  EF(ks, js) = v;
  if (jj < w - 1) {
    if (kk < h - 1) { EF(ks+1, js+1) = v; EF(ks, js+1) = v; EF(ks+1, js) = v; }
    else EF(ks, js+1) = v;
  } else if (kk < h - 1) EF(ks+1, js) = v;
#undef EF
}

// ---- flux correction across slabs: the child's restricted x3 boundary flux as a message
// ([b][a][6]), and its application on the neighbouring slab of the parent (smr.c:1322-1340) ----
__global__ void __launch_bounds__(256)
k_flux_x3_export(DevGrid f, int side, Real *buf)
{
  const int n1 = f.Nx1/2, n2 = f.Nx2/2;
  const int lin = blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= n1*n2) return;
  const int a = lin % n1, b = lin / n1;
  const long m = (long)(side ? f.ke + 1 : f.ks)*f.sK + (long)(f.js + 2*b)*f.sJ + (f.is + 2*a);
  for (int v = 0; v < 6; v++) {
    const Real *q = fld(f, f.F, 2*6 + v) + m;
    Real s = q[0] + q[1];
    s += q[f.sJ] + q[f.sJ + 1];
    s *= 0.25;
    buf[(long)lin*6 + v] = s;
  }
}

__global__ void __launch_bounds__(256)
k_flux_x3_apply(DevGrid c, int side, int i0, int j0, int n1, int n2, int nvar, Real dt, const Real *buf)
{
  const int lin = blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= n1*n2) return;
  const int a = lin % n1, b = lin / n1;
  const int kc = side ? c.ks : c.ke, kf = side ? c.ks : c.ke + 1;
  const Real q = side ? (dt/c.dx[2]) : -(dt/c.dx[2]);
  const long mc = (long)kc*c.sK + (long)(j0 + b)*c.sJ + (i0 + a), mf = (long)kf*c.sK + (long)(j0 + b)*c.sJ + (i0 + a);
  for (int v = 0; v < nvar; v++)
    fld(c, c.U, v)[mc] -= q*(fld(c, c.F, 2*6 + v)[mf] - buf[(long)lin*6 + v]);
}

// ---- 2-D Grids (Nx3 = 1; aa_mesh_create_2d): one plane per field, five fields, the flux family F as [dir][5] with the kept
// second-pass fluxes in the global momentum order (hydro2d_kernels.hip k2d_step_keep).  A block is S2_R wavefronts of 64 lanes
// along x1; every kernel touches an outline or a ghost shell only, and none needs an atomic or LDS. ------------------------------
#define S2_W 64
#define S2_R 4

// restriction: 2x2 fine zones -> one parent zone.  smr.c Step 3a on a 2-D Grid: the pair of the lower row, plus the pair of the
// upper row, times 0.25 (the x3 pass is skipped: Nx[2] = 1)
__device__ __forceinline__ void restrict2_body(const DevGrid &f, const DevGrid &c, const Link &L)
{
  const int a = (int)blockIdx.x*S2_W + (int)threadIdx.x, b = (int)blockIdx.y*S2_R + (int)threadIdx.y;
  if (a >= L.n[0] || b >= L.n[1]) return;
  const long mc = (long)(L.cs[1] + b)*c.sJ + (L.cs[0] + a);
  const long mf = (long)(f.js + 2*b)*f.sJ + (f.is + 2*a);
#pragma unroll
  for (int v = 0; v < 5; v++) {
    const Real *q = fld(f, f.U, v) + mf;
    Real s = q[0] + q[1];
    s += q[f.sJ] + q[f.sJ + 1];
    s *= 0.25;
    fld(c, c.U, v)[mc] = s;
  }
}
__global__ void __launch_bounds__(S2_W*S2_R)
k2d_restrict(DevGrid f, DevGrid c, Link L)
{ restrict2_body(f, c, L); }

// flux correction of the parent zones just outside the child (smr.c Step 2a); the child's flux through a parent face is the sum
// of its two faces times 0.5 (Step 3c with nDim = 2).  One thread per parent face of a side; dim_arg < 0: the four sides in one
// launch, side = blockIdx.y (they correct disjoint parent zones)
__device__ __forceinline__ void flux_correct2_body(const DevGrid &f, const DevGrid &c, const Link &L, int dim_arg, Real dt)
{
  const int dim = (dim_arg >= 0) ? dim_arg : (int)blockIdx.y;
  if (dim_arg < 0 && !L.corr[dim]) return;
  const int d = dim >> 1, t = 1 - d;
  const int a = (int)blockIdx.x*S2_W + (int)threadIdx.x;
  if (a >= L.n[t]) return;
  const long sc[2] = {1, c.sJ}, sf[2] = {1, f.sJ};
  const int flo[2] = {f.is, f.js}, fhi[2] = {f.ie, f.je};
  int ic[2]; ic[t] = L.cs[t] + a;
  Real q;
  if (dim & 1) { ic[d] = L.ce[d] + 1; q =  (dt/c.dx[d]); }
  else         { ic[d] = L.cs[d] - 1; q = -(dt/c.dx[d]); }
  const long mcell = ic[1]*sc[1] + ic[0];
  ic[d] = (dim & 1) ? L.ce[d] + 1 : L.cs[d];
  const long mface_c = ic[1]*sc[1] + ic[0];
  int jf[2]; jf[t] = flo[t] + 2*a; jf[d] = (dim & 1) ? fhi[d] + 1 : flo[d];
  const long mface_f = jf[1]*sf[1] + jf[0];
#pragma unroll
  for (int v = 0; v < 5; v++) {
    const Real mine = fld(c, c.F, d*5 + v)[mface_c];
    const Real *qf = fld(f, f.F, d*5 + v) + mface_f;
    Real fine = qf[0] + qf[sf[t]];
    fine *= 0.5;
    fld(c, c.U, v)[mcell] -= q*(mine - fine);
  }
}
__global__ void __launch_bounds__(S2_W)
k2d_flux_correct(DevGrid f, DevGrid c, Link L, int dim_arg, Real dt)
{ flux_correct2_body(f, c, L, dim_arg, dt); }

// snapshot of the parent zones cs-3 .. ce+3 around the child in x1 and x2, taken when the parent "sends" (smr.c Step 1 of Prolongate)
__device__ __forceinline__ void box_copy2_body(const DevGrid &c, const Link &L, Real *box)
{
  const int b0 = L.n[0] + 6, b1 = L.n[1] + 6;
  const int i = (int)blockIdx.x*S2_W + (int)threadIdx.x, j = (int)blockIdx.y*S2_R + (int)threadIdx.y;
  if (i >= b0 || j >= b1) return;
  const long nb = (long)b0*b1;
  const long m = (long)(L.cs[1] - 3 + j)*c.sJ + (L.cs[0] - 3 + i);
#pragma unroll
  for (int v = 0; v < 5; v++) box[(long)v*nb + (long)j*b0 + i] = fld(c, c.U, v)[m];
}
__global__ void __launch_bounds__(S2_W*S2_R)
k2d_box_copy(DevGrid c, Link L, Real *box)
{ box_copy2_body(c, L, box); }

// ---- the same kernels for a step queued by aa_mesh_run_2d: the Mesh's ONE clock (hydro2d_launch.h Run2D, in device memory) is read
// at the top, as the *_dc entry points of hydro2d_kernels.hip do.  Restriction OVERWRITES the parent with a function of the child, but
// the flux correction ADDS to the parent: behind the stop (`live` = 0) both return before any store, and dt is the clock's.  The
// snapshot for the prolongation stands behind k2d_mesh_advance, which has already written the NEXT step's `live`: it asks `stepped`,
// whether the step in front of that kernel was taken (see mesh_queue_step_2d for why a snapshot behind a stop must not be retaken).
__global__ void __launch_bounds__(S2_W*S2_R)
k2d_restrict_dc(DevGrid f, DevGrid c, Link L, const Run2D *rc)
{ if (!rc->c.live) return; restrict2_body(f, c, L); }
__global__ void __launch_bounds__(S2_W)
k2d_flux_correct_dc(DevGrid f, DevGrid c, Link L, int dim_arg, const Run2D *rc)
{ if (!rc->c.live) return; flux_correct2_body(f, c, L, dim_arg, rc->c.dt); }
__global__ void __launch_bounds__(S2_W*S2_R)
k2d_box_copy_dc(DevGrid c, Link L, Real *box, const Run2D *rc)
{ if (!rc->stepped) return; box_copy2_body(c, L, box); }

// one thread = one parent zone under 2x2 ghost zones of the child.  ProCon (smr.c:3068) on a 2-D Grid: the planes below and above
// are copies of the plane itself (Step 3a, nDim == 2), so the x3 slope is mcd_slope of equal values = 0 and its term -0.25*0 adds
// nothing; k = 0 only is stored.  The four sides dim < 2*nDim; dim_arg < 0: all in one launch, side = blockIdx.z
__global__ void __launch_bounds__(S2_W*S2_R)
k2d_prolong(DevGrid f, Link L, const Real *box, int dim_arg)
{
  const int dim = (dim_arg >= 0) ? dim_arg : (int)blockIdx.z;
  if (dim_arg < 0 && !L.prol[dim]) return;
  const int lo[2] = {f.is, f.js}, hi[2] = {f.ie, f.je};
  int ps[2], cnt[2];
  for (int d = 0; d < 2; d++) { ps[d] = lo[d] - NG; cnt[d] = (hi[d] - lo[d] + 1 + 2*NG)/2; }
  if (dim & 1) ps[dim >> 1] = hi[dim >> 1] + 1;
  cnt[dim >> 1] = NG/2;
  const int a = (int)blockIdx.x*S2_W + (int)threadIdx.x, b = (int)blockIdx.y*S2_R + (int)threadIdx.y;
  if (a >= cnt[0] || b >= cnt[1]) return;
  const int i = ps[0] + 2*a, j = ps[1] + 2*b;                                 // lower fine zone of the 2x2 block
  const int b0 = L.n[0] + 6;
  const long nb = (long)b0*(L.n[1] + 6), sb1 = b0;
  // parent zone in box coordinates: fine lo-4 lies in parent cs-2 = box index 1
  const long mb = (long)((j - (lo[1] - NG))/2 + 1)*sb1 + ((i - (lo[0] - NG))/2 + 1);
  Real P[5][4];
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const Real *q = box + (long)v*nb + mb;
    const Real uc = q[0];
    const Real dq1 = mcd_slope(q[-1], uc, q[1]);
    const Real dq2 = mcd_slope(q[-sb1], uc, q[sb1]);
    for (int jj = 0; jj < 2; jj++) for (int ii = 0; ii < 2; ii++)
      P[v][jj*2 + ii] = uc + (0.5*ii - 0.25)*dq1 + (0.5*jj - 0.25)*dq2;
  }
  {  // the internal energy, not E, is interpolated
    const Real *qd = box + mb, *q1 = box + nb + mb, *q2 = box + 2*nb + mb, *q3 = box + 3*nb + mb, *qe = box + 4*nb + mb;
#define EINT(o) (qe[o] - 0.5*(q1[o]*q1[o] + q2[o]*q2[o] + q3[o]*q3[o])/qd[o])
    const Real Pi = EINT(0);
    const Real dq1 = mcd_slope(EINT(-1), Pi, EINT(1));
    const Real dq2 = mcd_slope(EINT(-sb1), Pi, EINT(sb1));
#undef EINT
    for (int jj = 0; jj < 2; jj++) for (int ii = 0; ii < 2; ii++) {
      const int o = jj*2 + ii;
      Real e = Pi + (0.5*ii - 0.25)*dq1 + (0.5*jj - 0.25)*dq2;
      e += 0.5*(P[1][o]*P[1][o] + P[2][o]*P[2][o] + P[3][o]*P[3][o])/P[0][o];
      P[4][o] = e;
    }
  }
#pragma unroll
  for (int v = 0; v < 5; v++) {
    Real *u = fld(f, f.U, v);
    for (int jj = 0; jj < 2; jj++) for (int ii = 0; ii < 2; ii++)
      u[(long)(j + jj)*f.sJ + (i + ii)] = P[v][jj*2 + ii];
  }
}

inline unsigned nblk(long n, int b) { return (unsigned)((n + b - 1)/b); }

// ---- a Mesh on in-library slabs: the x3 halo of ALL levels two neighbouring slabs share in one launch per slab.  What
// k_pack_x3 / k_unpack_x3 (hydro_kernels.hip) do for one Grid -- four k-planes, all i and j, one lane per zone with i fastest, the
// buffer of a level laid out [v][kk][j][i] -- for the levels in a row: level l's block starts nvar*first doubles into the buffer
// (the same offset on both slabs: it depends on N1 x N2 of the coarser levels only).  side = blockIdx.y: 0 the lower neighbour,
// 1 the upper one; the levels shared with a neighbour are a prefix of the slab's levels (nesting), nshare[side] of them. ----------
struct HaloLev { Real *U; long sJ, sK, nc, first; int N1, N2, kp[2], ku[2]; };   // first: lanes before this level; kp / ku: first plane packed / unpacked per side
struct HaloBatch { int nshare[2], nvar, pad; long total[2]; HaloLev lev[AA_MAXLEV]; };

template <bool PACK>
__global__ void __launch_bounds__(256)
k_halo_levels(HaloBatch B, Real *buf0, Real *buf1)
{
  const int side = (int)blockIdx.y;
  Real *buf = side ? buf1 : buf0;
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (!buf || lin >= B.total[side]) return;
  int l = 0;
  while (l + 1 < B.nshare[side] && lin >= B.lev[l + 1].first) l++;
  const HaloLev &h = B.lev[l];
  const long q = lin - h.first, plane = (long)h.N1*h.N2, ntot = plane*NG;
  const int i = (int)(q % h.N1), j = (int)((q / h.N1) % h.N2), kk = (int)(q / plane);
  const long m = (long)((PACK ? h.kp[side] : h.ku[side]) + kk)*h.sK + (long)j*h.sJ + i;
  Real *b = buf + h.first*B.nvar + q;
  for (int v = 0; v < B.nvar; v++) {
    if (PACK) b[(long)v*ntot] = h.U[(long)v*h.nc + m];
    else h.U[(long)v*h.nc + m] = b[(long)v*ntot];
  }
}

// a flux correction that crosses a cut: the child's piece on slab src ends at the cut, the parent plane outside is on slab dst
struct FluxMsg {
  int l, side, src, dst, i0, j0, n1, n2;      // link l (level l+1 on level l); side of the child's boundary
  Real *sbuf = nullptr, *rbuf = nullptr, *hbuf = nullptr;      // on src's device, on dst's device, pinned (staged route only)
  hipEvent_t sent = nullptr, done = nullptr; bool done_valid = false;
};

}  // namespace

// one local stack per slab (the aa_mesh_create_local machinery) plus what crosses slabs
struct CutMesh {
  int n = 0;                                  // slabs of the root
  mc_mesh *mc = nullptr;                      // spans, links, corr_to / corr_in (mesh_cuts.h)
  std::vector<aa_mesh*> local;                // local[s]: the pieces on slab s, root first
  std::vector<int> dev;
  bool staged = false;                        // no peer access between neighbours (or AA_SLAB_NO_PEER=1): through pinned host memory
  bool batch = true;                          // AA_MESH_HALO_BATCH=0: the exchange of all levels as one exchange per level
  std::vector<HaloBatch> hb;
  std::vector<Real*> send[2], recv[2], hstage[2];
  std::vector<hipEvent_t> packed, copied, unpacked, staged_ev;
  std::vector<bool> copied_valid, unpacked_valid;
  std::vector<hipStream_t> xfer, xout;
  bool halo_due = false;
  std::vector<FluxMsg> msgs;
  long long counts[3] = {0, 0, 0};            // of the exchanges of all levels so far: pack + unpack launches, copies, exchanges
};

// Grids in the order of the reference's loops: level by level from the root, Domains of a level in deck order
// (MeshS.Domain[nl][nd]).  Link L joins grid L+1 (the child) to grid par[L] (its parent); with one Domain per level par[L] = L.
// Domains of a level neither overlap nor touch (init_mesh.c:398-418): a child has ONE parent.
struct aa_mesh {
  int nl = 0;                      // number of Grids
  aa_grid *lev[AA_MAXLEV];
  int disp[AA_MAXLEV][3];
  int par[AA_MAXLEV];              // par[L]: parent grid of grid L+1
  int f2c[AA_MAXLEV];              // the links finest level first, deck order inside a level (smr.c:1224)
  Link link[AA_MAXLEV];            // link[L]: grid L+1 on grid par[L]
  Real *box[AA_MAXLEV];            // prolongation snapshot of the parent's zones around grid L+1
  hipStream_t st = nullptr; bool own_stream = true;
  // aa_mesh_step: the integrators of the levels read and write their own level only (main.c:572-585 calls them one after the other
  // and couples the levels afterwards), and the Grids of the reference's decks are too small to fill the GPU alone: level l > 0
  // integrates on side[l], forked from and joined to `st` by events (AA_MESH_OVERLAP=0: one after the other on `st`)
  hipStream_t side[AA_MAXLEV] = {nullptr}; hipEvent_t ev_fork = nullptr, ev_join[AA_MAXLEV] = {nullptr}; bool overlap = true;
  bool one_launch = true;          // the six sides of a flux correction / prolongation in one launch each
  bool two_d = false;              // aa_mesh_create_2d: every level is a 2-D Grid (Nx3 = 1): the k2d_* kernels, the 2-D integrators
  double tcoarse = 0;              // ionrad_3d.c:44
  double time = 0, dt = 0; int nstep = 0;   // MeshS
  CutMesh *cut = nullptr;          // the levels are composite handles cut at the same root planes (aa_create_cut): see the end of this file
  bool local = false;              // made by aa_mesh_create_local: one rank's stack of slabs
  // aa_mesh_run_2d (a Mesh of 2-D Grids): steps queued per read of the clock (AA_2D_BATCH when the Mesh was made; 0: it loops over
  // aa_mesh_step), the ONE clock of all levels in device memory, its page-locked mirror and that one's device address (made by the
  // first call that reaches the device), and the Grids as k2d_mesh_advance sees them
  int batch_2d = 0;
  Run2D *run2d_dev = nullptr; RunClock *clock = nullptr, *clock_dev = nullptr;
  MeshClockTab tab;
  // aa_mesh_run_3d (a Mesh of 3-D Grids): AA_3D_BATCH when the Mesh was made (0: it loops over aa_mesh_step), ONE device array with a
  // Run3D per Grid (hydro3d_launch.h MeshClockTab3 says why one each), and the Grids as k3d_mesh_advance sees them; `clock` and
  // `clock_dev` above are the mirror of either call (a Mesh is 2-D or 3-D)
  int batch_3d = 0;
  Run3D *run3d_dev = nullptr;
  MeshClockTab3 tab3;
  // aa_mesh_run_hst_arm: the ONE history schedule of the Mesh (api_internal.h HstRun; every Grid keeps its own partial rows, ring
  // and rows)
  HstRun hst;
};

extern "C" {

void aa_mesh_destroy(aa_mesh *m);
static int cut_create(int nlevels, aa_grid **levels, const int *disp, aa_mesh **out);
static void cut_destroy(aa_mesh *m);
static int cut_restrict_correct_pair(aa_mesh *m, int l);
static int cut_ionrad_restrict_correct(aa_mesh *m);
static int cut_prolongate(aa_mesh *m);
static int cut_new_dt(aa_mesh *m);
static int cut_ionflux_prolong(aa_mesh *m, int l);
static int cut_start(aa_mesh *m, bool with_dt);
static int cut_step(aa_mesh *m, int *niter);
// error paths of the create functions: the caller keeps its Grids as they were (mesh_alloc marked them as levels of a Mesh)
static void mesh_drop(aa_mesh *m)
{
  for (int l = 0; l < m->nl; l++) if (m->lev[l]) { m->lev[l]->keep_flux = false; m->lev[l]->keep = {0, {{0}}}; }
  delete m;
}
static int mesh_finish(aa_mesh *m, aa_grid **levels, aa_mesh **out, bool may_overlap = true)
{
  hipError_t e = hipSetDevice(levels[0]->p.device);
  if (e == hipSuccess) e = hipStreamCreate(&m->st);
  if (e != hipSuccess) { mesh_drop(m); return aa_fail(-2, "[aa_mesh_create]: %s", hipGetErrorString(e)); }
  for (int l = 0; l < m->nl; l++) aa_set_stream(m->lev[l], (void*)m->st);
  { const char *ev = getenv("AA_MESH_OVERLAP"); m->overlap = may_overlap && (ev ? atoi(ev) != 0 : true); }
  { const char *ev = getenv("AA_SMR_ONE_LAUNCH"); m->one_launch = ev ? atoi(ev) != 0 : true; }
  if (m->two_d) {      // AA_2D_BATCH as aa_create reads it for a Grid, with the Mesh's own default
    const char *ev = getenv("AA_2D_BATCH");
    m->batch_2d = ev ? atoi(ev) : AA_2D_MESH_BATCH_DEFAULT;
    if (m->batch_2d < 0 || m->batch_2d > 1024) { const int v = m->batch_2d; aa_mesh_destroy(m); return aa_fail(-1, "[aa_mesh_create_2d]: AA_2D_BATCH=%d: must be 0 (step by step) or 1..1024", v); }
  }
  if (!m->two_d) {     // AA_3D_BATCH likewise (a rank's stack of slabs and a cut Mesh never queue: aa_mesh_run_3d refuses them)
    const char *ev = getenv("AA_3D_BATCH");
    m->batch_3d = ev ? atoi(ev) : AA_3D_MESH_BATCH_DEFAULT;
    if (m->batch_3d < 0 || m->batch_3d > 1024) { const int v = m->batch_3d; aa_mesh_destroy(m); return aa_fail(-1, "[aa_mesh_create]: AA_3D_BATCH=%d: must be 0 (step by step) or 1..1024", v); }
  }
  if (m->overlap && m->nl > 1) {
    e = hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming);
    for (int l = 1; l < m->nl && e == hipSuccess; l++) {
      e = hipStreamCreateWithFlags(&m->side[l], hipStreamNonBlocking);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&m->ev_join[l], hipEventDisableTiming);
    }
    if (e != hipSuccess) { aa_mesh_destroy(m); return aa_fail(-2, "[aa_mesh_create]: %s", hipGetErrorString(e)); }
  }
  for (int l = 0; l + 1 < m->nl; l++) {
    const Link &L = m->link[l];
    const size_t nb = m->two_d ? (size_t)(L.n[0] + 6)*(L.n[1] + 6)*5 : (size_t)(L.n[0] + 6)*(L.n[1] + 6)*(L.n[2] + 6)*6;
    if (hipMalloc(&m->box[l], nb*sizeof(Real)) != hipSuccess) { aa_mesh_destroy(m); return aa_fail(-2, "[aa_mesh_create]: hipMalloc box"); }
    (void)hipMemset(m->box[l], 0, nb*sizeof(Real));
  }
  // a 2-D Grid's F holds first-pass fluxes of whatever it integrated before: RestrictCorrect of aa_mesh_start / _resume must read
  // zeros on the kept lines (main.c:401: the reference's myFlx are still empty there, q*(0 - 0))
  if (m->two_d)
    for (int l = 0; l < m->nl; l++) (void)hipMemsetAsync(m->lev[l]->d.F, 0, (size_t)10*m->lev[l]->d.nc*sizeof(Real), m->st);
  // the face planes whose second-pass fluxes k_flux_correct / k_flux_x3_export / k_flux_x3_apply read:
  // a level's own boundary faces and the outline of its child
  for (int l = 0; l < m->nl; l++) {
    aa_grid *g = m->lev[l];
    const int lo[3] = {g->d.is, g->d.js, g->d.ks}, hi[3] = {g->d.ie, g->d.je, g->d.ke};
    g->keep.n = 8;
    int nch = 0;
    for (int d = 0; d < 3; d++) { for (int q = 0; q < 8; q++) g->keep.p[d][q] = lo[d]; g->keep.p[d][1] = hi[d] + 1; }
    for (int L = 0; L + 1 < m->nl; L++) {
      if (m->par[L] != l) continue;
      if (nch == 3) { aa_mesh_destroy(m); return aa_fail(-1, "[aa_mesh_create]: more than three child Domains on one Grid"); }
      for (int d = 0; d < 3; d++) { g->keep.p[d][2 + 2*nch] = m->link[L].cs[d]; g->keep.p[d][3 + 2*nch] = m->link[L].ce[d] + 1; }
      nch++;
    }
  }
  { // the links finest level first, deck order inside a level
    int n = 0, maxlev = 0;
    for (int L = 0; L + 1 < m->nl; L++) if (m->lev[L + 1]->level > maxlev) maxlev = m->lev[L + 1]->level;
    for (int lev = maxlev; lev >= 1; lev--) for (int L = 0; L + 1 < m->nl; L++) if (m->lev[L + 1]->level == lev) m->f2c[n++] = L;
  }
  *out = m;
  return 0;
}

static aa_mesh *mesh_alloc(int nlevels, aa_grid **levels, bool two_d = false)
{
  if (!levels || nlevels < 1 || nlevels > AA_MAXLEV) { aa_fail(-1, "[aa_mesh_create]: bad arguments"); return nullptr; }
  aa_mesh *m = new aa_mesh();
  m->nl = nlevels; m->two_d = two_d;
  for (int l = 0; l < AA_MAXLEV; l++) { m->lev[l] = nullptr; m->box[l] = nullptr; }
  for (int l = 0; l < nlevels; l++) {
    aa_grid *g = levels[l];
    if (!g || (l == 0 ? g->level != 0 : (g->level < 1 || g->level < levels[l - 1]->level || g->level > levels[l - 1]->level + 1))) {
      mesh_drop(m); aa_fail(-1, "[aa_mesh_create]: grids must come level by level from the root (grid %d)", l); return nullptr; }
    if (!g->slab.empty()) { mesh_drop(m); aa_fail(-1, "[aa_mesh_create]: levels[%d] is cut into slabs: not available here (aa_mesh_create takes the levels of a Mesh cut at the root's planes, all made by aa_create_cut)", l); return nullptr; }
    if (g->p.device != levels[0]->p.device) { mesh_drop(m); aa_fail(-1, "[aa_mesh_create]: all levels must live on one device"); return nullptr; }
    if (g->one_d) { mesh_drop(m); aa_fail(-1, "[aa_mesh_create]: levels[%d] is a 1-D Grid: static mesh refinement is not available in 1-D", l); return nullptr; }
    if (two_d) {      // aa_mesh_create_2d: what the reference's 2-D SMR targets (CTU + H-correction, van Leer) pin
      if (!g->two_d) { mesh_drop(m); aa_fail(-1, "[aa_mesh_create_2d]: levels[%d] is a 3-D Grid: aa_mesh_create", l); return nullptr; }
      if (g->p.integrator != levels[0]->p.integrator) {
        mesh_drop(m); aa_fail(-1, "[aa_mesh_create_2d]: levels[%d] has integrator %d, the root %d: the levels of a Mesh share one integrator", l, g->p.integrator, levels[0]->p.integrator); return nullptr; }
      if (g->p.integrator == 2) {
        mesh_drop(m); aa_fail(-1, "[aa_mesh_create_2d]: levels[%d] has integrator = 2 (CTU without H-correction): no reference build with static mesh refinement pins it", l); return nullptr; }
      // third order (aa_set_order_2d): the reference's order is a build option, one for all Domains; blast_smr_ppm is CTU + H-correction
      if (g->order_2d != levels[0]->order_2d) {
        mesh_drop(m); aa_fail(-1, "[aa_mesh_create_2d]: levels[%d] is at order %d, the root at %d: the levels of a Mesh share one reconstruction order (aa_set_order_2d on every level)", l, g->order_2d, levels[0]->order_2d); return nullptr; }
      if (g->order_2d == 3 && g->p.integrator == 1) {
        mesh_drop(m); aa_fail(-1, "[aa_mesh_create_2d]: levels[%d] is a van Leer level at third order: no reference build with static mesh refinement pins it (CTU + H-correction only)", l); return nullptr; }
    } else
    if (g->two_d) { mesh_drop(m); aa_fail(-1, "[aa_mesh_create]: levels[%d] is a 2-D Grid: aa_mesh_create_2d (this is the 3-D constructor)", l); return nullptr; }
    if (g->fofc) { mesh_drop(m); aa_fail(-1, "[aa_mesh_create]: levels[%d] has first-order flux correction on (aa_set_fofc): not available on the Grids of a Mesh", l); return nullptr; }
    m->lev[l] = g; m->box[l] = nullptr; m->par[l] = l;
    g->keep_flux = true;
  }
  return m;
}

// ionrad_smr.c:97-98 mixes a parent-local index with the child's root-relative Disp: with a displaced
// parent (3+ levels) the reference writes out of bounds.  Refused by default; AA_SMR_DEEP_RADIATION=fixed
// uses the index the formula evidently means (child origin - 2 x parent origin), a documented
// departure from the reference for decks like its own 5-level one.
static bool deep_radiation_fixed() { const char *e = getenv("AA_SMR_DEEP_RADIATION"); return e && strcmp(e, "fixed") == 0; }

// init_grid.c (overlap tables) + SMR_init (smr.c:2931).  Takes over the levels' streams: all
// levels run on one stream so that inter-level kernels are ordered without events.
static int mesh_create_nested(int nlevels, aa_grid **levels, const int *disp, aa_mesh **out, const bool two_d)
{
  const int nd = two_d ? 2 : 3;      // directions with more than one zone
  if (!disp || !out) return aa_fail(-1, "[aa_mesh_create]: bad arguments");
  if (levels && nlevels >= 1 && nlevels <= AA_MAXLEV) {      // composite handles: a Mesh on in-library slabs, or a refusal by name
    int ncomp = 0;
    for (int l = 0; l < nlevels; l++) if (levels[l] && levels[l]->link) ncomp++;
    if (ncomp && two_d) return aa_fail(-1, "[aa_mesh_create_2d]: a Mesh of 2-D Grids cannot be cut into x3 slabs");
    if (ncomp && ncomp != nlevels) {
      int l = 0; while (levels[l] && (levels[l]->link != nullptr) == (levels[0]->link != nullptr)) l++;
      return aa_fail(-1, "[aa_mesh_create]: levels[%d] is %s but levels[0] is %s: the levels of a Mesh are all plain Grids, or all cut at the same root planes (aa_create_cut)",
                     l, levels[l]->link ? "cut into slabs" : "a plain Grid", levels[0]->link ? "cut into slabs" : "a plain Grid");
    }
    if (ncomp) return cut_create(nlevels, levels, disp, out);
  }
  aa_mesh *m = mesh_alloc(nlevels, levels, two_d);
  if (!m) return -1;
  for (int c = 1; c < nlevels; c++) {
    const aa_grid *C = m->lev[c];
    const int *dc = disp + 3*c;
    // the Domain of the level below that contains this one
    int pi = -1;
    for (int q = 0; q < c && pi < 0; q++) {
      const aa_grid *Q = m->lev[q];
      bool inside = (Q->level == C->level - 1);
      for (int d = 0; d < nd && inside; d++) {
        const int dq = Q->level ? disp[3*q + d] : 0;
        if (dc[d]/2 < dq || (dc[d] + C->p.Nx[d])/2 > dq + Q->p.Nx[d]) inside = false;
      }
      if (inside) pi = q;
    }
    if (pi < 0) { mesh_drop(m); return aa_fail(-1, "[aa_mesh_create]: grid %d (level %d) is not nested in a Domain of level %d", c, C->level, C->level - 1); }
    const int l = c - 1;
    m->par[l] = pi;
    const aa_grid *P = m->lev[pi];
    Link &L = m->link[l];
    const int lo[3] = {P->d.is, P->d.js, P->d.ks};
    const int irefine = 1 << C->level;
    const int dp[3] = {P->level ? disp[3*pi] : 0, P->level ? disp[3*pi + 1] : 0, P->level ? disp[3*pi + 2] : 0};
    if (two_d) {      // one plane: nothing along x3 (Link: n = 1, cs = ce = 0, no side)
      if (dc[2] != 0) { mesh_drop(m); return aa_fail(-1, "[aa_mesh_create_2d]: grid %d has kDisp = %d: a 2-D Domain (Nx3 = 1) has no x3 displacement", c, dc[2]); }
      L.cs[2] = L.ce[2] = 0; L.n[2] = 1; L.cdisp[2] = 0; L.prol[4] = L.prol[5] = L.corr[4] = L.corr[5] = 0;
    }
    for (int d = 0; d < nd; d++) {
      const int a = dc[d]/2 - dp[d], b = (dc[d] + C->p.Nx[d])/2 - dp[d];
      if ((dc[d] & 1) || (C->p.Nx[d] & 1) || a < 0 || b > P->p.Nx[d]) {
        mesh_drop(m); return aa_fail(-1, "[aa_mesh_create]: grid %d is not nested in grid %d along x%d", c, pi, d + 1);
      }
      L.cs[d] = a + lo[d]; L.ce[d] = b + lo[d] - 1; L.n[d] = b - a; L.cdisp[d] = dc[d];
      L.prol[2*d]     = L.corr[2*d]     = (dc[d] != 0);
      L.prol[2*d + 1] = L.corr[2*d + 1] = ((dc[d] + C->p.Nx[d])/irefine != C->p.rootNx[d]);
      // init_mesh.c:320-360: a child may touch its parent's edge only on the root boundary
      if ((a == 0 && L.prol[2*d]) || (b == P->p.Nx[d] && L.prol[2*d + 1])) {
        mesh_drop(m); return aa_fail(-1, "[init_mesh] child Domain (grid %d) touches its parent in x%d", c, d + 1);
      }
      // init_mesh.c:484-499: nor closer than nghost/2 parent zones to its edge (the prolongation stencil)
      if (two_d && ((L.prol[2*d] && 2*a < NG) || (L.prol[2*d + 1] && 2*(P->p.Nx[d] - b) < NG))) {
        mesh_drop(m); return aa_fail(-1, "[init_mesh] child Domain (grid %d) closer than nghost/2 to its parent in x%d", c, d + 1);
      }
    }
    // init_mesh.c:398-418: Domains on the same level neither overlap nor touch
    for (int q = 1; q < c; q++) {
      const aa_grid *Q = m->lev[q];
      if (Q->level != C->level) continue;
      bool sep = false;
      for (int d = 0; d < nd; d++) if (dc[d] > disp[3*q + d] + Q->p.Nx[d] || disp[3*q + d] > dc[d] + C->p.Nx[d]) sep = true;
      if (!sep) { mesh_drop(m); return aa_fail(-1, "[init_mesh]: Domains at the same level overlap or touch (grids %d and %d)", q, c); }
    }
    if (P->p.ion && (dp[1] || dp[2])) {      // (see deep_radiation_fixed)
      if (!deep_radiation_fixed()) {
        mesh_drop(m); return aa_fail(-1, "[aa_mesh_create]: radiation across a displaced parent (grid %d) is undefined in the reference "
                                     "(set AA_SMR_DEEP_RADIATION=fixed for the corrected hand-off)", pi);
      }
      for (int d = 0; d < 3; d++) L.cdisp[d] = dc[d] - 2*dp[d];
    }
  }
  return mesh_finish(m, levels, out);
}
int aa_mesh_create(int nlevels, aa_grid **levels, const int *disp, aa_mesh **out)
{ return mesh_create_nested(nlevels, levels, disp, out, false); }
// the same contract for Grids that are all 2-D (Nx3 = 1): disp[3*l + 2] must be 0, the nesting rules hold in x1 and x2
int aa_mesh_create_2d(int nlevels, aa_grid **levels, const int *disp, aa_mesh **out)
{ return mesh_create_nested(nlevels, levels, disp, out, true); }

// One rank's stack of x3 slabs of a Mesh whose levels are all cut at the same planes (multi-GPU
// SMR).  links[21*l..]: cs[3] (local parent index incl. ghosts), n[3], prol[6], corr[6], cdisp[3]
// of level l+1 on level l.  A child slab may reach the edge of its parent slab; where the level
// itself ends at that edge (prol=1, corr=0) the parent plane outside is corrected on the
// neighbouring slab with aa_flux_x3_export / aa_flux_x3_apply.
static int mesh_create_local(int nlevels, aa_grid **levels, const int *links, aa_mesh **out, bool may_overlap);
int aa_mesh_create_local(int nlevels, aa_grid **levels, const int *links, aa_mesh **out)
{
  for (int l = 0; levels && l < nlevels && l < AA_MAXLEV; l++)
    if (levels[l] && levels[l]->link) return aa_fail(-1, "[aa_mesh_create_local]: levels[%d] is cut into slabs: a rank's stack holds plain Grids (one process on several GPUs: aa_create_cut + aa_mesh_create)", l);
  return mesh_create_local(nlevels, levels, links, out, true);
}
static int mesh_create_local(int nlevels, aa_grid **levels, const int *links, aa_mesh **out, bool may_overlap)
{
  if ((nlevels > 1 && !links) || !out) return aa_fail(-1, "[aa_mesh_create_local]: bad arguments");
  aa_mesh *m = mesh_alloc(nlevels, levels);
  if (!m) return -1;
  m->local = true;
  // links join grid l+1 to grid l here (par[l] = l): ONE Domain per level, a strict chain (mesh_alloc alone would also take siblings)
  for (int l = 0; l < nlevels; l++)
    if (m->lev[l]->level != l) { mesh_drop(m); return aa_fail(-1, "[aa_mesh_create_local]: grid %d is on level %d: a rank's stack holds one Domain per level", l, levels[l]->level); }
  for (int l = 0; l + 1 < nlevels; l++) {
    const int *q = links + 21*l;
    const aa_grid *P = m->lev[l], *C = m->lev[l + 1];
    Link &L = m->link[l];
    for (int d = 0; d < 3; d++) {
      L.cs[d] = q[d]; L.n[d] = q[3 + d]; L.ce[d] = q[d] + q[3 + d] - 1; L.cdisp[d] = q[18 + d];
      if (L.n[d]*2 != C->p.Nx[d] || L.cs[d] < AA_NGHOST || L.ce[d] >= AA_NGHOST + P->p.Nx[d]) {
        mesh_drop(m); return aa_fail(-1, "[aa_mesh_create_local]: link %d does not match the slabs along x%d", l, d + 1);
      }
    }
    for (int d = 0; d < 6; d++) { L.prol[d] = q[6 + d]; L.corr[d] = q[12 + d]; }
  }
  return mesh_finish(m, levels, out, may_overlap);
}

void aa_mesh_destroy(aa_mesh *m)      // the levels stay alive and go back to the default stream
{
  if (!m) return;
  if (m->cut) { cut_destroy(m); return; }
  hipStreamSynchronize(m->st);
  for (int l = 0; l < m->nl; l++) {
    m->lev[l]->st = nullptr; m->lev[l]->own_stream = false; if (m->box[l]) hipFree(m->box[l]);
    m->lev[l]->keep_flux = false; m->lev[l]->keep = {0, {{0}}};      // no longer a level of a Mesh
  }
  for (int l = 1; l < m->nl; l++) { if (m->side[l]) hipStreamDestroy(m->side[l]); if (m->ev_join[l]) hipEventDestroy(m->ev_join[l]); }
  if (m->ev_fork) hipEventDestroy(m->ev_fork);
  if (m->own_stream) hipStreamDestroy(m->st);
  if (m->run2d_dev) hipFree(m->run2d_dev);
  if (m->run3d_dev) hipFree(m->run3d_dev);
  if (m->clock) hipHostFree(m->clock);
  hst_free_sched(m->hst);
  delete m;
}

int aa_mesh_set_stream(aa_mesh *m, void *hip_stream)   // run every level on a caller-owned stream
{
  if (m->cut) return aa_fail(-1, "[aa_mesh_set_stream]: a Mesh cut into slabs runs on its slabs' own streams");
  hipStreamSynchronize(m->st);
  if (m->own_stream) { hipStreamDestroy(m->st); m->own_stream = false; }
  m->st = (hipStream_t)hip_stream;
  for (int l = 0; l < m->nl; l++) { m->lev[l]->st = m->st; m->lev[l]->own_stream = false; }
  return 0;
}

int aa_mesh_get_state(const aa_mesh *m, double *time, double *dt, int *nstep)
{ if (time) *time = m->time; if (dt) *dt = m->dt; if (nstep) *nstep = m->nstep; return 0; }
int aa_mesh_set_state(aa_mesh *m, double time, double dt, int nstep)
{ m->time = time; m->dt = dt; m->nstep = nstep; return 0; }

// smr.c:1207.  Before the first step (main.c:401) the reference's myFlx arrays are all zero and the
// flux correction adds q*(0-0); here the flux arrays are zero-initialised, to the same effect.
int aa_mesh_restrict_correct_pair(aa_mesh *m, int l)      // level l+1 -> level l
{
  if (m->cut) return cut_restrict_correct_pair(m, l);
  if (l >= 0 && l + 1 < m->nl) m->lev[m->par[l]]->active_dirty = true;
  if (l < 0 || l + 1 >= m->nl) return aa_fail(-1, "[aa_mesh_restrict_correct_pair]: pair %d", l);
  aa_grid *P = m->lev[m->par[l]], *C = m->lev[l + 1];       // link l: grid l+1 on its parent
  const Link &L = m->link[l];
  const int nvar = 5 + P->p.nscal;
  Scope s(P, "smr_restrict_correct");
  if (m->two_d) {
    hipLaunchKernelGGL(k2d_restrict, dim3(nblk(L.n[0], S2_W), nblk(L.n[1], S2_R)), dim3(S2_W, S2_R), 0, m->st, C->d, P->d, L);
    const int nmax = L.n[0] > L.n[1] ? L.n[0] : L.n[1];
    const bool any = L.corr[0] || L.corr[1] || L.corr[2] || L.corr[3];
    if (m->one_launch) {      // the four sides in ONE launch (AA_SMR_ONE_LAUNCH=0: one per side)
      if (any) hipLaunchKernelGGL(k2d_flux_correct, dim3(nblk(nmax, S2_W), 4), dim3(S2_W), 0, m->st, C->d, P->d, L, -1, (Real)P->dt);
    } else
    for (int dim = 0; dim < 4; dim++)
      if (L.corr[dim]) hipLaunchKernelGGL(k2d_flux_correct, dim3(nblk(L.n[1 - (dim >> 1)], S2_W)), dim3(S2_W), 0, m->st, C->d, P->d, L, dim, (Real)P->dt);
    HIPCHK(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(k_restrict, dim3(nblk((long)L.n[0]*L.n[1]*L.n[2], 256)), dim3(256), 0, m->st,
                     C->d, P->d, L, (1u << nvar) - 1u);
  if (m->one_launch) {      // the six sides in ONE launch (AA_SMR_ONE_LAUNCH=0: one per side)
    long nmax = 0; bool any = false;
    for (int dim = 0; dim < 6; dim++) {
      const int d = dim >> 1, d1 = (d == 0) ? 1 : 0, d2 = (d == 2) ? 1 : 2;
      if (L.corr[dim]) { any = true; const long n = (long)L.n[d1]*L.n[d2]; if (n > nmax) nmax = n; }
    }
    if (any) hipLaunchKernelGGL(k_flux_correct, dim3(nblk(nmax, 256), 6), dim3(256), 0, m->st, C->d, P->d, L, -1, nvar, (Real)P->dt);
  } else
  for (int dim = 0; dim < 6; dim++) {
    if (!L.corr[dim]) continue;
    const int d = dim >> 1, d1 = (d == 0) ? 1 : 0, d2 = (d == 2) ? 1 : 2;
    hipLaunchKernelGGL(k_flux_correct, dim3(nblk((long)L.n[d1]*L.n[d2], 256)), dim3(256), 0, m->st,
                       C->d, P->d, L, dim, nvar, (Real)P->dt);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int aa_mesh_restrict_correct(aa_mesh *m)
{
  // finest pair first: a level is restricted for its parent after it received its own child's
  // solution and flux correction (the order of the loop over levels at smr.c:1224)
  for (int l = 0; l + 1 < m->nl; l++) { int rc = aa_mesh_restrict_correct_pair(m, m->f2c[l]); if (rc) return rc; }
  return 0;
}

// smr.c:85: E and s[0] only, after the radiation step
int aa_mesh_ionrad_restrict_correct(aa_mesh *m)
{
  if (m->two_d) return aa_fail(-1, "[aa_mesh_ionrad_restrict_correct]: a Mesh of 2-D Grids has no ion radiation (the reference has ionrad_3d only)");
  if (m->cut) return cut_ionrad_restrict_correct(m);
  for (int l = 0; l < m->nl; l++) m->lev[l]->active_dirty = true;
  for (int q = 0; q + 1 < m->nl; q++) {
    const int l = m->f2c[q];
    aa_grid *P = m->lev[m->par[l]], *C = m->lev[l + 1];
    const Link &L = m->link[l];
    Scope s(P, "smr_ion_restrict");
    hipLaunchKernelGGL(k_restrict, dim3(nblk((long)L.n[0]*L.n[1]*L.n[2], 256)), dim3(256), 0, m->st,
                       C->d, P->d, L, (1u << 4) | (1u << 5));
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// smr.c:2359
int aa_mesh_prolongate(aa_mesh *m)
{
  if (m->cut) return cut_prolongate(m);
  for (int l = 0; l < m->nl; l++) {
    for (int c = 0; c + 1 < m->nl; c++) {      // Step 1: hand the zones around every child over
      if (m->par[c] != l) continue;
      const Link &L = m->link[c];
      if (m->two_d) {
        hipLaunchKernelGGL(k2d_box_copy, dim3(nblk(L.n[0] + 6, S2_W), nblk(L.n[1] + 6, S2_R)), dim3(S2_W, S2_R), 0, m->st, m->lev[l]->d, L, m->box[c]);
        continue;
      }
      const long nb = (long)(L.n[0] + 6)*(L.n[1] + 6)*(L.n[2] + 6);
      hipLaunchKernelGGL(k_box_copy, dim3(nblk(nb, 256)), dim3(256), 0, m->st, m->lev[l]->d, L, m->box[c]);
    }
    if (l > 0) {                               // Steps 2-3: own ghost zones from the parent's zones
      aa_grid *C = m->lev[l];
      const Link &L = m->link[l - 1];
      const int nvar = 5 + C->p.nscal;
      Scope s(C, "smr_prolongate");
      if (m->two_d) {      // the sides dim < 2*nDim (smr.c:2560); a side's region spans the other direction's ghost zones too
        const int c0 = (C->p.Nx[0] + 2*NG)/2, c1 = (C->p.Nx[1] + 2*NG)/2;
        const bool any = L.prol[0] || L.prol[1] || L.prol[2] || L.prol[3];
        if (m->one_launch) {
          if (any) hipLaunchKernelGGL(k2d_prolong, dim3(nblk(c0, S2_W), nblk(c1, S2_R), 4), dim3(S2_W, S2_R), 0, m->st, C->d, L, m->box[l - 1], -1);
        } else
        for (int dim = 0; dim < 4; dim++) {
          if (!L.prol[dim]) continue;
          const int n0 = (dim >> 1) == 0 ? NG/2 : c0, n1 = (dim >> 1) == 1 ? NG/2 : c1;
          hipLaunchKernelGGL(k2d_prolong, dim3(nblk(n0, S2_W), nblk(n1, S2_R)), dim3(S2_W, S2_R), 0, m->st, C->d, L, m->box[l - 1], dim);
        }
      } else
      if (m->one_launch) {
        long nmax = 0;
        for (int dim = 0; dim < 6; dim++) {
          if (!L.prol[dim]) continue;
          long cnt = 1;
          for (int d = 0; d < 3; d++) cnt *= (d == (dim >> 1)) ? NG/2 : (C->p.Nx[d] + 2*NG)/2;
          if (cnt > nmax) nmax = cnt;
        }
        if (nmax > 0) hipLaunchKernelGGL(k_prolong, dim3(nblk(nmax, 128), 6), dim3(128), 0, m->st, C->d, L, m->box[l - 1], -1, nvar);
      } else
      for (int dim = 0; dim < 6; dim++) {
        if (!L.prol[dim]) continue;
        long cnt = 1;
        for (int d = 0; d < 3; d++) cnt *= (d == (dim >> 1)) ? NG/2 : (C->p.Nx[d] + 2*NG)/2;
        hipLaunchKernelGGL(k_prolong, dim3(nblk(cnt, 128)), dim3(128), 0, m->st, C->d, L, m->box[l - 1], dim, nvar);
      }
    }
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// new_dt.c:167-185 of the Mesh, from the max_dti folded over its levels (time_step.h)
static void mesh_pick_dt(aa_mesh *m, double max_dti)
{
  const aa_params &p = m->lev[0]->p;
  m->dt = dt_pick(m->nstep, m->dt, dt_courant(p.cour_no, max_dti), m->time, p.tlim);
}
// new_dt.c:32 over all levels: max_v is carried from Grid to Grid (:33), one dt for the Mesh
int aa_mesh_new_dt(aa_mesh *m)
{
  if (m->cut) return cut_new_dt(m);
  double cum[3] = {0.0, 0.0, 0.0}, max_dti = 0.0;
  const int ndir = m->two_d ? 2 : 3;      // new_dt.c:126-161: max_v3 only where Nx3 > 1
  for (int l = 0; l < m->nl; l++) {
    aa_grid *g = m->lev[l];
    { Scope s(g, "new_dt");
      HIPCHK(hipMemsetAsync(g->sc->max_v, 0, 3*sizeof(unsigned long long), g->st));
      launch_cfl(g->d, g->sc, g->st); }
    int rc = aa_fetch_scalars(g); if (rc) return rc;
    double v[3]; max_v_of(*g->sc_host, v);
    max_dti = dt_fold_level(max_dti, cum, v, g->d.dx, ndir);
  }
  mesh_pick_dt(m, max_dti);
  for (int l = 0; l < m->nl; l++) m->lev[l]->dt = m->dt;
  return 0;
}

// ionrad_smr.c:345 + :34: the flux level l-1 left at the upstream face of level l, onto level l's rays
int aa_mesh_ionflux_prolong(aa_mesh *m, int l)
{
  if (m->two_d) return aa_fail(-1, "[aa_mesh_ionflux_prolong]: a Mesh of 2-D Grids has no ion radiation (the reference has ionrad_3d only)");
  if (l < 1 || l >= m->nl) return aa_fail(-1, "[aa_mesh_ionflux_prolong]: level %d", l);
  if (m->cut) return cut_ionflux_prolong(m, l);
  const Link &L = m->link[l - 1];
  aa_grid *P = m->lev[m->par[l - 1]];
  { int rc = aa_edgeflux_ready(P); if (rc) return rc; }       // the parent's EdgeFlux of its last sweep
  if (L.prol[0])
    hipLaunchKernelGGL(k_ionflux_prolong, dim3(nblk((long)(L.n[1] + 1)*(L.n[2] + 1), 256)), dim3(256), 0, m->st,
                       m->lev[l]->d, P->d, L);
  HIPCHK(hipGetLastError());
  return 0;
}

// multi-GPU SMR: the child's restricted boundary flux (DEVICE buffer of (Nx1/2)(Nx2/2)*6 doubles) ...
int aa_flux_x3_export(aa_grid *child, int side, double *dev_buf)
{
  if (!child->slab.empty()) return aa_fail(-1, "[aa_flux_x3_export]: not available on a Grid cut into slabs");
  const long n = (long)(child->p.Nx[0]/2)*(child->p.Nx[1]/2);
  hipLaunchKernelGGL(k_flux_x3_export, dim3(nblk(n, 256)), dim3(256), 0, child->st, child->d, side, dev_buf);
  HIPCHK(hipGetLastError());
  return 0;
}
// ... and its application to the plane of the parent slab across the cut (Grid dt as in RestrictCorrect)
int aa_flux_x3_apply(aa_grid *parent, int side, int i0, int j0, int n1, int n2, const double *dev_buf)
{
  parent->active_dirty = true;
  if (!parent->slab.empty()) return aa_fail(-1, "[aa_flux_x3_apply]: not available on a Grid cut into slabs");
  if (i0 < AA_NGHOST || j0 < AA_NGHOST || i0 + n1 > AA_NGHOST + parent->p.Nx[0] || j0 + n2 > AA_NGHOST + parent->p.Nx[1])
    return aa_fail(-1, "[aa_flux_x3_apply]: region outside the Grid");
  hipLaunchKernelGGL(k_flux_x3_apply, dim3(nblk((long)n1*n2, 256)), dim3(256), 0, parent->st, parent->d, side, i0, j0, n1, n2,
                     5 + parent->p.nscal, (Real)parent->dt, dev_buf);
  HIPCHK(hipGetLastError());
  return 0;
}

// ionrad_3d.c:862 with STATIC_MESH_REFINEMENT: the root sub-cycles to its own stopping criteria and
// publishes the time it covered; a refined level sub-cycles until it has covered exactly that
int aa_mesh_ion_radtransfer(aa_mesh *m, int l, int *niter_out)
{
  if (m->two_d) return aa_fail(-1, "[aa_mesh_ion_radtransfer]: a Mesh of 2-D Grids has no ion radiation (the reference has ionrad_3d only)");
  aa_grid *g = m->lev[l];
  const bool finegrid = (g->level != 0);
  double dt_done = 0.0;
  int niter = 0, rc;
  if (finegrid) { if ((rc = aa_mesh_ionflux_prolong(m, l))) return rc; }
  else m->tcoarse = 0;
  if ((rc = aa_ion_run(g, finegrid ? 1 : 0, finegrid ? m->tcoarse : g->dt, &niter, &dt_done))) return rc;
  if (!finegrid && (rc = ion_root_close(g, niter, dt_done, &m->tcoarse))) return rc;
  m->dt = g->dt;                             // :1030 pMesh->dt = pGrid->dt
  if (niter_out) *niter_out = niter;
  return 0;
}

// main.c:395-447 after problem() has filled every level
int aa_mesh_start(aa_mesh *m)
{
  int rc;
  if (m->cut) return cut_start(m, true);
  if ((rc = aa_mesh_restrict_correct(m))) return rc;
  for (int l = 0; l < m->nl; l++) {
    if ((rc = aa_bvals_mhd(m->lev[l]))) return rc;
    if ((rc = aa_bvals_ionrad(m->lev[l]))) return rc;
  }
  if ((rc = aa_mesh_prolongate(m))) return rc;
  return aa_mesh_new_dt(m);
}

// main.c:398-451 of a restarted run: aa_mesh_start without new_dt -- the file's dt is the next step's
int aa_mesh_resume(aa_mesh *m)
{
  int rc;
  if (m->cut) return cut_start(m, false);
  if ((rc = aa_mesh_restrict_correct(m))) return rc;
  for (int l = 0; l < m->nl; l++) {
    if ((rc = aa_bvals_mhd(m->lev[l]))) return rc;
    if ((rc = aa_bvals_ionrad(m->lev[l]))) return rc;
  }
  return aa_mesh_prolongate(m);
}

// one pass of main.c:519-669 with STATIC_MESH_REFINEMENT; niter[l] = radiation sub-cycles of level l
int aa_mesh_step(aa_mesh *m, int *niter)
{
  int rc;
  if (m->cut) return cut_step(m, niter);
  aa_grid *root = m->lev[0];
  if (root->p.ion && root->nradplane > 0) {                          // :546-562
    for (int l = 0; l < m->nl; l++) {
      int n = 0;
      m->lev[l]->time = m->time;
      if ((rc = aa_mesh_ion_radtransfer(m, l, &n))) return rc;
      if (niter) niter[l] = n;
      if ((rc = aa_bvals_mhd(m->lev[l]))) return rc;
    }
    if ((rc = aa_mesh_ionrad_restrict_correct(m))) return rc;
  } else if (niter) for (int l = 0; l < m->nl; l++) niter[l] = 0;
  const bool fork = m->overlap && m->nl > 1 && m->side[1];
  if (fork) {
    HIPCHK(hipEventRecord(m->ev_fork, m->st));
    for (int l = 1; l < m->nl; l++) HIPCHK(hipStreamWaitEvent(m->side[l], m->ev_fork, 0));
  }
  rc = 0;
  for (int l = 0; l < m->nl && !rc; l++) {                            // :572-585
    aa_grid *g = m->lev[l];
    if (fork && l > 0) g->st = m->side[l];
    if (m->two_d) rc = (g->p.integrator == 1 ? aa_integrate_2d_vl(g) : aa_integrate_2d_ctu(g));      // integrate.c:49-58
    else rc = (g->p.integrator == 1 ? aa_integrate_3d_vl(g) : aa_integrate_3d_ctu(g));
    g->st = m->st;
  }
  if (fork)
    for (int l = 1; l < m->nl; l++) { HIPCHK(hipEventRecord(m->ev_join[l], m->side[l])); HIPCHK(hipStreamWaitEvent(m->st, m->ev_join[l], 0)); }
  if (rc) return rc;
  if ((rc = aa_mesh_restrict_correct(m))) return rc;                  // :591
  for (int l = 0; l < m->nl; l++)                                     // :597 Userwork_in_loop
    if (m->lev[l]->npin > 0 && (rc = aa_apply_pinned_cells(m->lev[l]))) return rc;
  m->nstep++; m->time += m->dt;                                       // :618-626
  for (int l = 0; l < m->nl; l++) { m->lev[l]->time = m->time; m->lev[l]->nstep = m->nstep; }
  if ((rc = aa_mesh_new_dt(m))) return rc;                            // :629
  for (int l = 0; l < m->nl; l++) if ((rc = aa_bvals_mhd(m->lev[l]))) return rc;   // :635-644
  return aa_mesh_prolongate(m);                                       // :647
}

// ---- aa_mesh_run_2d: whole passes of aa_mesh_step's loop for a Mesh of 2-D Grids with ONE clock in device memory ----------------
// (the frame -- refusals of span and tlim, the loop over single steps, seed / queue / read the clock -- is run.hip's run_frame)
static int mesh_run_buffers(aa_mesh *m)
{
  if (m->clock) return 0;
  RunClock *h = nullptr, *hd = nullptr; Run2D *d = nullptr;
  if (hipHostMalloc(&h, sizeof(RunClock), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&hd, h, 0) != hipSuccess || hipMalloc(&d, sizeof(Run2D)) != hipSuccess) {
    if (h) hipHostFree(h);
    (void)hipGetLastError();
    return aa_fail(-2, "[aa_mesh_run_2d]: clock buffers");
  }
  memset(h, 0, sizeof(RunClock));
  m->clock = h; m->clock_dev = hd; m->run2d_dev = d;
  m->tab.n = m->nl; m->tab.pad = 0;
  for (int l = 0; l < AA_2D_MESH_GRIDS; l++) {
    const bool in = l < m->nl;
    m->tab.sc[l] = in ? m->lev[l]->sc : nullptr;
    m->tab.dx[2*l] = in ? m->lev[l]->d.dx[0] : 0.0; m->tab.dx[2*l + 1] = in ? m->lev[l]->d.dx[1] : 0.0;
  }
  return 0;
}

// The history rows of a queued step, where the call has a schedule armed: behind the step's boundary pass and prolongation (both
// write ghost zones only; the sums are over active zones) and in front of the next step's first kernel.  k_history_dc for every
// Grid in the Mesh's order, each into its own partial rows; then k_hst_row for the Grids in turn, each into its own ring at the
// schedule's row count -- all of them evaluate the rule on the Mesh's clock (a 3-D Mesh: the first Grid's, they are kept equal) and
// on the schedule as the step before left it; only the last launch moves the schedule on.
static void mesh_queue_hst(aa_mesh *m, const RunClock *clock, double tlim)
{
  Scope s(m->lev[0], "hst_row");
  int nb[AA_MAXLEV];
  for (int l = 0; l < m->nl; l++) nb[l] = launch_history_dc(m->lev[l]->d, m->lev[l]->p.nscal, m->lev[l]->hst_part, clock, tlim, m->hst.sched, m->st);
  for (int l = 0; l < m->nl; l++) launch_hst_row(m->lev[l], nb[l], clock, tlim, m->hst, l == m->nl - 1, m->st);
}

// One queued step: aa_mesh_step's order with no host in it.  Every kernel in front of k2d_mesh_advance reads dt and `live` from
// the Mesh's clock and stores nothing behind the stop.
//  * the integrator chain of every level, the update kernel in its flux-keeping form.  new_dt's maxima ride on it where the Grid
//    has no child: nothing writes such a Grid between its update and new_dt (pinned zones are refused).  A Grid WITH children is
//    rewritten by restriction and flux correction: its update kernel leaves no maxima, and k_cfl sweeps it behind the last
//    restrict_correct pair.  k_cfl only raises the Grid's own maxima (atomic MAX); behind a stop that is all it does, and the next
//    call's seed zeroes them again (aa_mesh_new_dt zeroes them itself).  MAX over the same doubles is order-free: dt is the same bits.
//  * restriction and flux correction, finest pair first, both behind the `live` guard (the correction ADDS to the parent).
//  * k2d_mesh_advance: nstep++, time += dt, new_dt over the Grids, the stop rule; `stepped` = this step was taken.
//  * bvals_mhd of every level, then the snapshots around every child (k2d_box_copy_dc) and the prolongation.  What they write
//    behind a stop, with U's active zones untouched:
//      - k_bc takes no dt and is not predicated.  Every level has four or more zones per direction (else: step by step, below), so
//        a ghost zone it writes is a copy of an ACTIVE zone (x1 pass) or of a row whose x1 ghost zones are either written by that
//        pass just before or lie on a fine/coarse side -- and then the zone copied to is a corner the prolongation of that side
//        overwrites again (its region spans the other direction's ghost zones).  So where k_bc is the last writer of a ghost zone
//        it writes again what is there.
//      - k2d_prolong is a function of the snapshot `box` alone, so it writes again what is there as long as the snapshot is the
//        one of the last step taken.  The snapshot itself is NOT a function of an unchanged state: it is taken before the parent's
//        own ghost zones are prolonged (smr.c Prolongate, Step 1), and a child two zones from its parent's fine/coarse side has
//        one of those ghost zones in its snapshot -- the value of the step before while the step is taken, the fresh one if the
//        snapshot were retaken behind the stop.  So k2d_box_copy_dc is predicated on `stepped` and the boxes stay as they are.
//    A following aa_mesh_step, an output or a restart dump therefore sees the state the last step taken left.
// Everything is a plain launch on the Mesh's ONE stream, in stream order; no kernel waits on memory or on another workgroup.  The
// fork of the levels onto their side streams (aa_mesh_step, AA_MESH_OVERLAP) is dropped here: with no host visit between the steps
// its two event hand-overs per level and step cost more than the overlap of these small chains gains (203 us per
// step of the reference's deck on one stream against 225 - 232 with the fork).
static int mesh_queue_step_2d(aa_mesh *m, double tlim)
{
  const Run2D *rc = m->run2d_dev;
  for (int l = 0; l < m->nl; l++) {
    bool parent = false;
    for (int c = 0; c + 1 < m->nl; c++) if (m->par[c] == l) parent = true;
    queue_chain_2d(m->lev[l], rc, parent ? nullptr : m->lev[l]->sc);      // (run.hip: the chain aa_run_2d queues, flux-keeping here; on m->st)
  }
  for (int q = 0; q + 1 < m->nl; q++) {                              // RestrictCorrect, finest pair first
    const int l = m->f2c[q];
    aa_grid *P = m->lev[m->par[l]], *C = m->lev[l + 1];
    const Link &L = m->link[l];
    Scope s(P, "smr_restrict_correct");
    hipLaunchKernelGGL(k2d_restrict_dc, dim3(nblk(L.n[0], S2_W), nblk(L.n[1], S2_R)), dim3(S2_W, S2_R), 0, m->st, C->d, P->d, L, rc);
    const int nmax = L.n[0] > L.n[1] ? L.n[0] : L.n[1];
    if (m->one_launch) {
      if (L.corr[0] || L.corr[1] || L.corr[2] || L.corr[3])
        hipLaunchKernelGGL(k2d_flux_correct_dc, dim3(nblk(nmax, S2_W), 4), dim3(S2_W), 0, m->st, C->d, P->d, L, -1, rc);
    } else
    for (int dim = 0; dim < 4; dim++)
      if (L.corr[dim]) hipLaunchKernelGGL(k2d_flux_correct_dc, dim3(nblk(L.n[1 - (dim >> 1)], S2_W)), dim3(S2_W), 0, m->st, C->d, P->d, L, dim, rc);
  }
  for (int l = 0; l < m->nl; l++) {                                  // new_dt's maxima of the Grids with children
    bool parent = false;
    for (int c = 0; c + 1 < m->nl; c++) if (m->par[c] == l) parent = true;
    if (parent) { Scope s(m->lev[l], "new_dt"); launch_cfl(m->lev[l]->d, m->lev[l]->sc, m->st); }
  }
  { Scope s(m->lev[0], "smr_advance"); launch_2d_mesh_advance(m->run2d_dev, m->tab, m->clock_dev, m->st); }
  for (int l = 0; l < m->nl; l++) {
    aa_grid *g = m->lev[l];
    Scope s(g, "bvals_mhd");
    for (int a = 0; a < 2; a++) launch_bc_dir(g->d, g->p.nscal, a, g->p.bc[2*a], g->p.bc[2*a + 1], m->st);
  }
  for (int l = 0; l < m->nl; l++) {                                  // Prolongate, in the order of aa_mesh_prolongate
    for (int c = 0; c + 1 < m->nl; c++) {
      if (m->par[c] != l) continue;
      const Link &L = m->link[c];
      hipLaunchKernelGGL(k2d_box_copy_dc, dim3(nblk(L.n[0] + 6, S2_W), nblk(L.n[1] + 6, S2_R)), dim3(S2_W, S2_R), 0, m->st, m->lev[l]->d, L, m->box[c], rc);
    }
    if (l == 0) continue;
    aa_grid *C = m->lev[l];
    const Link &L = m->link[l - 1];
    Scope s(C, "smr_prolongate");
    const int c0 = (C->p.Nx[0] + 2*NG)/2, c1 = (C->p.Nx[1] + 2*NG)/2;
    if (m->one_launch) {
      if (L.prol[0] || L.prol[1] || L.prol[2] || L.prol[3])
        hipLaunchKernelGGL(k2d_prolong, dim3(nblk(c0, S2_W), nblk(c1, S2_R), 4), dim3(S2_W, S2_R), 0, m->st, C->d, L, m->box[l - 1], -1);
    } else
    for (int dim = 0; dim < 4; dim++) {
      if (!L.prol[dim]) continue;
      const int n0 = (dim >> 1) == 0 ? NG/2 : c0, n1 = (dim >> 1) == 1 ? NG/2 : c1;
      hipLaunchKernelGGL(k2d_prolong, dim3(nblk(n0, S2_W), nblk(n1, S2_R)), dim3(S2_W, S2_R), 0, m->st, C->d, L, m->box[l - 1], dim);
    }
  }
  if (m->hst.active) mesh_queue_hst(m, &m->run2d_dev->c, tlim);      // (with no schedule armed the step launches what it always did)
  return 0;
}

static int mesh_run_step(void *self) { return aa_mesh_step((aa_mesh*)self, nullptr); }
static int mesh_run_begin(void *self, const RunClock &seed, double t_stop, double tlim, int nstep_stop, RunClock **clock)
{
  aa_mesh *m = (aa_mesh*)self;
  if (int rc = mesh_run_buffers(m)) return rc;
  for (int l = 0; l < m->nl; l++) { m->lev[l]->cfl_ready = false; m->lev[l]->active_dirty = true; }
  const Run2D v = {seed, t_stop, tlim, m->lev[0]->p.cour_no, nstep_stop, 0};
  launch_2d_mesh_seed(m->run2d_dev, v, m->tab, m->st);
  *clock = m->clock;
  return 0;
}
static int mesh_run_batch(void *self, double, double tlim, int)
{
  aa_mesh *m = (aa_mesh*)self;
  for (int k = 0; k < m->batch_2d; k++) { int rc = mesh_queue_step_2d(m, tlim); if (rc) return rc; }
  return 0;
}
// every level's copy of MeshS, as aa_mesh_step and aa_mesh_new_dt leave them
static void mesh_run_end(void *self)
{
  aa_mesh *m = (aa_mesh*)self;
  for (int l = 0; l < m->nl; l++) { m->lev[l]->time = m->time; m->lev[l]->nstep = m->nstep; m->lev[l]->dt = m->dt; }
}

// the Mesh's history schedule behind run_frame (api_internal.h RunOps): a row of every Grid from aa_history behind a single step;
// the seed of the device's schedule; every Grid's rows of a batch from its ring
static int mesh_hst_row(void *self)
{
  aa_mesh *m = (aa_mesh*)self;
  for (int l = 0; l < m->nl; l++) if (int rc = hst_row_host(m->lev[l], m->time, m->dt)) return rc;
  return 0;
}
static int mesh_hst_begin(void *self, int nstep) { aa_mesh *m = (aa_mesh*)self; launch_hst_seed(m->hst, nstep, m->st); return 0; }
static void mesh_hst_drain(void *self) { aa_mesh *m = (aa_mesh*)self; for (int l = 0; l < m->nl; l++) hst_drain_grid(m->lev[l], m->hst); }
// a schedule armed for this call is taken over and disarmed, whatever the call returns
struct MeshHstCall {
  aa_mesh *m;
  explicit MeshHstCall(aa_mesh *m_) : m(m_) {
    m->hst.active = m->hst.armed; m->hst.armed = false;
    if (m->hst.active) for (int l = 0; l < m->nl; l++) m->lev[l]->hst_rows.clear();
  }
  ~MeshHstCall() { m->hst.active = false; }
  void hooks(RunOps &o) const
  { if (m->hst.active) { o.hst = &m->hst; o.hst_row = mesh_hst_row; o.hst_begin = mesh_hst_begin; o.hst_drain = mesh_hst_drain; } }
};

int aa_mesh_run_2d_batch(const aa_mesh *m) { return m && m->two_d && !m->cut ? m->batch_2d : 0; }

int aa_mesh_run_2d(aa_mesh *m, double t_stop, double tlim, int nstep_stop, int *nsteps_done)
{
  if (!m) return aa_fail(-1, "[aa_mesh_run_2d]: null argument");
  MeshHstCall hst(m);
  if (m->cut) return aa_fail(-1, "[aa_mesh_run_2d]: this Mesh is cut into slabs: its levels step together on their slabs' streams, aa_mesh_step");
  if (m->local) return aa_fail(-1, "[aa_mesh_run_2d]: this Mesh is one rank's stack of slabs (aa_mesh_create_local): the ranks agree on dt between steps, aa_mesh_step");
  if (!m->two_d) return aa_fail(-1, "[aa_mesh_run_2d]: this is a Mesh of 3-D Grids: only a Mesh of 2-D Grids (aa_mesh_create_2d) runs many steps per host visit");
  bool small = false;
  for (int l = 0; l < m->nl; l++) {
    const aa_grid *g = m->lev[l];
    if (g->npin > 0) return aa_fail(-1, "[aa_mesh_run_2d]: grid %d (level %d) has pinned zones: such a Mesh steps one at a time, aa_mesh_step", l, g->level);
    if (g->d.Nx1 < AA_NGHOST || g->d.Nx2 < AA_NGHOST) small = true;
  }
  RunOps o;
  o.who = "aa_mesh_run_2d"; o.owner = "root"; o.self = m; o.time = &m->time; o.dt = &m->dt; o.nstep = &m->nstep; o.tlim = m->lev[0]->p.tlim;
  // step by step: the knob at 0, more Grids than the advance kernel's table holds, or a level with fewer zones than ghost zones
  // along a direction (mesh_queue_step_2d: a boundary kernel reads ghost zones there)
  o.stepwise = m->batch_2d == 0 || m->nl > AA_2D_MESH_GRIDS || small;
  o.step = mesh_run_step; o.begin = mesh_run_begin; o.batch = mesh_run_batch; o.end = mesh_run_end; o.st = m->st;
  o.host_syncs = &m->lev[0]->host_syncs;
  hst.hooks(o);
  return run_frame(o, t_stop, tlim, nstep_stop, nsteps_done);
}

// ---- aa_mesh_run_3d: the same for a Mesh of 3-D Grids whose levels are all on the default CTU chain (run.hip on_queued_chain_3d) ---
static int mesh_run_buffers_3d(aa_mesh *m)
{
  if (m->clock) return 0;
  RunClock *h = nullptr, *hd = nullptr; Run3D *d = nullptr;
  if (hipHostMalloc(&h, sizeof(RunClock), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&hd, h, 0) != hipSuccess || hipMalloc(&d, (size_t)m->nl*sizeof(Run3D)) != hipSuccess) {
    if (h) hipHostFree(h);
    (void)hipGetLastError();
    return aa_fail(-2, "[aa_mesh_run_3d]: clock buffers");
  }
  memset(h, 0, sizeof(RunClock));
  m->clock = h; m->clock_dev = hd; m->run3d_dev = d;
  m->tab3.n = m->nl; m->tab3.pad = 0;
  for (int l = 0; l < AA_3D_MESH_GRIDS; l++) {
    const bool in = l < m->nl;
    m->tab3.sc[l] = in ? m->lev[l]->sc : nullptr;
    for (int d3 = 0; d3 < 3; d3++) m->tab3.dx[3*l + d3] = in ? m->lev[l]->d.dx[d3] : 0.0;
  }
  return 0;
}

static bool mesh_has_child(const aa_mesh *m, int l)
{
  for (int c = 0; c + 1 < m->nl; c++) if (m->par[c] == l) return true;
  return false;
}

// One queued step of a 3-D Mesh: mesh_queue_step_2d's schedule and invariants with the 3-D kernels.  Grid l reads dt, `live` and
// the six ratios of ITS dx from the l-th Run3D of the Mesh's array (k3d_mesh_advance keeps time, dt, nstep, `live` and `stepped`
// equal in all of them); the coupling kernels, which join two Grids, read the parent's.
//  * the default CTU chain of every level (run.hip queue_chain_3d: the x2 march, k_correct_all with the other first passes on
//    board, k_flux2_update_keep_dc -- the second-pass fluxes on the level's boundary planes and its children's outlines stay in F).
//    new_dt's maxima ride on the update where the Grid has no child (CFL = true); a Grid WITH children runs the CFL = false
//    instance -- restriction and flux correction rewrite it -- and k_cfl sweeps it behind the last RestrictCorrect pair.  cfl_zone
//    is never contracted (hydro_kernels.hip), and MAX over the same doubles is order-free: dt is the bits of aa_mesh_new_dt.
//    Behind a stop k_cfl only raises the Grid's own maxima, which the next call's seed (or aa_mesh_new_dt) zeroes.
//  * k_restrict_dc / k_flux_correct_dc, finest pair first, behind the `live` guard.
//  * k3d_mesh_advance: nstep++, time += dt, new_dt over the Grids, every Grid's next ratios, the stop rule, `stepped`.
//  * bvals_mhd of every level, the snapshots around every child (k_box_copy_dc, behind `stepped`), the prolongation.
// What is not predicated takes no dt, and behind a stop -- U's active zones untouched, F and the boxes untouched -- it writes what
// is already there or scratch of the step:
//      - k_slopes*, k_eta_edges, the eta memset: slope and eta arrays, which the next taken step fills before it reads them.
//      - the boundary kernels (k_bc_shell, or k_bc in three passes x1, x2, x3).  Every level has AA_NGHOST or more zones along
//        every direction (else: step by step).  A side is either a physical boundary (flag != 0) or fine/coarse (flag 0: the
//        kernels leave it alone; six sides, any mixture).  A ghost zone they write lies outside the active range along one, two
//        or three directions (faces, edges, corners); its source has the coordinates along the physical directions mapped into
//        the active range and the others kept.  If the zone is ghost along physical directions only, the source is an ACTIVE
//        zone, untouched behind the stop.  If it is also ghost along a fine/coarse direction, the source is a prolonged ghost
//        zone -- and the zone itself lies in the region the prolongation of that side writes behind the boundary pass in the
//        same step (k_prolong's region of a side spans the ghost zones of the other two directions), so the boundary kernel
//        is not its last writer.  The three-pass form writes the same zones from the same sources pass by pass.
//      - k_prolong is a function of the snapshot `box` alone, and the box is retaken only behind a step that was taken: a child
//        whose outline lies two parent zones from the parent's own fine/coarse side has prolonged ghost zones of the PARENT in its
//        snapshot, taken (smr.c Prolongate, Step 1) before the parent's prolongation of the same call refreshes them -- a
//        snapshot retaken behind the stop would hold the fresh ones.  So the boxes stay, and k_prolong writes again what is there.
//    A following aa_mesh_step, an output or a restart dump therefore sees the state the last step taken left.
// Plain launches on the Mesh's ONE stream, in stream order; the fork of the levels onto side streams (aa_mesh_step,
// AA_MESH_OVERLAP) is dropped as in 2-D.  Nothing is captured, nothing launched cooperatively, no kernel waits on memory or on
// another workgroup; the host reads the clock only behind run_frame's hipStreamSynchronize.
static int mesh_queue_step_3d(aa_mesh *m, double tlim)
{
  Run3D *rcs = m->run3d_dev;
  for (int l = 0; l < m->nl; l++) queue_chain_3d(m->lev[l], rcs + l, mesh_has_child(m, l) ? nullptr : m->lev[l]->sc);   // (on m->st: every level's stream)
  for (int q = 0; q + 1 < m->nl; q++) {                              // RestrictCorrect, finest pair first
    const int l = m->f2c[q];
    aa_grid *P = m->lev[m->par[l]], *C = m->lev[l + 1];
    const Link &L = m->link[l];
    const Run3D *rc = rcs + m->par[l];
    const int nvar = 5 + P->p.nscal;
    Scope s(P, "smr_restrict_correct");
    hipLaunchKernelGGL(k_restrict_dc, dim3(nblk((long)L.n[0]*L.n[1]*L.n[2], 256)), dim3(256), 0, m->st, C->d, P->d, L, (1u << nvar) - 1u, rc);
    if (m->one_launch) {
      long nmax = 0;
      for (int dim = 0; dim < 6; dim++) {
        const int d = dim >> 1, d1 = (d == 0) ? 1 : 0, d2 = (d == 2) ? 1 : 2;
        if (L.corr[dim]) { const long n = (long)L.n[d1]*L.n[d2]; if (n > nmax) nmax = n; }
      }
      if (nmax > 0) hipLaunchKernelGGL(k_flux_correct_dc, dim3(nblk(nmax, 256), 6), dim3(256), 0, m->st, C->d, P->d, L, -1, nvar, rc);
    } else
    for (int dim = 0; dim < 6; dim++) {
      if (!L.corr[dim]) continue;
      const int d = dim >> 1, d1 = (d == 0) ? 1 : 0, d2 = (d == 2) ? 1 : 2;
      hipLaunchKernelGGL(k_flux_correct_dc, dim3(nblk((long)L.n[d1]*L.n[d2], 256)), dim3(256), 0, m->st, C->d, P->d, L, dim, nvar, rc);
    }
  }
  for (int l = 0; l < m->nl; l++)                                    // new_dt's maxima of the Grids with children
    if (mesh_has_child(m, l)) { Scope s(m->lev[l], "new_dt"); launch_cfl(m->lev[l]->d, m->lev[l]->sc, m->st); }
  { Scope s(m->lev[0], "smr_advance"); launch_3d_mesh_advance(rcs, m->tab3, m->clock_dev, m->st); }
  for (int l = 0; l < m->nl; l++) queue_bvals_3d(m->lev[l]);
  for (int l = 0; l < m->nl; l++) {                                  // Prolongate, in the order of aa_mesh_prolongate
    for (int c = 0; c + 1 < m->nl; c++) {
      if (m->par[c] != l) continue;
      const Link &L = m->link[c];
      const long nb = (long)(L.n[0] + 6)*(L.n[1] + 6)*(L.n[2] + 6);
      hipLaunchKernelGGL(k_box_copy_dc, dim3(nblk(nb, 256)), dim3(256), 0, m->st, m->lev[l]->d, L, m->box[c], rcs + l);
    }
    if (l == 0) continue;
    aa_grid *C = m->lev[l];
    const Link &L = m->link[l - 1];
    const int nvar = 5 + C->p.nscal;
    Scope s(C, "smr_prolongate");
    long cnt[6], nmax = 0;
    for (int dim = 0; dim < 6; dim++) {
      cnt[dim] = 0;
      if (!L.prol[dim]) continue;
      cnt[dim] = 1;
      for (int d = 0; d < 3; d++) cnt[dim] *= (d == (dim >> 1)) ? NG/2 : (C->p.Nx[d] + 2*NG)/2;
      if (cnt[dim] > nmax) nmax = cnt[dim];
    }
    if (m->one_launch) {
      if (nmax > 0) hipLaunchKernelGGL(k_prolong, dim3(nblk(nmax, 128), 6), dim3(128), 0, m->st, C->d, L, m->box[l - 1], -1, nvar);
    } else
    for (int dim = 0; dim < 6; dim++)
      if (cnt[dim] > 0) hipLaunchKernelGGL(k_prolong, dim3(nblk(cnt[dim], 128)), dim3(128), 0, m->st, C->d, L, m->box[l - 1], dim, nvar);
  }
  if (m->hst.active) mesh_queue_hst(m, &rcs[0].c, tlim);      // (as mesh_queue_step_2d)
  return 0;
}

static int mesh_run_begin_3d(void *self, const RunClock &seed, double t_stop, double tlim, int nstep_stop, RunClock **clock)
{
  aa_mesh *m = (aa_mesh*)self;
  if (int rc = mesh_run_buffers_3d(m)) return rc;
  for (int l = 0; l < m->nl; l++) { m->lev[l]->cfl_ready = false; m->lev[l]->active_dirty = true; }
  const Run3D v = {seed, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, t_stop, tlim, m->lev[0]->p.cour_no, nstep_stop, 0};      // (k3d_mesh_seed forms every Grid's ratios)
  launch_3d_mesh_seed(m->run3d_dev, v, m->tab3, m->st);
  *clock = m->clock;
  return 0;
}
static int mesh_run_batch_3d(void *self, double, double tlim, int)
{
  aa_mesh *m = (aa_mesh*)self;
  for (int k = 0; k < m->batch_3d; k++) { int rc = mesh_queue_step_3d(m, tlim); if (rc) return rc; }
  return 0;
}

// whether aa_mesh_run_3d queues this Mesh's steps: the knob above 0, the table holds the Grids, and every level is on the chain
// whose kernels have entries on the device clock, the flux-keeping update entry included
static bool mesh_queues_3d(const aa_mesh *m)
{
  if (!m || m->two_d || m->cut || m->local || m->batch_3d == 0 || m->nl > AA_3D_MESH_GRIDS) return false;
  for (int l = 0; l < m->nl; l++) {
    const aa_grid *g = m->lev[l];
    if (!on_queued_chain_3d(g) || !flux2_update_keep_dc_built(g->p.nscal, g->grav)) return false;
  }
  return true;
}

int aa_mesh_run_3d_batch(const aa_mesh *m) { return mesh_queues_3d(m) ? m->batch_3d : 0; }

int aa_mesh_run_3d(aa_mesh *m, double t_stop, double tlim, int nstep_stop, int *nsteps_done)
{
  if (!m) return aa_fail(-1, "[aa_mesh_run_3d]: null argument");
  MeshHstCall hst(m);
  if (m->cut) return aa_fail(-1, "[aa_mesh_run_3d]: this Mesh is cut into slabs: its levels step together on their slabs' streams, aa_mesh_step");
  if (m->local) return aa_fail(-1, "[aa_mesh_run_3d]: this Mesh is one rank's stack of slabs (aa_mesh_create_local): the ranks agree on dt between steps, aa_mesh_step");
  if (m->two_d) return aa_fail(-1, "[aa_mesh_run_3d]: this is a Mesh of 2-D Grids (aa_mesh_create_2d): aa_mesh_run_2d");
  for (int l = 0; l < m->nl; l++) {
    const aa_grid *g = m->lev[l];
    if (g->npin > 0) return aa_fail(-1, "[aa_mesh_run_3d]: grid %d (level %d) has pinned zones: such a Mesh steps one at a time, aa_mesh_step", l, g->level);
  }
  RunOps o;
  o.who = "aa_mesh_run_3d"; o.owner = "root"; o.self = m; o.time = &m->time; o.dt = &m->dt; o.nstep = &m->nstep; o.tlim = m->lev[0]->p.tlim;
  o.stepwise = !mesh_queues_3d(m);
  o.step = mesh_run_step; o.begin = mesh_run_begin_3d; o.batch = mesh_run_batch_3d; o.end = mesh_run_end; o.st = m->st;
  o.host_syncs = &m->lev[0]->host_syncs;
  hst.hooks(o);
  return run_frame(o, t_stop, tlim, nstep_stop, nsteps_done);
}

// ---- the history schedule of the next aa_mesh_run_2d / aa_mesh_run_3d call (run.hip has a Grid's: aa_run_hst_arm) -----------------
int aa_mesh_run_hst_arm(aa_mesh *m, double t_next, double dt_out, int nlim)
{
  const char *who = "aa_mesh_run_hst_arm";
  if (!m) return aa_fail(-1, "[%s]: null argument", who);
  if (m->cut) return aa_fail(-1, "[%s]: this Mesh is cut into slabs: its levels step together on their slabs' streams, aa_mesh_step and aa_history", who);
  if (m->local) return aa_fail(-1, "[%s]: this Mesh is one rank's stack of slabs (aa_mesh_create_local): the ranks add their rows on the host, aa_mesh_step and aa_history", who);
  const int cap = m->two_d ? m->batch_2d : m->batch_3d;      // rows of one batch; 0: the call steps one at a time and needs no device buffer
  if (cap > 0) {
    for (int l = 0; l < m->nl; l++) if (int rc = hst_grid_buffers(m->lev[l], cap, who)) return rc;
    if (int rc = hst_sched_buffers(m->hst, who)) return rc;
  }
  m->hst.t_next = t_next; m->hst.dt_out = dt_out; m->hst.nlim = nlim < 0 ? -1 : nlim; m->hst.cap = cap;
  m->hst.armed = true;
  return 0;
}
int aa_mesh_run_hst_rows(aa_mesh *m, int grid, int cap, double *rows, int *nrows, double *t_next)
{
  if (!m) return aa_fail(-1, "[aa_mesh_run_hst_rows]: null argument");
  if (grid < 0 || grid >= m->nl) return aa_fail(-1, "[aa_mesh_run_hst_rows]: grid=%d of a Mesh of %d Grids", grid, m->nl);
  const std::vector<double> &r = m->lev[grid]->hst_rows;
  const int n = (int)(r.size()/AA_HST_ROW);
  if (rows && cap > 0) memcpy(rows, r.data(), (size_t)(n < cap ? n : cap)*AA_HST_ROW*sizeof(double));
  if (nrows) *nrows = n;
  if (t_next) *t_next = m->hst.t_next;
  return 0;
}


// ==== a Mesh on in-library slabs: one process, N devices =======================================================================
// Every level is a composite handle of aa_create_cut, all cut at the same root planes: slab s of every level lives on the device
// of the root's slab s, and the pieces on one device form a local stack (mesh_create_local with the links of mesh_cuts.h) on ONE
// stream, so that the level coupling inside a device needs no events.  Restriction, the radiation hand-off and prolongation stay
// inside a slab (prolongation reads the parent's ghost planes where a level starts exactly at a cut, so a posted halo is finished
// first).  What crosses slabs: the x3 halo of every level, the flux correction of the parent plane that lies across a cut from
// the child's boundary, and the scalar reductions.  The order is that of aa_mesh_step / aa_mesh_start above, with one difference
// that keeps the cut run equal to the undivided one: the x3 exchange behind the radiation step is posted AFTER
// ionradRestrictCorrect (the boundary conditions stay where they were), because a slab's ghost planes are its neighbour's ACTIVE
// zones, which the restriction rewrites.  The levels integrate one after the other (no AA_MESH_OVERLAP on a cut Mesh).

static aa_grid *cut_piece(aa_mesh *m, int l, int s)      // level l on root slab s (nullptr: no zones there)
{
  SlabLink *K = m->lev[l]->link;
  const int si = s - K->s0;
  return (si >= 0 && si < K->n) ? m->lev[l]->slab[si] : nullptr;
}
#define CUT_DEV(C, s) HIPCHK(hipSetDevice((C)->dev[s]))

static void cut_destroy(aa_mesh *m)
{
  DevGuard keep;
  CutMesh *C = m->cut;
  for (int s = 0; s < C->n; s++) {
    if (s < (int)C->dev.size()) hipSetDevice(C->dev[s]);
    if (s < (int)C->local.size() && C->local[s]) { hipStreamSynchronize(C->local[s]->st); }
    if (s < (int)C->xfer.size() && C->xfer[s]) { hipStreamSynchronize(C->xfer[s]); hipStreamDestroy(C->xfer[s]); }
    if (s < (int)C->xout.size() && C->xout[s]) { hipStreamSynchronize(C->xout[s]); hipStreamDestroy(C->xout[s]); }
    for (int w = 0; w < 2; w++) {
      if (s < (int)C->send[w].size() && C->send[w][s]) hipFree(C->send[w][s]);
      if (s < (int)C->recv[w].size() && C->recv[w][s]) hipFree(C->recv[w][s]);
      if (s < (int)C->hstage[w].size() && C->hstage[w][s]) hipHostFree(C->hstage[w][s]);
    }
    if (s < (int)C->packed.size() && C->packed[s]) hipEventDestroy(C->packed[s]);
    if (s < (int)C->copied.size() && C->copied[s]) hipEventDestroy(C->copied[s]);
    if (s < (int)C->unpacked.size() && C->unpacked[s]) hipEventDestroy(C->unpacked[s]);
    if (s < (int)C->staged_ev.size() && C->staged_ev[s]) hipEventDestroy(C->staged_ev[s]);
  }
  for (FluxMsg &q : C->msgs) {
    if (q.src < (int)C->dev.size()) { hipSetDevice(C->dev[q.src]); if (C->local[q.src]) hipStreamSynchronize(C->local[q.src]->st); }
    if (q.dst < (int)C->dev.size()) { hipSetDevice(C->dev[q.dst]); if (C->local[q.dst]) hipStreamSynchronize(C->local[q.dst]->st); }
    if (q.sbuf) { hipSetDevice(C->dev[q.src]); hipFree(q.sbuf); }
    if (q.rbuf) { hipSetDevice(C->dev[q.dst]); hipFree(q.rbuf); }
    if (q.hbuf) hipHostFree(q.hbuf);
    if (q.sent) hipEventDestroy(q.sent);
    if (q.done) hipEventDestroy(q.done);
  }
  for (int s = 0; s < (int)C->local.size(); s++) if (C->local[s]) { hipSetDevice(C->dev[s]); aa_mesh_destroy(C->local[s]); }
  delete C->mc;
  delete C;
  delete m;
}

static int cut_create(int nlevels, aa_grid **levels, const int *disp, aa_mesh **out)
{
  DevGuard keep;
  SlabLink *R = levels[0]->link;
  for (int l = 0; l < nlevels; l++) {
    aa_grid *g = levels[l];
    SlabLink *K = g->link;
    if (!K->by_cuts) return aa_fail(-1, "[aa_mesh_create]: levels[%d] was cut by aa_create (aa_params.nslab / AA_NGPU): the levels of a cut Mesh come from aa_create_cut", l);
    if (g->level != l) return aa_fail(-1, "[aa_mesh_create]: levels[%d] is on level %d: several Domains on a level are not cut across GPUs (one Domain per level on a cut Mesh)", l, g->level);
    if (K->ntotal != R->ntotal || K->cuts != R->cuts) return aa_fail(-1, "[aa_mesh_create]: levels[%d] has different cuts than the root: all levels of a Mesh are cut at the same root planes", l);
    for (int si = 0; si < K->n; si++)
      if (K->dev[si] != R->dev[K->s0 + si]) return aa_fail(-1, "[aa_mesh_create]: slab %d of levels[%d] lives on HIP device %d, the root's on %d", K->s0 + si, l, K->dev[si], R->dev[K->s0 + si]);
    if (l && K->kdisp != disp[3*l + 2]) return aa_fail(-1, "[aa_mesh_create]: levels[%d] was cut with kdisp = %d, the Mesh gives kDisp = %d", l, K->kdisp, disp[3*l + 2]);
    if (g->keep_flux) return aa_fail(-1, "[aa_mesh_create]: levels[%d] already belongs to a Mesh", l);
    if (g->p.integrator != levels[0]->p.integrator) return aa_fail(-1, "[aa_mesh_create]: levels[%d] has integrator %d, the root %d", l, g->p.integrator, levels[0]->p.integrator);
  }
  // the nesting rules of mesh_create_nested, on the undivided Domains
  mc_level lev[AA_MAXLEV];
  for (int l = 0; l < nlevels; l++) for (int d = 0; d < 3; d++) { lev[l].Nx[d] = levels[l]->p.Nx[d]; lev[l].disp[d] = l ? disp[3*l + d] : 0; }
  for (int c = 1; c < nlevels; c++) {
    const int irefine = 1 << c;
    for (int d = 0; d < 3; d++) {
      const int dc = lev[c].disp[d], nc = lev[c].Nx[d], dp = lev[c - 1].disp[d], np = lev[c - 1].Nx[d];
      const int a = dc/2 - dp, b = (dc + nc)/2 - dp;
      if ((dc & 1) || (nc & 1) || a < 0 || b > np) return aa_fail(-1, "[aa_mesh_create]: grid %d is not nested in grid %d along x%d", c, c - 1, d + 1);
      const bool plo = (dc != 0), phi = ((dc + nc)/irefine != levels[c]->p.rootNx[d]);
      if ((a == 0 && plo) || (b == np && phi)) return aa_fail(-1, "[init_mesh] child Domain (grid %d) touches its parent in x%d", c, d + 1);
    }
    if (levels[c - 1]->p.ion && (lev[c - 1].disp[1] || lev[c - 1].disp[2])) {
      if (!deep_radiation_fixed())
        return aa_fail(-1, "[aa_mesh_create]: radiation across a displaced parent (grid %d) is undefined in the reference "
                           "(set AA_SMR_DEEP_RADIATION=fixed for the corrected hand-off)", c - 1);
    }
  }
  aa_mesh *m = new aa_mesh();
  CutMesh *C = new CutMesh();
  m->cut = C; m->nl = nlevels; m->overlap = false; m->own_stream = false;
  for (int l = 0; l < AA_MAXLEV; l++) { m->lev[l] = nullptr; m->box[l] = nullptr; }
  for (int l = 0; l < nlevels; l++) { m->lev[l] = levels[l]; m->par[l] = l; for (int d = 0; d < 3; d++) m->disp[l][d] = lev[l].disp[d]; }
  for (int l = 0; l + 1 < nlevels; l++) m->f2c[l] = nlevels - 2 - l;
  C->n = R->ntotal; C->dev = R->dev; C->staged = R->staged;
  C->mc = new mc_mesh();
  char msg[256] = "";
  const aa_params &p0 = levels[0]->p;
  if (mc_build(C->mc, nlevels, lev, p0.rootNx, C->n, R->cuts.data(), p0.bc[4] == AA_BC_PERIODIC && p0.bc[5] == AA_BC_PERIODIC, msg, sizeof msg)) {
    cut_destroy(m); return aa_fail(-1, "[aa_mesh_create]: %s", msg);
  }
  { const char *e = getenv("AA_MESH_HALO_BATCH"); C->batch = e ? atoi(e) != 0 : true; }
  const int n = C->n, nvar = 5 + p0.nscal;
#define CUT_CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { cut_destroy(m); \
  return aa_fail(-2, "[aa_mesh_create] HIP error %s at %s:%d: %s", #x, __FILE__, __LINE__, hipGetErrorString(e_)); } } while (0)
  C->local.assign(n, nullptr);
  for (int s = 0; s < n; s++) {
    const mc_slab &S = C->mc->slab[s];
    aa_grid *pieces[AA_MAXLEV]; int links[21*AA_MAXLEV];
    for (int l = 0; l < S.nl; l++) {
      pieces[l] = cut_piece(m, l, s);
      SlabLink *K = levels[l]->link;
      const int d3 = lev[l].disp[2];
      if (!pieces[l] || K->k0[s - K->s0] != S.piece[l].k0 - d3 || K->nk[s - K->s0] != S.piece[l].k1 - S.piece[l].k0) {
        cut_destroy(m); return aa_fail(-1, "[aa_mesh_create]: level %d on slab %d does not lie over the root's planes %d .. %d", l, s, R->cuts[s], R->cuts[s + 1]);
      }
    }
    for (int l = 0; l + 1 < S.nl; l++) mc_link_ints(&S.link[l], links + 21*l);
    CUT_CHK(hipSetDevice(C->dev[s]));
    int rc = mesh_create_local(S.nl, pieces, links, &C->local[s], false);
    if (rc) { C->local[s] = nullptr; cut_destroy(m); return rc; }
  }
  // the exchange of all levels in one launch per slab: buffers, events and streams as slabs.hip keeps them per Grid
  C->hb.assign(n, HaloBatch());
  C->packed.assign(n, nullptr); C->copied.assign(n, nullptr); C->unpacked.assign(n, nullptr); C->staged_ev.assign(n, nullptr);
  C->copied_valid.assign(n, false); C->unpacked_valid.assign(n, false);
  C->xfer.assign(n, nullptr); C->xout.assign(n, nullptr);
  for (int w = 0; w < 2; w++) { C->send[w].assign(n, nullptr); C->recv[w].assign(n, nullptr); C->hstage[w].assign(n, nullptr); }
  for (int s = 0; s < n; s++) {
    const mc_slab &S = C->mc->slab[s];
    HaloBatch &B = C->hb[s];
    memset(&B, 0, sizeof B);
    B.nvar = nvar;
    long first = 0;
    for (int l = 0; l < S.nl; l++) {
      const aa_grid *g = cut_piece(m, l, s);
      HaloLev &h = B.lev[l];
      h.U = g->d.U; h.sJ = g->d.sJ; h.sK = g->d.sK; h.nc = g->d.nc; h.first = first; h.N1 = g->d.N1; h.N2 = g->d.N2;
      h.kp[0] = g->d.ks; h.kp[1] = g->d.ke - NG + 1; h.ku[0] = g->d.ks - NG; h.ku[1] = g->d.ke + 1;
      first += (long)g->d.N1*g->d.N2*NG;
      if (S.piece[l].lo >= 0) { B.nshare[0] = l + 1; B.total[0] = first; }
      if (S.piece[l].hi >= 0) { B.nshare[1] = l + 1; B.total[1] = first; }
    }
    CUT_CHK(hipSetDevice(C->dev[s]));
    for (int w = 0; w < 2; w++) if (B.total[w] > 0) {
      const size_t bytes = (size_t)B.total[w]*nvar*sizeof(Real);
      CUT_CHK(hipMalloc(&C->send[w][s], bytes)); CUT_CHK(hipMalloc(&C->recv[w][s], bytes));
      if (C->staged) CUT_CHK(hipHostMalloc(&C->hstage[w][s], bytes));
    }
    CUT_CHK(hipEventCreateWithFlags(&C->packed[s], hipEventDisableTiming));
    CUT_CHK(hipEventCreateWithFlags(&C->copied[s], hipEventDisableTiming));
    CUT_CHK(hipEventCreateWithFlags(&C->unpacked[s], hipEventDisableTiming));
    CUT_CHK(hipStreamCreateWithFlags(&C->xfer[s], hipStreamNonBlocking));
    if (C->staged) {
      CUT_CHK(hipStreamCreateWithFlags(&C->xout[s], hipStreamNonBlocking));
      CUT_CHK(hipEventCreateWithFlags(&C->staged_ev[s], hipEventDisableTiming));
    }
  }
  // flux corrections that cross a cut (corr_in of the receiving slab names the sender)
  for (int t = 0; t < n; t++) {
    const mc_slab &S = C->mc->slab[t];
    for (int q = 0; q < S.ncorr_in; q++) {
      const mc_corr_in &ci = S.corr_in[q];
      if (C->mc->slab[ci.src].link[ci.level].corr_to[ci.side] != t) { cut_destroy(m); return aa_fail(-1, "[aa_mesh_create]: flux correction tables disagree (level %d, slabs %d -> %d)", ci.level, ci.src, t); }
      FluxMsg f;
      f.l = ci.level; f.side = ci.side; f.src = ci.src; f.dst = t; f.i0 = ci.i0; f.j0 = ci.j0; f.n1 = ci.n1; f.n2 = ci.n2;
      C->msgs.push_back(f);
      FluxMsg &F = C->msgs.back();
      const size_t bytes = (size_t)F.n1*F.n2*6*sizeof(Real);
      CUT_CHK(hipSetDevice(C->dev[F.src]));
      CUT_CHK(hipMalloc(&F.sbuf, bytes));
      CUT_CHK(hipEventCreateWithFlags(&F.sent, hipEventDisableTiming));
      CUT_CHK(hipSetDevice(C->dev[F.dst]));
      CUT_CHK(hipMalloc(&F.rbuf, bytes));
      CUT_CHK(hipEventCreateWithFlags(&F.done, hipEventDisableTiming));
      if (C->staged) CUT_CHK(hipHostMalloc(&F.hbuf, bytes));
    }
  }
#undef CUT_CHK
  *out = m;
  return 0;
}

static int cut_restrict_correct_pair(aa_mesh *m, int l)
{
  if (l < 0 || l + 1 >= m->nl) return aa_fail(-1, "[aa_mesh_restrict_correct_pair]: pair %d", l);
  DevGuard keep;
  CutMesh *C = m->cut;
  for (int s = 0; s < C->n; s++) {
    if (C->mc->slab[s].nl <= l + 1) continue;
    CUT_DEV(C, s);
    int rc = aa_mesh_restrict_correct_pair(C->local[s], l); if (rc) return rc;
  }
  for (FluxMsg &F : C->msgs) {
    if (F.l != l) continue;
    const size_t bytes = (size_t)F.n1*F.n2*6*sizeof(Real);
    aa_grid *ch = cut_piece(m, l + 1, F.src), *pa = cut_piece(m, l, F.dst);
    hipStream_t ss = C->local[F.src]->st, ds = C->local[F.dst]->st;
    CUT_DEV(C, F.src);
    if (F.done_valid) HIPCHK(hipStreamWaitEvent(ss, F.done, 0));            // the previous message has left sbuf
    hipLaunchKernelGGL(k_flux_x3_export, dim3(nblk((long)F.n1*F.n2, 256)), dim3(256), 0, ss, ch->d, F.side, F.sbuf);
    if (C->staged) HIPCHK(hipMemcpyAsync(F.hbuf, F.sbuf, bytes, hipMemcpyDeviceToHost, ss));
    HIPCHK(hipEventRecord(F.sent, ss));
    CUT_DEV(C, F.dst);
    HIPCHK(hipStreamWaitEvent(ds, F.sent, 0));
    if (C->staged) HIPCHK(hipMemcpyAsync(F.rbuf, F.hbuf, bytes, hipMemcpyHostToDevice, ds));
    else if (C->dev[F.src] == C->dev[F.dst]) HIPCHK(hipMemcpyAsync(F.rbuf, F.sbuf, bytes, hipMemcpyDeviceToDevice, ds));
    else HIPCHK(hipMemcpyPeerAsync(F.rbuf, C->dev[F.dst], F.sbuf, C->dev[F.src], bytes, ds));
    HIPCHK(hipEventRecord(F.done, ds)); F.done_valid = true;
    pa->active_dirty = true;
    hipLaunchKernelGGL(k_flux_x3_apply, dim3(nblk((long)F.n1*F.n2, 256)), dim3(256), 0, ds, pa->d, F.side, F.i0, F.j0, F.n1, F.n2,
                       5 + pa->p.nscal, (Real)pa->dt, F.rbuf);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

static int cut_ionrad_restrict_correct(aa_mesh *m)
{
  DevGuard keep;
  CutMesh *C = m->cut;
  for (int s = 0; s < C->n; s++) { CUT_DEV(C, s); int rc = aa_mesh_ionrad_restrict_correct(C->local[s]); if (rc) return rc; }
  return 0;
}

static int cut_ionflux_prolong(aa_mesh *m, int l)
{
  DevGuard keep;
  CutMesh *C = m->cut;
  for (int s = 0; s < C->n; s++) {
    if (C->mc->slab[s].nl <= l) continue;
    CUT_DEV(C, s);
    int rc = aa_mesh_ionflux_prolong(C->local[s], l); if (rc) return rc;
  }
  return 0;
}

// the ghost planes of the exchange of all levels are written (MPI_Waitall + unpack of every level, one launch per slab)
static int cut_halo_finish(aa_mesh *m)
{
  CutMesh *C = m->cut;
  if (!C->halo_due) return 0;
  C->halo_due = false;
  DevGuard keep;
  for (int r = 0; r < C->n; r++) {
    const HaloBatch &B = C->hb[r];
    if (B.total[0] == 0 && B.total[1] == 0) continue;
    CUT_DEV(C, r);
    hipStream_t st = C->local[r]->st;
    HIPCHK(hipStreamWaitEvent(st, C->copied[r], 0));
    const long tot = B.total[0] > B.total[1] ? B.total[0] : B.total[1];
    hipLaunchKernelGGL(k_halo_levels<false>, dim3(nblk(tot, 256), 2), dim3(256), 0, st, B,
                       B.total[0] ? C->recv[0][r] : (Real*)nullptr, B.total[1] ? C->recv[1][r] : (Real*)nullptr);
    HIPCHK(hipEventRecord(C->unpacked[r], st));
    C->unpacked_valid[r] = true;
    C->counts[0]++;
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// bvals_mhd of every level (main.c:635-644, :412-440): the boundary conditions of every piece, then the x3 halo of all levels --
// ONE pack launch per slab, ONE copy per neighbour, ONE unpack launch per slab (cut_halo_finish); with AA_MESH_HALO_BATCH=0 one
// exchange per level through the levels' own buffers (slabs.hip)
static int cut_exchange_all(aa_mesh *m, bool with_bc)
{
  CutMesh *C = m->cut;
  int rc;
  if ((rc = cut_halo_finish(m))) return rc;
  for (int l = 0; l < m->nl; l++) {
    if (with_bc) { if ((rc = slabs_bvals_local(m->lev[l]))) return rc; }
    else if ((rc = slabs_halo_finish(m->lev[l]))) return rc;
  }
  if (!C->batch) {
    for (int l = 0; l < m->nl; l++) if ((rc = slabs_halo_exchange(m->lev[l]))) return rc;
    return 0;
  }
  DevGuard keep;
  const int nvar = C->hb[0].nvar;
  bool any = false;
  for (int s = 0; s < C->n; s++) {
    const HaloBatch &B = C->hb[s];
    if (B.total[0] == 0 && B.total[1] == 0) continue;
    any = true;
    CUT_DEV(C, s);
    hipStream_t st = C->local[s]->st;
    const mc_piece &root = C->mc->slab[s].piece[0];
    // my send buffers are free once both neighbours have pulled the previous exchange out of them
    for (int o : {root.lo, root.hi}) if (o >= 0 && C->copied_valid[o]) HIPCHK(hipStreamWaitEvent(st, C->copied[o], 0));
    const long tot = B.total[0] > B.total[1] ? B.total[0] : B.total[1];
    hipLaunchKernelGGL(k_halo_levels<true>, dim3(nblk(tot, 256), 2), dim3(256), 0, st, B,
                       B.total[0] ? C->send[0][s] : (Real*)nullptr, B.total[1] ? C->send[1][s] : (Real*)nullptr);
    HIPCHK(hipEventRecord(C->packed[s], st));
    C->counts[0]++;
    if (C->staged) {
      HIPCHK(hipStreamWaitEvent(C->xout[s], C->packed[s], 0));
      for (int w = 0; w < 2; w++) if (B.total[w])
        HIPCHK(hipMemcpyAsync(C->hstage[w][s], C->send[w][s], (size_t)B.total[w]*nvar*sizeof(Real), hipMemcpyDeviceToHost, C->xout[s]));
      HIPCHK(hipEventRecord(C->staged_ev[s], C->xout[s]));
    }
  }
  for (int r = 0; r < C->n; r++) {
    const HaloBatch &B = C->hb[r];
    if (B.total[0] == 0 && B.total[1] == 0) continue;
    CUT_DEV(C, r);
    hipStream_t x = C->xfer[r];
    const mc_piece &root = C->mc->slab[r].piece[0];
    if (C->unpacked_valid[r]) HIPCHK(hipStreamWaitEvent(x, C->unpacked[r], 0));     // my recv buffers are free
    for (int w = 0; w < 2; w++) {
      if (!B.total[w]) continue;
      const int o = w ? root.hi : root.lo;      // my lower ghost planes are the lower neighbour's upper planes, and the other way round
      const size_t bytes = (size_t)B.total[w]*nvar*sizeof(Real);
      HIPCHK(hipStreamWaitEvent(x, C->staged ? C->staged_ev[o] : C->packed[o], 0));
      if (C->staged) HIPCHK(hipMemcpyAsync(C->recv[w][r], C->hstage[1 - w][o], bytes, hipMemcpyHostToDevice, x));
      else if (C->dev[r] == C->dev[o]) HIPCHK(hipMemcpyAsync(C->recv[w][r], C->send[1 - w][o], bytes, hipMemcpyDeviceToDevice, x));
      else HIPCHK(hipMemcpyPeerAsync(C->recv[w][r], C->dev[r], C->send[1 - w][o], C->dev[o], bytes, x));
      C->counts[1]++;
    }
    HIPCHK(hipEventRecord(C->copied[r], x));
    C->copied_valid[r] = true;
  }
  C->halo_due = any;
  C->counts[2]++;
  HIPCHK(hipGetLastError());
  return 0;
}

static int cut_halo_flush(aa_mesh *m)      // every posted exchange, of all levels or of one, has written its ghost planes
{
  int rc = cut_halo_finish(m); if (rc) return rc;
  for (int l = 0; l < m->nl; l++) if ((rc = slabs_halo_finish(m->lev[l]))) return rc;
  return 0;
}

static int cut_prolongate(aa_mesh *m)
{
  int rc = cut_halo_flush(m); if (rc) return rc;      // k_box_copy reads the parent's ghost planes where a child starts at a cut
  DevGuard keep;
  CutMesh *C = m->cut;
  for (int s = 0; s < C->n; s++) { CUT_DEV(C, s); if ((rc = aa_mesh_prolongate(C->local[s]))) return rc; }
  return 0;
}

// new_dt.c:32 over all levels: every piece leaves its maxima in pinned memory, ONE wait, then the host folds -- MAX over the
// slabs of a level, carried from level to level as aa_mesh_new_dt does
static int cut_new_dt(aa_mesh *m)
{
  DevGuard keep;
  CutMesh *C = m->cut;
  int rc;
  for (int l = 0; l < m->nl; l++) if ((rc = slabs_cfl_queue(m->lev[l]))) return rc;
  for (int s = 0; s < C->n; s++) { CUT_DEV(C, s); HIPCHK(hipStreamSynchronize(C->local[s]->st)); }
  m->lev[0]->host_syncs++;
  double cum[3] = {0.0, 0.0, 0.0}, max_dti = 0.0;
  for (int l = 0; l < m->nl; l++) {
    const SlabLink *K = m->lev[l]->link;
    for (int si = 0; si < K->n; si++) { double v[3]; max_v_of(K->hsc[si], v); dt_carry(cum, v, 3); }
    max_dti = dt_fold(max_dti, cum, m->lev[l]->slab[0]->d.dx, 3);
  }
  mesh_pick_dt(m, max_dti);
  for (int l = 0; l < m->nl; l++) { m->lev[l]->dt = m->dt; slabs_push_state(m->lev[l]); }
  return 0;
}

static int cut_start(aa_mesh *m, bool with_dt)      // aa_mesh_start / aa_mesh_resume
{
  int rc;
  if ((rc = aa_mesh_restrict_correct(m))) return rc;
  if ((rc = cut_exchange_all(m, true))) return rc;
  for (int l = 0; l < m->nl; l++) if ((rc = aa_bvals_ionrad(m->lev[l]))) return rc;
  if ((rc = cut_prolongate(m))) return rc;
  return with_dt ? cut_new_dt(m) : 0;
}

static int cut_step(aa_mesh *m, int *niter)         // aa_mesh_step
{
  int rc;
  aa_grid *root = m->lev[0];
  if (root->p.ion && root->nradplane > 0) {
    for (int l = 0; l < m->nl; l++) {
      int n = 0;
      m->lev[l]->time = m->time;
      if ((rc = aa_mesh_ion_radtransfer(m, l, &n))) return rc;
      if (niter) niter[l] = n;
      if ((rc = slabs_bvals_local(m->lev[l]))) return rc;       // (the exchange follows the restriction: see the head of this part)
    }
    if ((rc = cut_ionrad_restrict_correct(m))) return rc;
    if ((rc = cut_exchange_all(m, false))) return rc;
  } else if (niter) for (int l = 0; l < m->nl; l++) niter[l] = 0;
  if ((rc = cut_halo_flush(m))) return rc;
  for (int l = 0; l < m->nl; l++) {
    aa_grid *g = m->lev[l];
    if ((rc = (g->p.integrator == 1 ? aa_integrate_3d_vl(g) : aa_integrate_3d_ctu(g)))) return rc;
  }
  if ((rc = aa_mesh_restrict_correct(m))) return rc;
  for (int l = 0; l < m->nl; l++)
    if (m->lev[l]->npin > 0 && (rc = aa_apply_pinned_cells(m->lev[l]))) return rc;
  m->nstep++; m->time += m->dt;
  for (int l = 0; l < m->nl; l++) { m->lev[l]->time = m->time; m->lev[l]->nstep = m->nstep; }
  if ((rc = cut_new_dt(m))) return rc;
  if ((rc = cut_exchange_all(m, true))) return rc;
  return cut_prolongate(m);
}

// launches (pack + unpack), copies and exchanges of the all-level x3 exchanges of a cut Mesh so far (zeros on any other Mesh, and
// with AA_MESH_HALO_BATCH=0, where every level exchanges through its own Grid's kernels)
int aa_mesh_halo_counts(const aa_mesh *m, long long out[3])
{
  for (int q = 0; q < 3; q++) out[q] = m->cut ? m->cut->counts[q] : 0;
  return 0;
}
int aa_mesh_nslab(const aa_mesh *m) { return m->cut ? m->cut->n : 1; }

}  // extern "C"
