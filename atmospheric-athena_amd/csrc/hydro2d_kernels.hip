// hydro2d_kernels.hip -- the hydro hot path of a 2-D Grid (Nx3 = 1; gfx950): integrate_2d_ctu.c and integrate_2d_vl.c of the
// reference for HYDRO, ADIABATIC, CARTESIAN, second or third order, no gravity, no cooling, no passive scalar.  The per-cell and
// per-face arithmetic is that of hydro_dev.h, unchanged; this file only restates the 2-D loop nests.
//
// Layout (api.hip aa_create): one plane [N2][sJ] per field, no ghost zones along x3 (ks = ke = 0), fields nc = sJ*N2 apart,
//   U   5 fields  d, M1, M2, M3, E                               (global momentum frame)
//   LR  20 fields [dir][L|R][d, Mx, My, Mz, E]                   (SWEEP frame: x1 (M1,M2,M3), x2 (M2,M3,M1); integrate_2d_ctu.c:1087-1097)
//                 van Leer: fields 0 .. 4 hold U^{n+1/2} in the global frame
//   F   10 fields [dir][d, Mx, My, Mz, E]                        first-pass fluxes, sweep frame (CTU only)
//   eta 2 fields  eta1, eta2                                     (CTU only)
//   edge 5 x ntx x N2 doubles: what lane 0 / lane 63 of an x1 tile needs from the neighbouring tile (see below)
//
// Kernel shape: a block is T2_R wavefronts, each 64 lanes along x1 on whole 128-byte lines (tiles start at i = is, which
// aa_create puts on a line), one row of zones per wavefront.  Tiles do not overlap in x1: what a face needs of the zone
// one lane down (its left state) or up (the flux of the upper face) comes by wavefront shuffle; across the tile's edge it
// comes from the `edge` buffer, filled by a small side kernel with one thread per tile edge and row.  Along x2 the same
// quantities travel through LDS between the block's wavefronts; one wavefront of the block is a halo row that only feeds
// its neighbour.  Second-pass fluxes never reach HBM: k2d_step computes the fluxes of a zone's two lower faces, takes the
// upper ones from its neighbours, updates the zone and folds new_dt's maxima.
//
// CTU: k2d_edge_wl, k2d_first, k2d_correct, k2d_edge<CTU2>, k2d_step<CTU2>   (3 launches + 2 side kernels)
// VL : k2d_edge<VL1>, k2d_step<VL1>, k2d_edge<VL2>, k2d_step<VL2>            (2 launches + 2 side kernels)
// A level of a Mesh (csrc/smr.hip, aa_mesh_create_2d) takes k2d_step_keep<CTU2 | VL2> in place of k2d_step: the same body, which
// also stores the second-pass fluxes of the faces on the level-boundary lines into F for the flux correction.
//
// aa_run_2d (csrc/api2d.hip) queues many steps without the host in between: every kernel above has a second entry point, *_dc, with
// the same body, which takes dt from the device clock (hydro2d_launch.h Run2D) instead of a kernel argument and returns at once when
// the clock has stopped; k2d_advance, one wavefront behind the update kernel, does new_dt and the loop's bookkeeping on the device.
//
// Third order (aa_set_order_2d; the reference's --with-order=3): everything that reconstructs -- k2d_edge_wl, k2d_first, and the VL2
// forms of k2d_edge and k2d_step -- has a second instantiation, ORD = 3, picked on the host (with_ord).  Only recon_zone differs: it
// reads the five zones m - 2s .. m + 2s from memory, evaluates the three limited slopes the zone's parabola needs and calls ppm_cell
// (lr_states_ppm.c).  What travels by shuffle, LDS and the edge buffer are face states and fluxes, as before, so the tiling is that
// of second order.  Stencil bounds: the first pass reconstructs the zones of [is-2, ie+2] x [js-2, je+2], whose five-zone stencils
// end at is-4 = 0 and ie+4 = N1-1 (js-4 = 0, je+4 = N2-1): exactly the four ghost zones; VL2 reconstructs [is-1, ie+1] x [js-1, je+1]
// on a U^{n+1/2} that VL1 wrote over [is-3, ie+3] x [js-3, je+3].  Threads outside the range compute on a zone clamped into it.
#include <hip/hip_runtime.h>
#include "grid.h"
#include "hydro_dev.h"
#include "hydro2d_launch.h"

namespace aa {

#define T2_W 64
#define T2_R 8            /* wavefronts (rows) per block, one of them the halo row */

AA_DEV Real *U2(const DevGrid &g, int v) { return g.U + (long)v*g.nc; }
AA_DEV Real *LR2(const DevGrid &g, int d, int side, int v) { return g.LR + (long)((d*2 + side)*5 + v)*g.nc; }
AA_DEV Real *F2(const DevGrid &g, int d, int v) { return g.F + (long)(d*5 + v)*g.nc; }
AA_DEV int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// a zone of a global-frame state (5 fields nc apart) in the sweep frame of direction D
template <int D>
AA_DEV void load_cons(const Real *b, long nc, long m, Real u[6])
{
  u[0] = b[m]; u[4] = b[4*nc + m]; u[5] = 0.0;
  if (D == 0) { u[1] = b[nc + m];   u[2] = b[2*nc + m]; u[3] = b[3*nc + m]; }
  else        { u[1] = b[2*nc + m]; u[2] = b[3*nc + m]; u[3] = b[nc + m]; }
}
AA_DEV void load5(const Real *b, long nc, long m, Real u[6])
{
#pragma unroll
  for (int v = 0; v < 5; v++) u[v] = b[(long)v*nc + m];
  u[5] = 0.0;
}
AA_DEV void store5(Real *b, long nc, long m, const Real u[6])
{
#pragma unroll
  for (int v = 0; v < 5; v++) b[(long)v*nc + m] = u[v];
}

// the zone at m reconstructed along D: Wl of its upper face, Wr of its lower face.  ORD 2: PLM (lr_states_plm.c) from the zones
// m - s .. m + s; ORD 3: PPM (lr_states_ppm.c) from m - 2s .. m + 2s, the slopes of m - s, m, m + s evaluated here (the direct form:
// a zone's slope is evaluated by each of the three zones whose parabola needs it).  TRACE: with characteristic tracing (CTU)
template <int D, bool TRACE, int ORD>
AA_DEV void recon_zone(const Real *src, const DevGrid &g, long m, Real dt, Real wl_next[6], Real wr_here[6])
{
  const long s = D == 0 ? 1L : g.sJ;
  if (ORD == 3) {
    Real u[6], w5[5][6], dw[3][6];
#pragma unroll
    for (int q = 0; q < 5; q++) { load_cons<D>(src, g.nc, m + (q - 2)*s, u); cons_to_prim<0>(u, w5[q], g.Gamma_1); }
#pragma unroll
    for (int q = 0; q < 3; q++) limited_slopes<0>(w5[q], w5[q + 1], w5[q + 2], g.Gamma, dw[q]);
    ppm_cell<0, TRACE>(w5[1], w5[2], w5[3], dw[0], dw[1], dw[2], dt/g.dx[D], g.Gamma, wl_next, wr_here);
    return;
  }
  Real u[6], wm[6], w[6], wp[6];
  load_cons<D>(src, g.nc, m - s, u); cons_to_prim<0>(u, wm, g.Gamma_1);
  load_cons<D>(src, g.nc, m, u);     cons_to_prim<0>(u, w, g.Gamma_1);
  load_cons<D>(src, g.nc, m + s, u); cons_to_prim<0>(u, wp, g.Gamma_1);
  plm_cell<0, TRACE>(wm, w, wp, dt/g.dx[D], g.Gamma, wl_next, wr_here);
}

// first-pass flux of one face from its primitive L/R states (integrate_2d_ctu.c Step 1d / 2d: etah = 0)
AA_DEV void face_first(const DevGrid &g, const Real wl[6], const Real wr[6], Real ul[6], Real ur[6], Real f[6])
{
  prim_to_cons<0>(wl, ul, g.Gamma_1, g.rGamma_1);
  prim_to_cons<0>(wr, ur, g.Gamma_1, g.rGamma_1);
  flux_roe<0>(ul, ur, wl, wr, 0.0, g.Gamma, g.Gamma_1, f);
}

// ---- CTU, Steps 1 and 2 -------------------------------------------------------------------------------------------------
// side kernel: the left state of the first x1 face of every tile but the first (the zone below it belongs to the tile before)
template <int ORD>
AA_DEV void edge_wl_body(const DevGrid &g, Real dt, Real *edge, int ntx)
{
  const int jl = g.js - 2, nj = g.je - g.js + 5;
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= (long)nj*(ntx - 1)) return;
  const int j = jl + (int)(lin % nj), t = 1 + (int)(lin / nj);
  const int i0 = g.is + 64*(t - 1);
  if (i0 > g.ie + 2) return;
  Real wl[6], wr[6];
  recon_zone<0, true, ORD>(g.U, g, (long)j*g.sJ + i0 - 1, dt, wl, wr);
  const long es = (long)ntx*g.N2;
#pragma unroll
  for (int v = 0; v < 5; v++) edge[v*es + (long)t*g.N2 + j] = wl[v];
}

template <int ORD>
__global__ void __launch_bounds__(64)
k2d_edge_wl(DevGrid g, Real dt, Real *edge, int ntx)
{ edge_wl_body<ORD>(g, dt, edge, ntx); }

// L/R states and first-pass fluxes of the lower x1 and x2 face of every zone of [is-2, ie+2] x [js-2, je+2]
template <int ORD>
AA_DEV void first_body(const DevGrid &g, Real dt, const Real *edge)
{
  __shared__ Real sh[5][T2_R][T2_W];
  const int lane = threadIdx.x, ty = threadIdx.y;
  const int il = g.is - 2, iu = g.ie + 2, jl = g.js - 2, ju = g.je + 2;
  const int i = g.is + 64*((int)blockIdx.x - 1) + lane;
  const int j = jl + (T2_R - 1)*(int)blockIdx.y + ty - 1;           // ty = 0: the halo row below the block's zones
  const int ic = clampi(i, il, iu), jc = clampi(j, jl, ju);         // (threads outside the range compute on a zone inside it and store nothing)
  const bool in_i = i >= il && i <= iu, in_j = j >= jl && j <= ju;
  const long m = (long)jc*g.sJ + ic;
  Real wl[6], wr[6], wln[6], ul[6], ur[6], f[6];

  recon_zone<1, true, ORD>(g.U, g, m, dt, wln, wr);
#pragma unroll
  for (int v = 0; v < 5; v++) sh[v][ty][lane] = wln[v];
  Real wr2[6];
#pragma unroll
  for (int v = 0; v < 6; v++) wr2[v] = wr[v];

  if (ty > 0) {          // (one row per wavefront: the branch is uniform)
    recon_zone<0, true, ORD>(g.U, g, m, dt, wln, wr);
#pragma unroll
    for (int v = 0; v < 5; v++) wl[v] = __shfl_up(wln[v], 1);
    wl[5] = 0.0;
    if (lane == 0 && blockIdx.x >= 1) {
      const long es = (long)gridDim.x*g.N2;
#pragma unroll
      for (int v = 0; v < 5; v++) wl[v] = edge[v*es + (long)blockIdx.x*g.N2 + jc];
    }
    face_first(g, wl, wr, ul, ur, f);
    if (in_j && i >= il + 1 && i <= iu) {
      store5(LR2(g, 0, 0, 0), g.nc, m, ul); store5(LR2(g, 0, 1, 0), g.nc, m, ur); store5(F2(g, 0, 0), g.nc, m, f);
    }
  }
  __syncthreads();
  if (ty > 0) {
#pragma unroll
    for (int v = 0; v < 5; v++) wl[v] = sh[v][ty - 1][lane];
    wl[5] = 0.0;
    face_first(g, wl, wr2, ul, ur, f);
    if (in_i && j >= jl + 1 && j <= ju) {
      store5(LR2(g, 1, 0, 0), g.nc, m, ul); store5(LR2(g, 1, 1, 0), g.nc, m, ur); store5(F2(g, 1, 0), g.nc, m, f);
    }
  }
}

template <int ORD>
__global__ void __launch_bounds__(T2_W*T2_R)
k2d_first(DevGrid g, Real dt, const Real *edge)
{ first_body<ORD>(g, dt, edge); }

// ---- CTU, Steps 5a, 6a and 9a: transverse flux gradients on the face states, then eta1 / eta2 ----------------------------
// a -= h*(fp - fm) for the five fields, with the transverse flux's components permuted into this face's frame
// (x1 faces take (d, Mz, Mx, My, E) of the x2 fluxes, x2 faces (d, My, Mz, Mx, E) of the x1 fluxes)
template <int D>
AA_DEV void correct_state(Real u[6], Real h, const Real fp[6], const Real fm[6])
{
  u[0] -= h*(fp[0] - fm[0]);
  if (D == 0) { u[1] -= h*(fp[3] - fm[3]); u[2] -= h*(fp[1] - fm[1]); u[3] -= h*(fp[2] - fm[2]); }
  else        { u[1] -= h*(fp[2] - fm[2]); u[2] -= h*(fp[3] - fm[3]); u[3] -= h*(fp[1] - fm[1]); }
  u[4] -= h*(fp[4] - fm[4]);
}
AA_DEV void correct_body(const DevGrid &g, Real dt, int hcorr)
{
  const int il = g.is - 2, iu = g.ie + 2, jl = g.js - 2, ju = g.je + 2;
  const int i = g.is + 64*((int)blockIdx.x - 1) + (int)threadIdx.x;
  const int j = jl + 1 + 4*(int)blockIdx.y + (int)threadIdx.y;
  if (i < il + 1 || i > iu || j > ju) return;
  const long m = (long)j*g.sJ + i;
  const Real hdtodx1 = 0.5*(dt/g.dx[0]), hdtodx2 = 0.5*(dt/g.dx[1]);
  Real ul[6], ur[6], fp[6], fm[6];
  if (j <= ju - 1) {                                       // x1 face (j, i)
    load5(LR2(g, 0, 0, 0), g.nc, m, ul); load5(LR2(g, 0, 1, 0), g.nc, m, ur);
    load5(F2(g, 1, 0), g.nc, m + g.sJ - 1, fp); load5(F2(g, 1, 0), g.nc, m - 1, fm);
    correct_state<0>(ul, hdtodx2, fp, fm);
    load5(F2(g, 1, 0), g.nc, m + g.sJ, fp); load5(F2(g, 1, 0), g.nc, m, fm);
    correct_state<0>(ur, hdtodx2, fp, fm);
    store5(LR2(g, 0, 0, 0), g.nc, m, ul); store5(LR2(g, 0, 1, 0), g.nc, m, ur);
    if (j >= g.js - 1 && j <= g.je + 1 && i >= g.is - 1 && i <= g.ie + 2) {
      Real e = 0.0;
      if (hcorr) {
        const Real lambdar = lambda_face(ur, g.Gamma, g.Gamma_1, 1.0), lambdal = lambda_face(ul, g.Gamma, g.Gamma_1, -1.0);
        e = 0.5*fabs(lambdar - lambdal);
      }
      g.eta[m] = e;
    }
  }
  if (i <= iu - 1) {                                       // x2 face (j, i)
    load5(LR2(g, 1, 0, 0), g.nc, m, ul); load5(LR2(g, 1, 1, 0), g.nc, m, ur);
    load5(F2(g, 0, 0), g.nc, m - g.sJ + 1, fp); load5(F2(g, 0, 0), g.nc, m - g.sJ, fm);
    correct_state<1>(ul, hdtodx1, fp, fm);
    load5(F2(g, 0, 0), g.nc, m + 1, fp); load5(F2(g, 0, 0), g.nc, m, fm);
    correct_state<1>(ur, hdtodx1, fp, fm);
    store5(LR2(g, 1, 0, 0), g.nc, m, ul); store5(LR2(g, 1, 1, 0), g.nc, m, ur);
    if (j >= g.js - 1 && j <= g.je + 2 && i >= g.is - 1 && i <= g.ie + 1) {
      Real e = 0.0;
      if (hcorr) {
        const Real lambdar = lambda_face(ur, g.Gamma, g.Gamma_1, 1.0), lambdal = lambda_face(ul, g.Gamma, g.Gamma_1, -1.0);
        e = 0.5*fabs(lambdar - lambdal);
      }
      g.eta[g.nc + m] = e;
    }
  }
}

__global__ void __launch_bounds__(256)
k2d_correct(DevGrid g, Real dt, int hcorr)
{ correct_body(g, dt, hcorr); }

// ---- the flux of the lower face of zone (j, i) along D, in the sweep frame, for the three fused update kernels -----------
enum { M_CTU2 = 0, M_VL1 = 1, M_VL2 = 2 };
template <int MODE, int D, int ORD>
AA_DEV void face_flux(const DevGrid &g, int i, int j, Real dt, Real f[6])
{
  const long m = (long)j*g.sJ + i;
  const long s = D == 0 ? 1L : g.sJ;
  Real ul[6], ur[6], wl[6], wr[6];
  if (MODE == M_CTU2) {
    // Steps 9b / 9c: the largest of the five etas around the face, in the reference's order (MAX as a ternary), then the flux
    const Real *e1 = g.eta, *e2 = g.eta + g.nc;
    Real etah;
    if (D == 0) {
      etah = rmax(e2[m - 1], e2[m]);
      etah = rmax(etah, e2[m + g.sJ - 1]);
      etah = rmax(etah, e2[m + g.sJ]);
      etah = rmax(etah, e1[m]);
    } else {
      etah = rmax(e1[m - g.sJ], e1[m]);
      etah = rmax(etah, e1[m - g.sJ + 1]);
      etah = rmax(etah, e1[m + 1]);
      etah = rmax(etah, e2[m]);
    }
    load5(LR2(g, D, 0, 0), g.nc, m, ul); load5(LR2(g, D, 1, 0), g.nc, m, ur);
    cons_to_prim<0>(ul, wl, g.Gamma_1); cons_to_prim<0>(ur, wr, g.Gamma_1);
    flux_roe<0>(ul, ur, wl, wr, etah, g.Gamma, g.Gamma_1, f);
  } else if (MODE == M_VL1) {
    // integrate_2d_vl.c Steps 1-2: donor cell, through the primitive variables and back as the reference does
    Real u[6];
    load_cons<D>(g.U, g.nc, m - s, u); cons_to_prim<0>(u, wl, g.Gamma_1);
    load_cons<D>(g.U, g.nc, m, u);     cons_to_prim<0>(u, wr, g.Gamma_1);
    face_first(g, wl, wr, ul, ur, f);
  } else {
    // Steps 7-10: PLM / PPM without tracing on U^{n+1/2} (LR fields 0 .. 4), then the flux
    Real dump[6];
    recon_zone<D, false, ORD>(g.LR, g, m - s, dt, wl, dump);
    recon_zone<D, false, ORD>(g.LR, g, m, dt, dump, wr);
    face_first(g, wl, wr, ul, ur, f);
  }
}
template <int MODE> struct Range2 {
  __host__ __device__ static int ext() { return MODE == M_VL1 ? 3 : 0; }      // zones updated: the active ones, or those 3 ghost zones out
  __host__ __device__ static int toff() { return MODE == M_VL1 ? 1 : 0; }     // x1 tiles in front of the one that starts at is
};

// side kernel: the x1 flux of the face above the last lane of every x1 tile
template <int MODE, int ORD>
AA_DEV void edge_body(const DevGrid &g, Real dt, Real *edge, int ntx)
{
  const int X = Range2<MODE>::ext();
  const int lo_j = g.js - X, nj = g.je - g.js + 1 + 2*X, hi_i = g.ie + X;
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= (long)nj*ntx) return;
  const int j = lo_j + (int)(lin % nj), t = (int)(lin / nj);
  const int i = g.is + 64*(t - Range2<MODE>::toff()) + 64;
  if (i < g.is - X + 1 || i > hi_i + 1) return;
  Real f[6];
  face_flux<MODE, 0, ORD>(g, i, j, dt, f);
  const long es = (long)ntx*g.N2;
#pragma unroll
  for (int v = 0; v < 5; v++) edge[v*es + (long)t*g.N2 + j] = f[v];
}

template <int MODE, int ORD>
__global__ void __launch_bounds__(64)
k2d_edge(DevGrid g, Real dt, Real *edge, int ntx)
{ edge_body<MODE, ORD>(g, dt, edge, ntx); }

// new_dt.c:72-140 for one zone (the operands and their order as in the CFL kernel of the 3-D path; never contracted, so that
// the maxima are the same bits whichever kernel visits the zone)
AA_DEV void cfl_zone2(Real d, Real m1, Real m2, Real m3, Real e, Real Gamma, Real Gamma_1, Real mx[2])
{
#pragma clang fp contract(off)
  const Real di = 1.0/d;
  const Real v1 = m1*di, v2 = m2*di, v3 = m3*di;
  const Real qsq = v1*v1 + v2*v2 + v3*v3;
  const Real p = rmax(Gamma_1*(e - 0.5*d*qsq), AA_TINY);
  const Real a = sqrt(Gamma*p*di);
  mx[0] = rmax(mx[0], fabs(v1) + a); mx[1] = rmax(mx[1], fabs(v2) + a);
}

// fluxes of the two lower faces + update of the zone (+ new_dt's maxima): U^{n+1/2} of the van Leer predictor (M_VL1, c = dt/2dx,
// written to LR), the full update of either integrator (c = dt/dx, U in place; x1 differences first, then x2: Steps 12a-b / 13)
// KEEP (a level of a Mesh, csrc/smr.hip): the fluxes of the faces on the lines of `kp` -- the Grid's own boundary and the outline of
// its children -- also go to the flux family F, in the GLOBAL momentum order of the reference's myFlx (integrate_2d_ctu.c:1722-1877:
// x1 faces M1, M2, M3 = Mx, My, Mz; x2 faces Mz, Mx, My).  F is free here: k2d_correct has consumed the first-pass fluxes, and the
// van Leer integrator never uses it.  Every face of [is, ie+1] x [js, je] (x1) and [is, ie] x [js, je+1] (x2) is computed by some
// thread of this launch: the x1 face above a tile's last lane arrives from the tile-edge path and is stored by that lane, and the
// rows the halo wavefront solves for the block above are stored by both (the same bits).
AA_DEV bool on_kept_line(const KeepPlanes &kp, int d, int x)
{
  bool hit = false;
#pragma unroll
  for (int q = 0; q < 8; q++) hit = hit || kp.p[d][q] == x;
  return hit;
}
template <int MODE, bool CFL, bool KEEP, int ORD>
AA_DEV void step_body(const DevGrid &g, Real dt, Real c1, Real c2, const Real *edge, DevScalars *sc, const KeepPlanes *kp)
{
  __shared__ Real sh[5][T2_R][T2_W];
  __shared__ Real red[2][T2_R];
  const int X = Range2<MODE>::ext();
  const int lane = threadIdx.x, ty = threadIdx.y;
  const int lo_i = g.is - X, hi_i = g.ie + X, lo_j = g.js - X, hi_j = g.je + X;
  const int i = g.is + 64*((int)blockIdx.x - Range2<MODE>::toff()) + lane;
  const int j = lo_j + (T2_R - 1)*(int)blockIdx.y + ty;             // ty = T2_R - 1: the halo row above the block's zones
  const int ic = clampi(i, lo_i, hi_i), jc = clampi(j, lo_j, hi_j);
  Real f1[6], f2[6], f1p[6], f2p[6];

  // x2 flux of the lower face: rows lo_j .. hi_j + 1
  face_flux<MODE, 1, ORD>(g, ic, clampi(j, lo_j, hi_j + 1), dt, f2);
#pragma unroll
  for (int v = 0; v < 5; v++) sh[v][ty][lane] = f2[v];
  if (KEEP) {
    if (i >= lo_i && i <= hi_i && j <= hi_j + 1 && on_kept_line(*kp, 1, j)) {
      const long m = (long)j*g.sJ + i;
      F2(g, 1, 0)[m] = f2[0]; F2(g, 1, 1)[m] = f2[3]; F2(g, 1, 2)[m] = f2[1]; F2(g, 1, 3)[m] = f2[2]; F2(g, 1, 4)[m] = f2[4];
    }
  }
  const bool zone = ty < T2_R - 1 && i >= lo_i && i <= hi_i && j <= hi_j;
  if (ty < T2_R - 1) {                                             // (uniform per wavefront)
    face_flux<MODE, 0, ORD>(g, clampi(i, lo_i, hi_i + 1), jc, dt, f1);
#pragma unroll
    for (int v = 0; v < 5; v++) f1p[v] = __shfl_down(f1[v], 1);
    if (lane == 63 && zone) {
      const long es = (long)gridDim.x*g.N2;
#pragma unroll
      for (int v = 0; v < 5; v++) f1p[v] = edge[v*es + (long)blockIdx.x*g.N2 + j];
    }
    if (KEEP) {
      if (j <= hi_j) {
        const long m = (long)j*g.sJ + i;
        if (i >= lo_i && i <= hi_i + 1 && on_kept_line(*kp, 0, i)) store5(F2(g, 0, 0), g.nc, m, f1);
        if (lane == 63 && zone && on_kept_line(*kp, 0, i + 1)) store5(F2(g, 0, 0), g.nc, m + 1, f1p);
      }
    }
  }
  __syncthreads();
  Real mx[2] = {0.0, 0.0};
  if (zone) {
#pragma unroll
    for (int v = 0; v < 5; v++) f2p[v] = sh[v][ty + 1][lane];
    const long m = (long)j*g.sJ + i;
    Real u[5];
#pragma unroll
    for (int v = 0; v < 5; v++) u[v] = U2(g, v)[m];
    u[0] -= c1*(f1p[0] - f1[0]);
    u[1] -= c1*(f1p[1] - f1[1]);
    u[2] -= c1*(f1p[2] - f1[2]);
    u[3] -= c1*(f1p[3] - f1[3]);
    u[4] -= c1*(f1p[4] - f1[4]);
    u[0] -= c2*(f2p[0] - f2[0]);
    u[1] -= c2*(f2p[3] - f2[3]);
    u[2] -= c2*(f2p[1] - f2[1]);
    u[3] -= c2*(f2p[2] - f2[2]);
    u[4] -= c2*(f2p[4] - f2[4]);
    Real *dst = MODE == M_VL1 ? g.LR : g.U;
#pragma unroll
    for (int v = 0; v < 5; v++) dst[(long)v*g.nc + m] = u[v];
    if (CFL) cfl_zone2(u[0], u[1], u[2], u[3], u[4], g.Gamma, g.Gamma_1, mx);
  }
  if (CFL) {
    // (a NaN maximum loses every comparison here and is dropped by the atomic, as in the CFL kernel of the 3-D path)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mx[0] = rmax(mx[0], __shfl_xor(mx[0], o)); mx[1] = rmax(mx[1], __shfl_xor(mx[1], o)); }
    if (lane == 0) { red[0][ty] = mx[0]; red[1][ty] = mx[1]; }
    __syncthreads();
    if (ty == 0 && lane < 2) {
      Real r = red[lane][0];
      for (int q = 1; q < T2_R; q++) r = rmax(r, red[lane][q]);
      if (r == r) atomicMax(&sc->max_v[lane], (unsigned long long)__double_as_longlong(r));
    }
  }
}
// (ORD: of the reconstruction of M_VL2; the other two modes reconstruct nothing and are instantiated at 2 only)
template <int MODE, bool CFL, int ORD>
__global__ void __launch_bounds__(T2_W*T2_R)
k2d_step(DevGrid g, Real dt, Real c1, Real c2, const Real *edge, DevScalars *sc)
{ step_body<MODE, CFL, false, ORD>(g, dt, c1, c2, edge, sc, nullptr); }
template <int MODE, bool CFL, int ORD>
__global__ void __launch_bounds__(T2_W*T2_R)
k2d_step_keep(DevGrid g, Real dt, Real c1, Real c2, const Real *edge, DevScalars *sc, KeepPlanes kp)
{ step_body<MODE, CFL, true, ORD>(g, dt, c1, c2, edge, sc, &kp); }

// ---- the device clock (aa_run_2d; hydro2d_launch.h Run2D) ------------------------------------------------------------------
// dt/dx and dt/2dx of the update kernels (time_step.h dt_over_dx / half_dt_over_dx) are the bits the launch wrappers below form on
// the host for the kernels that take dt as an argument.  (Every other use of dt -- recon_zone, correct_body -- is evaluated on the
// device in either form, by the same code.)
// The *_dc entry points: `live` and dt in one uniform load at the top (the clock is written by k2d_advance / k2d_seed, kernels in
// front of this one on the same stream, and by nobody while this one runs); a step queued behind the stop returns here, before
// any store and before any barrier (the whole grid takes the same branch).
template <int ORD>
__global__ void __launch_bounds__(64)
k2d_edge_wl_dc(DevGrid g, const Run2D *rc, Real *edge, int ntx)
{ if (!rc->c.live) return; edge_wl_body<ORD>(g, rc->c.dt, edge, ntx); }
template <int ORD>
__global__ void __launch_bounds__(T2_W*T2_R)
k2d_first_dc(DevGrid g, const Run2D *rc, const Real *edge)
{ if (!rc->c.live) return; first_body<ORD>(g, rc->c.dt, edge); }
__global__ void __launch_bounds__(256)
k2d_correct_dc(DevGrid g, const Run2D *rc, int hcorr)
{ if (!rc->c.live) return; correct_body(g, rc->c.dt, hcorr); }
template <int MODE, int ORD>
__global__ void __launch_bounds__(64)
k2d_edge_dc(DevGrid g, const Run2D *rc, Real *edge, int ntx)
{ if (!rc->c.live) return; edge_body<MODE, ORD>(g, rc->c.dt, edge, ntx); }
template <int MODE, bool CFL, int ORD>
__global__ void __launch_bounds__(T2_W*T2_R)
k2d_step_dc(DevGrid g, const Run2D *rc, const Real *edge, DevScalars *sc)
{
  if (!rc->c.live) return;
  const Real dt = rc->c.dt;
  const Real c1 = MODE == M_VL1 ? half_dt_over_dx(dt, g.dx[0]) : dt_over_dx(dt, g.dx[0]);
  const Real c2 = MODE == M_VL1 ? half_dt_over_dx(dt, g.dx[1]) : dt_over_dx(dt, g.dx[1]);
  step_body<MODE, CFL, false, ORD>(g, dt, c1, c2, edge, sc, nullptr);
}

// the clock of a call: what aa_run_2d knows on the host, and the maxima zeroed for the first step's update kernel
__global__ void __launch_bounds__(64)
k2d_seed(Run2D *rc, Run2D v, DevScalars *sc)
{
  if (threadIdx.x != 0) return;
  *rc = v;
  sc->max_v[0] = 0ULL; sc->max_v[1] = 0ULL; sc->max_v[2] = 0ULL;
}
// One wavefront behind the update kernel of every step: what aa_step does on the host behind the integrator (main.c:618-629;
// api.hip aa_step, aa_new_dt_local with ndir = 2, aa_new_dt), with the same operations in the same order, none contracted.  The
// boundary pass that follows takes no dt.  Launch rule (as k1d_run states it for itself): a plain launch in stream order; nothing
// here waits for another workgroup or spins on memory, so the launch ends whatever the data are.
__global__ void __launch_bounds__(64)
k2d_advance(Run2D *rc, DevScalars *sc, Real dx0, Real dx1, RunClock *out)
{
  if (threadIdx.x != 0 || !rc->c.live) return;
  RunClock c = rc->c;
  c.nstep++; c.time += c.dt;
  const Real max_v[2] = {__longlong_as_double((long long)sc->max_v[0]), __longlong_as_double((long long)sc->max_v[1])}, dx[2] = {dx0, dx1};
  c.dt = dt_pick(c.nstep, c.dt, dt_courant(rc->cour_no, dt_fold(0.0, max_v, dx, 2)), c.time, rc->tlim);   // new_dt.c:156-185 (time_step.h)
  sc->max_v[0] = 0ULL; sc->max_v[1] = 0ULL; sc->max_v[2] = 0ULL;                               // for the next step's update kernel
  c.live = run_live(c.time, rc->t_stop, c.nstep, rc->nstep_stop, c.dt);                        // (a NaN dt stops too)
  rc->c = c; *out = c;
}

// ---- the Grids of a 2-D Mesh on one clock (aa_mesh_run_2d, csrc/smr.hip) ----------------------------------------------------------
// k2d_step_keep behind the clock load: KeepPlanes stays a by-value argument, c1 and c2 are the bits launch_step_keep forms on the host
template <int MODE, bool CFL, int ORD>
__global__ void __launch_bounds__(T2_W*T2_R)
k2d_step_keep_dc(DevGrid g, const Run2D *rc, const Real *edge, DevScalars *sc, KeepPlanes kp)
{
  if (!rc->c.live) return;
  const Real dt = rc->c.dt;
  step_body<MODE, CFL, true, ORD>(g, dt, dt_over_dx(dt, g.dx[0]), dt_over_dx(dt, g.dx[1]), edge, sc, &kp);
}
// the clock of a call, and new_dt's maxima of every Grid zeroed for the first step (lane l: Grid l)
__global__ void __launch_bounds__(64)
k2d_mesh_seed(Run2D *rc, Run2D v, MeshClockTab tab)
{
  const int l = threadIdx.x;
  if (l == 0) *rc = v;
  if (l < tab.n) { DevScalars *sc = tab.sc[l]; sc->max_v[0] = 0ULL; sc->max_v[1] = 0ULL; sc->max_v[2] = 0ULL; }
}
// One wavefront behind the level coupling of every queued step: what aa_mesh_step does on the host between RestrictCorrect and
// bvals_mhd (main.c:618-629; smr.hip aa_mesh_step, aa_mesh_new_dt) -- the arithmetic is time_step.h run_advance_levels, the
// maxima are those the update kernels (Grids without children) and k_cfl (Grids with children) left in every Grid's DevScalars.
// Lane l reads and zeroes the maxima of Grid l, lane 0 does the rest.  `stepped` tells the kernels queued behind this one whether
// the step in front of it was taken (k2d_box_copy_dc).  Launch rule as k2d_advance: a plain launch in stream order, no waiting.
__global__ void __launch_bounds__(64)
k2d_mesh_advance(Run2D *rc, MeshClockTab tab, RunClock *out)
{
  __shared__ Real mv[2*AA_2D_MESH_GRIDS], dx[2*AA_2D_MESH_GRIDS];
  const int l = threadIdx.x, live = rc->c.live;
  if (!live) { if (l == 0) rc->stepped = 0; return; }        // (uniform: the whole wavefront returns)
  if (l < tab.n) {
    DevScalars *sc = tab.sc[l];
    mv[2*l] = __longlong_as_double((long long)sc->max_v[0]); mv[2*l + 1] = __longlong_as_double((long long)sc->max_v[1]);
    sc->max_v[0] = 0ULL; sc->max_v[1] = 0ULL; sc->max_v[2] = 0ULL;                              // for the next step
    dx[2*l] = tab.dx[2*l]; dx[2*l + 1] = tab.dx[2*l + 1];
  }
  __syncthreads();
  if (l != 0) return;
  RunClock c = rc->c;
  run_advance_levels(&c, rc->t_stop, rc->tlim, rc->cour_no, rc->nstep_stop, tab.n, 2, mv, dx);
  rc->c = c; rc->stepped = 1; *out = c;
}

// ---- launch wrappers -----------------------------------------------------------------------------------------------------
static inline unsigned cdiv(long a, long b) { return (unsigned)((a + b - 1)/b); }

int ntiles_2d(const DevGrid &g) { return 2 + (g.Nx1 + 2)/64; }      // the most x1 tiles any of the kernels below launches

// `order` (2 or 3: the Grid's effective reconstruction order, aa_set_order_2d) picks the instantiation of what reconstructs
void launch_2d_ctu_first(const DevGrid &g, Real dt, Real *edge, int order, hipStream_t st)
{
  const int ntx = 1 + (int)cdiv(g.Nx1 + 2, 64);                     // tile -1 (is-64 .. is-1) and the tiles up to ie+2
  const int nj = g.Nx2 + 4;
  with_ord(order == 3, [&](auto ORD) {
    if (ntx > 1) hipLaunchKernelGGL((k2d_edge_wl<ORD>), dim3(cdiv((long)nj*(ntx - 1), 64)), dim3(64), 0, st, g, dt, edge, ntx);
    hipLaunchKernelGGL((k2d_first<ORD>), dim3(ntx, cdiv(nj, T2_R - 1)), dim3(T2_W, T2_R), 0, st, g, dt, edge);
  });
}
void launch_2d_ctu_first(const DevGrid &g, Real dt, Real *edge, hipStream_t st) { launch_2d_ctu_first(g, dt, edge, 2, st); }
void launch_2d_ctu_correct(const DevGrid &g, Real dt, bool hcorr, hipStream_t st)
{
  const int ntx = 1 + (int)cdiv(g.Nx1 + 2, 64);
  hipLaunchKernelGGL(k2d_correct, dim3(ntx, cdiv(g.Nx2 + 4, 4)), dim3(64, 4), 0, st, g, dt, hcorr ? 1 : 0);
}
template <int MODE, bool CFL, int ORD = 2>
static void launch_step(const DevGrid &g, Real dt, Real c1, Real c2, Real *edge, DevScalars *sc, hipStream_t st)
{
  const int X = Range2<MODE>::ext();
  const int ntx = Range2<MODE>::toff() + (int)cdiv(g.Nx1 + X, 64), nj = g.Nx2 + 2*X;
  hipLaunchKernelGGL((k2d_edge<MODE, ORD>), dim3(cdiv((long)nj*ntx, 64)), dim3(64), 0, st, g, dt, edge, ntx);
  hipLaunchKernelGGL((k2d_step<MODE, CFL, ORD>), dim3(ntx, cdiv(nj, T2_R - 1)), dim3(T2_W, T2_R), 0, st, g, dt, c1, c2, edge, sc);
}
// the keeping form (KEEP above), for the levels of a Mesh; the side kernel is the same
template <int MODE, bool CFL, int ORD = 2>
static void launch_step_keep(const DevGrid &g, Real dt, Real *edge, DevScalars *sc, const KeepPlanes &kp, hipStream_t st)
{
  const int ntx = (int)cdiv(g.Nx1, 64), nj = g.Nx2;
  hipLaunchKernelGGL((k2d_edge<MODE, ORD>), dim3(cdiv((long)nj*ntx, 64)), dim3(64), 0, st, g, dt, edge, ntx);
  hipLaunchKernelGGL((k2d_step_keep<MODE, CFL, ORD>), dim3(ntx, cdiv(nj, T2_R - 1)), dim3(T2_W, T2_R), 0, st, g, dt, dt/g.dx[0], dt/g.dx[1], edge, sc, kp);
}
void launch_2d_ctu_flux2_update_keep(const DevGrid &g, Real dt, Real *edge, DevScalars *sc, const KeepPlanes &kp, hipStream_t st)
{ with_flag(sc != nullptr, [&](auto CFL) { launch_step_keep<M_CTU2, CFL>(g, dt, edge, sc, kp, st); }); }
// (second order only: aa_mesh_create_2d refuses van Leer levels at third order, so the keeping form of VL2 has no ORD = 3 instantiation)
void launch_2d_vl_flux2_update_keep(const DevGrid &g, Real dt, Real *edge, DevScalars *sc, const KeepPlanes &kp, hipStream_t st)
{ with_flag(sc != nullptr, [&](auto CFL) { launch_step_keep<M_VL2, CFL>(g, dt, edge, sc, kp, st); }); }
void launch_2d_ctu_flux2_update(const DevGrid &g, Real dt, Real *edge, DevScalars *sc, hipStream_t st)
{ with_flag(sc != nullptr, [&](auto CFL) { launch_step<M_CTU2, CFL>(g, dt, dt/g.dx[0], dt/g.dx[1], edge, sc, st); }); }
void launch_2d_vl_predict(const DevGrid &g, Real dt, Real *edge, hipStream_t st)
{ launch_step<M_VL1, false>(g, dt, 0.5*(dt/g.dx[0]), 0.5*(dt/g.dx[1]), edge, nullptr, st); }
void launch_2d_vl_flux2_update(const DevGrid &g, Real dt, Real *edge, DevScalars *sc, int order, hipStream_t st)
{ with_flag(sc != nullptr, [&](auto CFL) { with_ord(order == 3, [&](auto ORD) { launch_step<M_VL2, CFL, ORD>(g, dt, dt/g.dx[0], dt/g.dx[1], edge, sc, st); }); }); }
void launch_2d_vl_flux2_update(const DevGrid &g, Real dt, Real *edge, DevScalars *sc, hipStream_t st) { launch_2d_vl_flux2_update(g, dt, edge, sc, 2, st); }

// ---- the same chains on the device clock (aa_run_2d): the launch geometry of the wrappers above, dt from `rc` -------------------
void launch_2d_ctu_first_dc(const DevGrid &g, const Run2D *rc, Real *edge, int order, hipStream_t st)
{
  const int ntx = 1 + (int)cdiv(g.Nx1 + 2, 64);
  const int nj = g.Nx2 + 4;
  with_ord(order == 3, [&](auto ORD) {
    if (ntx > 1) hipLaunchKernelGGL((k2d_edge_wl_dc<ORD>), dim3(cdiv((long)nj*(ntx - 1), 64)), dim3(64), 0, st, g, rc, edge, ntx);
    hipLaunchKernelGGL((k2d_first_dc<ORD>), dim3(ntx, cdiv(nj, T2_R - 1)), dim3(T2_W, T2_R), 0, st, g, rc, edge);
  });
}
void launch_2d_ctu_correct_dc(const DevGrid &g, const Run2D *rc, bool hcorr, hipStream_t st)
{
  const int ntx = 1 + (int)cdiv(g.Nx1 + 2, 64);
  hipLaunchKernelGGL(k2d_correct_dc, dim3(ntx, cdiv(g.Nx2 + 4, 4)), dim3(64, 4), 0, st, g, rc, hcorr ? 1 : 0);
}
template <int MODE, bool CFL, int ORD = 2>
static void launch_step_dc(const DevGrid &g, const Run2D *rc, Real *edge, DevScalars *sc, hipStream_t st)
{
  const int X = Range2<MODE>::ext();
  const int ntx = Range2<MODE>::toff() + (int)cdiv(g.Nx1 + X, 64), nj = g.Nx2 + 2*X;
  hipLaunchKernelGGL((k2d_edge_dc<MODE, ORD>), dim3(cdiv((long)nj*ntx, 64)), dim3(64), 0, st, g, rc, edge, ntx);
  hipLaunchKernelGGL((k2d_step_dc<MODE, CFL, ORD>), dim3(ntx, cdiv(nj, T2_R - 1)), dim3(T2_W, T2_R), 0, st, g, rc, edge, sc);
}
void launch_2d_ctu_flux2_update_dc(const DevGrid &g, const Run2D *rc, Real *edge, DevScalars *sc, hipStream_t st)
{ launch_step_dc<M_CTU2, true>(g, rc, edge, sc, st); }
void launch_2d_vl_predict_dc(const DevGrid &g, const Run2D *rc, Real *edge, hipStream_t st)
{ launch_step_dc<M_VL1, false>(g, rc, edge, nullptr, st); }
void launch_2d_vl_flux2_update_dc(const DevGrid &g, const Run2D *rc, Real *edge, DevScalars *sc, int order, hipStream_t st)
{ with_ord(order == 3, [&](auto ORD) { launch_step_dc<M_VL2, true, ORD>(g, rc, edge, sc, st); }); }
void launch_2d_seed(Run2D *rc, const Run2D &v, DevScalars *sc, hipStream_t st)
{ hipLaunchKernelGGL(k2d_seed, dim3(1), dim3(64), 0, st, rc, v, sc); }
void launch_2d_advance(const DevGrid &g, Run2D *rc, DevScalars *sc, RunClock *out, hipStream_t st)
{ hipLaunchKernelGGL(k2d_advance, dim3(1), dim3(64), 0, st, rc, sc, g.dx[0], g.dx[1], out); }

// ---- the Grids of a 2-D Mesh on one clock (aa_mesh_run_2d): launch_step_keep's geometry, dt from `rc` ----------------------------
template <int MODE, bool CFL, int ORD = 2>
static void launch_step_keep_dc(const DevGrid &g, const Run2D *rc, Real *edge, DevScalars *sc, const KeepPlanes &kp, hipStream_t st)
{
  const int ntx = (int)cdiv(g.Nx1, 64), nj = g.Nx2;
  hipLaunchKernelGGL((k2d_edge_dc<MODE, ORD>), dim3(cdiv((long)nj*ntx, 64)), dim3(64), 0, st, g, rc, edge, ntx);
  hipLaunchKernelGGL((k2d_step_keep_dc<MODE, CFL, ORD>), dim3(ntx, cdiv(nj, T2_R - 1)), dim3(T2_W, T2_R), 0, st, g, rc, edge, sc, kp);
}
void launch_2d_ctu_flux2_update_keep_dc(const DevGrid &g, const Run2D *rc, Real *edge, DevScalars *sc, const KeepPlanes &kp, hipStream_t st)
{ with_flag(sc != nullptr, [&](auto CFL) { launch_step_keep_dc<M_CTU2, CFL>(g, rc, edge, sc, kp, st); }); }
void launch_2d_vl_flux2_update_keep_dc(const DevGrid &g, const Run2D *rc, Real *edge, DevScalars *sc, const KeepPlanes &kp, hipStream_t st)
{ with_flag(sc != nullptr, [&](auto CFL) { launch_step_keep_dc<M_VL2, CFL>(g, rc, edge, sc, kp, st); }); }
void launch_2d_mesh_seed(Run2D *rc, const Run2D &v, const MeshClockTab &tab, hipStream_t st)
{ hipLaunchKernelGGL(k2d_mesh_seed, dim3(1), dim3(64), 0, st, rc, v, tab); }
void launch_2d_mesh_advance(Run2D *rc, const MeshClockTab &tab, RunClock *out, hipStream_t st)
{ hipLaunchKernelGGL(k2d_mesh_advance, dim3(1), dim3(64), 0, st, rc, tab, out); }

}  // namespace aa
