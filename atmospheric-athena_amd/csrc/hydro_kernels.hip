// hydro_kernels.hip -- the 3-D CTU integrator of integrators/integrate_3d_ctu.c as HIP kernels
// for gfx950 (HYDRO / ADIABATIC / CARTESIAN / PLM-characteristic / Roe + H-correction).
//
// Kernel chain of one integrate_3d_ctu() call (reference steps in brackets):
//   sweep<x2>, sweep<x3>, sweep<x1>   [1-3]  prim conversion + PLM/tracing + gravity kick +
//                                            first-pass Roe flux; writes only F of that direction
//   correct_all                       [5-8a,9a] per cell: L/R states re-derived instead of read
//                                            back, transverse flux-gradient corrections, stores the
//                                            corrected Ul,Ur, eta of the faces and d^{n+1/2}
//                                            (small Grids: one tile kernel per direction, x1 fused with
//                                            its first pass)
//   flux2_update                      [9b-d,11a,12] etah = max of 9 etas, second-pass Roe fluxes (kept in
//                                            registers / LDS), gravity source + conservative update of U
//                                            (AA_FUSED_UPDATE=0: flux2<x1..x3> + update through HBM)
// All arrays are struct-of-arrays with i fastest (grid.h); every global access of a wavefront
// is to consecutive i.  The x1 sweep exchanges neighbour cells through LDS; the x2/x3 sweeps
// march a register sliding window along the sweep direction so no cell is converted or
// reconstructed twice.  FP64 vector arithmetic throughout: there is no dense contraction, so
// MFMA is not used.
#include <stdlib.h>
#include "grid.h"
#include "hydro3d_launch.h"
#include "hydro_dev.h"

// Compiled twice: as it stands into namespace aa, and with -DAA_COOLING=1 into namespace aa_cool -- the same kernels with the
// optically thin cooling terms of integrate_3d_ctu.c (Steps 1c-3c :359-368, :662-671, :846-855; 8b :2133-2266; 11c :2943-2953) for the
// cooling function the reference ships (KoyInut, microphysics/cool.c:48).  api.hip launches the second set when a cooling
// function is enrolled (aa_set_cooling); the kernels of every other run do not carry a register or an instruction of it.
#ifndef AA_COOLING
#define AA_COOLING 0
#endif
#if AA_COOLING
namespace aa_cool {
using namespace aa;
#else
namespace aa {
#endif

// ---- field accessors ------------------------------------------------------------------
AA_DEV Real *Uf(const DevGrid &g, int v) { return g.U + (long)v*g.nc; }
AA_DEV Real *LRf(const DevGrid &g, int d, int side, int v) { return g.LR + (long)((d*2 + side)*6 + v)*g.nc; }
AA_DEV Real *Ff(const DevGrid &g, int d, int v) { return g.F + (long)(d*6 + v)*g.nc; }
AA_DEV Real *Ef(const DevGrid &g, int d) { return g.eta + (long)d*g.nc; }
AA_DEV Real *Pf(const DevGrid &g, int which) { return g.phi + (long)which*g.nc; }   // 0 centre, 1+d face
// ---- the same fields as the marching kernels address them: scalar base + one 32-bit zone offset --------
// A field access of a march loop is base + zext(mb) + immediate: `base` a uniform 64-bit byte address in a scalar register pair,
// `mb` the zone's byte offset inside a field as ONE 32-bit unsigned vector register, formed once per iteration, and the +-1 zone
// neighbours in the instruction's immediate.  Everything uniform -- which field (multiples of nc), the +-sJ / +-sK / 2 sK
// neighbours -- is added to the base on the scalar unit, never to the offset.  The strides are made opaque INSIDE the loop body
// (zone_strides), so that a base is formed where it is used, by a running scalar add from the base before it, and the ~60 bases
// of a kernel cannot be hoisted out of the loop and spilled into lanes of vector registers.
// mb < 2^32 for every Grid aa_create accepts (field_offsets_fit, hydro3d_launch.h).
struct ZStr { unsigned nc8, sJ8, sK8; };            // bytes between two fields of a family, two rows, two planes
typedef const char *FBase;                          // a field's base: uniform
AA_DEV ZStr zone_strides(const DevGrid &g)
{
  ZStr z = {(unsigned)g.nc*8u, (unsigned)g.sJ*8u, (unsigned)g.sK*8u};
  asm volatile("" : "+s"(z.nc8), "+s"(z.sJ8), "+s"(z.sK8));
  return z;
}
AA_DEV unsigned zone_off(long m) { unsigned mb = (unsigned)m*8u; asm volatile("" : "+v"(mb)); return mb; }   // zone index -> byte offset
// The instruction takes the 32-bit offset only where the compiler sees its zero-extension in the basic block of the access (it selects
// instructions block by block, and an extension made once at the head of the iteration reaches the other blocks as a 64-bit pair
// and is added to the base by a 64-bit vector add).  So every group of accesses that may sit in a block of its own -- a helper, the
// body of a branch -- starts from its own copy of the offset: one v_mov per group instead of one 64-bit add per access.  (Tied to
// the group's base so that two groups' copies are not merged back into one in front of both.)
AA_DEV unsigned zsite(unsigned mb, FBase b) { asm("" : "+v"(mb) : "s"(b)); return mb; }
AA_DEV FBase fbase(const Real *fam, const ZStr &z, int n) { return (FBase)fam + (unsigned long)z.nc8*(unsigned)n; }   // field n of a family
AA_DEV FBase fnext(FBase b, const ZStr &z) { return b + z.nc8; }                                                      // the field behind b
AA_DEV FBase fup(FBase b, unsigned s) { return b + s; }                                                              // the zone one row / plane up
AA_DEV FBase fdn(FBase b, unsigned s) { return b - s; }
AA_DEV const Real *zp(FBase b, unsigned mb) { return (const Real *)(b + mb); }              // [0], [1], [-1]: the zone and its x1 neighbours
AA_DEV Real *zpw(FBase b, unsigned mb) { return (Real *)(const_cast<char *>(b) + mb); }
AA_DEV void zstore(FBase b, unsigned mb, Real x) { zpw(b, zsite(mb, b))[0] = x; }      // a store that stands alone in its branch
// dt/dx_d and half of it, formed by the launcher (the same IEEE quotient the kernels form): as kernel arguments they live in scalar
// registers; formed in the kernel they took twelve vector registers through the whole march of k_correct_all, six in k_flux2_update
struct StepRatios { Real dtodx[3], q[3]; };
static inline StepRatios step_ratios(const DevGrid &g, Real dt)
{ StepRatios sr; for (int d = 0; d < 3; d++) { sr.dtodx[d] = dt/g.dx[d]; sr.q[d] = 0.5*(dt/g.dx[d]); } return sr; }

#if AA_COOLING
// microphysics/cool.c:48-86 KoyInut(): the cooling rate [erg cm^-3 s^-1] of the diffuse ISM (Koyama & Inutsuka 2002, eq. 4) from
// density and pressure in cgs units, limited so that the temperature stays above its equilibrium value over dt
AA_DEV Real cool_koyinut(Real dens, Real Press, Real dt, Real Gamma_1)
{
  const Real mbar = (1.37)*(1.6733e-24), kb = 1.380658e-16, HeatRate = 2.0e-26, Tmin = 10;
  const Real n = dens/mbar;
  const Real logn = log10(n);
  const Real T = rmax((Press/(n*kb)), Tmin);
  Real Teq = Tmin;
  const Real coolratepp = HeatRate*(n*(1.0e7*exp(-1.184e5/(T+1000.)) + 0.014*sqrt(T)*exp(-92.0/T)) - 1.0);
  const Real dT = coolratepp*dt*Gamma_1/kb;
  if ((T-dT) <= 185.0) {
    const Real lognT = 3.9247499 - 1.8479378*logn + 1.5335032*logn*logn
     -0.47665872*pow(logn,3.0) + 0.076789136*pow(logn,4.0)-0.0049052587*pow(logn,5.0);
    Teq = pow(10.0,lognT) / n;
  }
  const Real MaxdT = kb*(T-Teq)/(dt*Gamma_1);
  return n*rmin(coolratepp,MaxdT);
}
// Steps 1c / 2c / 3c (cont): the L/R primitive states lose pressure over half a step
AA_DEV void cool_states(const DevGrid &g, Real dt, Real wl[6], Real wr[6])
{
  const Real coolfl = cool_koyinut(wl[0], wl[4], (0.5*dt), g.Gamma_1);
  const Real coolfr = cool_koyinut(wr[0], wr[4], (0.5*dt), g.Gamma_1);
  wl[4] -= 0.5*dt*g.Gamma_1*coolfl;
  wr[4] -= 0.5*dt*g.Gamma_1*coolfr;
}
// Step 8b: P^{n+1/2} of zone m from U^n, the first-pass flux differences across the zone (global frame) and, with a static
// potential, q_e (phi_r - phi_l) d
AA_DEV Real p_half(const Real um[3], Real ue, const Real q[3], const Real dF[3][6], bool grav, const Real gm[3], Real dhalf, Real Gamma_1)
{
  Real Mh[3];
#pragma unroll
  for (int e = 0; e < 3; e++) {
    Mh[e] = um[e] - q[0]*dF[0][1 + e] - q[1]*dF[1][1 + e] - q[2]*dF[2][1 + e];
    if (grav) Mh[e] -= gm[e];
  }
  const Real Eh = ue - q[0]*dF[0][4] - q[1]*dF[1][4] - q[2]*dF[2][4];
  Real ph = Eh - 0.5*(Mh[0]*Mh[0] + Mh[1]*Mh[1] + Mh[2]*Mh[2])/dhalf;
  ph *= Gamma_1;
  return ph;
}
#endif

// sweep-frame component n of direction D lives in global field gv<D>(n):
// (Mx,My,Mz) = (M[D], M[D+1], M[D+2])   integrate_3d_ctu.c:206-208, :544-546, :727-729
template <int D> AA_DEV constexpr int gv(int n) { return (n >= 1 && n <= 3) ? 1 + ((D + n - 1) % 3) : n; }
template <int D> AA_DEV long stride(const DevGrid &g) { return D == 0 ? 1L : (D == 1 ? g.sJ : g.sK); }
AA_DEV long stride_rt(const DevGrid &g, int d) { return d == 0 ? 1L : (d == 1 ? g.sJ : g.sK); }

template <int D, int NS>
AA_DEV void load_sweep(const Real *fam, long nc, long m, Real out[6])
{
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) out[n] = fam[(long)gv<D>(n)*nc + m];
  if (!NS) out[5] = 0.0;
}
template <int D, int NS>
AA_DEV void store_sweep(Real *fam, long nc, long m, const Real in[6])
{
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) fam[(long)gv<D>(n)*nc + m] = in[n];
}
// the march loops' form: `fam` the base of field 0 of the family (uniform, any +-sJ / +-sK hop already in it), dz the x1 neighbour;
// the fields are walked in storage order (a running scalar add) and land in the sweep frame by register naming
template <int D> AA_DEV unsigned zstride(const ZStr &z) { return D == 0 ? 8u : (D == 1 ? z.sJ8 : z.sK8); }
template <int D, int NS>
AA_DEV void load_sweep(FBase fam, const ZStr &z, unsigned mb, int dz, Real out[6])
{
  Real t[6];
  mb = zsite(mb, fam);
#pragma unroll
  for (int v = 0; v < 6; v++) { t[v] = (v < 5 + NS) ? zp(fam, mb)[dz] : 0.0; fam = fnext(fam, z); }
#pragma unroll
  for (int n = 0; n < 6; n++) out[n] = t[gv<D>(n)];
}
template <int D, int NS>
AA_DEV void store_sweep(FBase fam, const ZStr &z, unsigned mb, const Real in[6])
{
  Real t[6];
#pragma unroll
  for (int n = 0; n < 6; n++) t[gv<D>(n)] = in[n];
  mb = zsite(mb, fam);
#pragma unroll
  for (int v = 0; v < 5 + NS; v++) { zpw(fam, mb)[0] = t[v]; fam = fnext(fam, z); }
}

// L/R states of one cell: piecewise linear (ORD 2, lr_states_plm.c) or piecewise parabolic (ORD 3,
// lr_states_ppm.c; the slopes of the cell and of its two neighbours along D come from k_slopes)
AA_DEV Real *Sf(const DevGrid &g, int d, int n) { return g.slope + (long)(d*6 + n)*g.nc; }
template <int NS, bool TRACE, int ORD, int D>
AA_DEV void recon_cell(const DevGrid &g, long mcell, const Real wm[6], const Real w[6], const Real wp[6], Real dtodx,
                       Real wl_next[6], Real wr_here[6])
{
  if (ORD == 3) {
    const long s = stride<D>(g);
    Real Dm[6], D0[6], Dp[6];
#pragma unroll
    for (int n = 0; n < 5 + NS; n++) { const Real *q = Sf(g, D, n) + mcell; Dm[n] = q[-s]; D0[n] = q[0]; Dp[n] = q[s]; }
    if (!NS) { Dm[5] = 0.0; D0[5] = 0.0; Dp[5] = 0.0; }
    ppm_cell<NS, TRACE>(wm, w, wp, Dm, D0, Dp, dtodx, g.Gamma, wl_next, wr_here);
  } else plm_cell<NS, TRACE>(wm, w, wp, dtodx, g.Gamma, wl_next, wr_here);
}
// the march loops' form: the cell is zone mb of the fields moved by the uniform byte offset uo
template <int NS, bool TRACE, int ORD, int D>
AA_DEV void recon_cell(const DevGrid &g, const ZStr &z, long uo, unsigned mb, const Real wm[6], const Real w[6], const Real wp[6], Real dtodx,
                       Real wl_next[6], Real wr_here[6])
{
  if (ORD == 3) {
    Real Dm[6], D0[6], Dp[6];
    FBase b = fbase(g.slope, z, D*6) + uo;
#pragma unroll
    for (int n = 0; n < 6; n++) {
      if (n < 5 + NS) {
        D0[n] = zp(b, mb)[0];
        if (D == 0) { Dm[n] = zp(b, mb)[-1]; Dp[n] = zp(b, mb)[1]; }
        else { Dm[n] = zp(fdn(b, zstride<D>(z)), mb)[0]; Dp[n] = zp(fup(b, zstride<D>(z)), mb)[0]; }
        b = fnext(b, z);
      } else { Dm[n] = 0.0; D0[n] = 0.0; Dp[n] = 0.0; }
    }
    ppm_cell<NS, TRACE>(wm, w, wp, Dm, D0, Dp, dtodx, g.Gamma, wl_next, wr_here);
  } else plm_cell<NS, TRACE>(wm, w, wp, dtodx, g.Gamma, wl_next, wr_here);
}

// ---- order 3: monotonised slopes of every cell along D (Steps 1-5 of lr_states_ppm.c) -----------
// cells: along D [s-3, e+3] (a parabola of cell c in [s-2, e+2] needs c-1 and c+1), transverse
// [s-2, e+2] as the sweeps
template <int NS, int D>
__global__ void __launch_bounds__(256)
k_slopes(DevGrid g, const Real *src)
{
  const int lo[3] = {g.is, g.js, g.ks}, hi[3] = {g.ie, g.je, g.ke};
  int n3[3], o3[3];
#pragma unroll
  for (int d = 0; d < 3; d++) { o3[d] = lo[d] - (d == D ? 3 : 2); n3[d] = hi[d] - lo[d] + 1 + (d == D ? 6 : 4); }
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= (long)n3[0]*n3[1]*n3[2]) return;
  const int i = o3[0] + (int)(lin % n3[0]), j = o3[1] + (int)((lin / n3[0]) % n3[1]), k = o3[2] + (int)(lin / ((long)n3[0]*n3[1]));
  const long m = (long)k*g.sK + (long)j*g.sJ + i, s = stride<D>(g);
  Real u[6], wm[6], w[6], wp[6], dWm[6];
  load_sweep<D, NS>(src, g.nc, m - s, u); cons_to_prim<NS>(u, wm, g.Gamma_1);
  load_sweep<D, NS>(src, g.nc, m,     u); cons_to_prim<NS>(u, w,  g.Gamma_1);
  load_sweep<D, NS>(src, g.nc, m + s, u); cons_to_prim<NS>(u, wp, g.Gamma_1);
  limited_slopes<NS>(wm, w, wp, g.Gamma, dWm);
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) Sf(g, D, n)[m] = dWm[n];
}

// What a sweep does at each interface once the L/R primitive states are known.
//   MODE_FLUX1  CTU steps 1c-1d: gravity kick, conversion to conserved, first-pass flux (etah=0);
//               only the flux is stored
//   MODE_CORR   CTU steps 5-7 + 9a: the same L/R states are RE-derived (bit-identical: same code),
//               corrected with the transverse flux gradients (+ gravity), stored, and the
//               H-correction eta of the face is computed.  Recomputing PLM here instead of storing
//               the uncorrected face states in the first pass and reading them back saves
//               2 x 12 doubles of HBM traffic per zone and direction.
//   MODE_VL     integrate_3d_vl.c:751-795: no tracing (done in plm_cell), no kick, flux only
//   MODE_BOTH   FLUX1 and CORR in one pass: used for x1, which runs after the x2/x3 first passes
//               (their fluxes are all its correction needs), saving one x1 reconstruction sweep
enum { MODE_FLUX1 = 0, MODE_CORR = 1, MODE_VL = 2, MODE_BOTH = 3 };

template <int NS, int D, bool GRAV>
AA_DEV void face_correct(const DevGrid &g, long m, int i, int j, int k, Real dt, const Real ul_s[6], const Real ur_s[6])
{
  // ranges (integrate_3d_ctu.c:978, :1282, :1691): along D [s-1, e+2] (the sweep's own range),
  // transverse [s-1, e+1]
  const bool in = (D == 0 || (i >= g.is - 1 && i <= g.ie + 1)) && (D == 1 || (j >= g.js - 1 && j <= g.je + 1)) &&
                  (D == 2 || (k >= g.ks - 1 && k <= g.ke + 1));
  if (!in) return;
  constexpr int NV = 5 + NS;
  const long sD = stride<D>(g), ml = m - sD;
  Real ul[6], ur[6], q[3];
#pragma unroll
  for (int n = 0; n < 6; n++) { ul[gv<D>(n)] = ul_s[n]; ur[gv<D>(n)] = ur_s[n]; }   // to the global frame
#pragma unroll
  for (int d = 0; d < 3; d++) q[d] = 0.5*(dt/g.dx[d]);
#pragma unroll
  for (int e = 0; e < 3; e++) {
    if (e == D) continue;
    const long se = stride_rt(g, e);
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const Real *fe = Ff(g, e, v);
      ul[v] -= q[e]*(fe[ml + se] - fe[ml]);
      ur[v] -= q[e]*(fe[m + se] - fe[m]);
    }
  }
  if (GRAV) {   // :1167-1219, :1463-1526, :1873-1937
    const Real *pc = Pf(g, 0);
    const Real dR = Uf(g, 0)[m], dL = Uf(g, 0)[ml];
    Real phic = pc[m];
#pragma unroll
    for (int e = 0; e < 3; e++) {
      if (e == D) continue;
      const long se = stride_rt(g, e);
      const Real *pfe = Pf(g, 1 + e), *fd = Ff(g, e, 0);
      Real phir = pfe[m + se], phil = pfe[m];
      ur[1 + e] -= q[e]*(phir - phil)*dR;
      ur[4] -= q[e]*(fd[m]*(phic - phil) + fd[m + se]*(phir - phic));
    }
    phic = pc[ml];
#pragma unroll
    for (int e = 0; e < 3; e++) {
      if (e == D) continue;
      const long se = stride_rt(g, e);
      const Real *pfe = Pf(g, 1 + e), *fd = Ff(g, e, 0);
      Real phir = pfe[ml + se], phil = pfe[ml];
      ul[1 + e] -= q[e]*(phir - phil)*dL;
      ul[4] -= q[e]*(fd[ml]*(phic - phil) + fd[ml + se]*(phir - phic));
    }
  }
#pragma unroll
  for (int v = 0; v < NV; v++) { LRf(g, D, 0, v)[m] = ul[v]; LRf(g, D, 1, v)[m] = ur[v]; }
  // eta (integrate_3d_ctu.c:2300-2343), in the sweep frame of D
  Real sl[6], sr[6];
#pragma unroll
  for (int n = 0; n < 6; n++) { sl[n] = ul[gv<D>(n)]; sr[n] = ur[gv<D>(n)]; }
  Real lambdar = lambda_face(sr, g.Gamma, g.Gamma_1, 1.0), lambdal = lambda_face(sl, g.Gamma, g.Gamma_1, -1.0);
  Ef(g, D)[m] = 0.5*fabs(lambdar - lambdal);
  if ((GRAV || AA_COOLING) && D == 1 && j <= g.je + 1) {       // d^{n+1/2}, :2104-2125 (needs all first-pass fluxes:
                                               // done in the x2 correct pass, which runs after them)
    const Real dh = Uf(g, 0)[m]
      - q[0]*(Ff(g, 0, 0)[m + 1]    - Ff(g, 0, 0)[m])
      - q[1]*(Ff(g, 1, 0)[m + g.sJ] - Ff(g, 1, 0)[m])
      - q[2]*(Ff(g, 2, 0)[m + g.sK] - Ff(g, 2, 0)[m]);
    g.dhalf[m] = dh;
#if AA_COOLING
    {   // P^{n+1/2}, :2133-2266
      Real dF[3][6], gm[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int e = 0; e < 3; e++) {
        const long se = stride_rt(g, e);
#pragma unroll
        for (int v = 0; v < 6; v++) dF[e][v] = (v < NV) ? Ff(g, e, v)[m + se] - Ff(g, e, v)[m] : 0.0;
        if (GRAV) gm[e] = q[e]*(Pf(g, 1 + e)[m + se] - Pf(g, 1 + e)[m])*Uf(g, 0)[m];
      }
      const Real um[3] = {Uf(g, 1)[m], Uf(g, 2)[m], Uf(g, 3)[m]};
      g.phalf[m] = p_half(um, Uf(g, 4)[m], q, dF, GRAV, gm, dh, g.Gamma_1);
    }
#endif
  }
}

template <int NS, int D, bool GRAV, int MODE>
AA_DEV void face_work(const DevGrid &g, long m, int i, int j, int k, Real dt, Real wl[6], Real wr[6])
{
  if (GRAV && MODE != MODE_VL) {   // integrate_3d_ctu.c:318-342 (x1), :611-628 (x2), :795-812 (x3)
    const long s = stride<D>(g);
    const Real dtodx = dt/g.dx[D];
    Real phicr = Pf(g, 0)[m], phicl = Pf(g, 0)[m - s], phifc = Pf(g, 1 + D)[m];
    wl[1] -= dtodx*(phifc - phicl);
    wr[1] -= dtodx*(phicr - phifc);
  }
#if AA_COOLING
  if (MODE != MODE_VL) cool_states(g, dt, wl, wr);       // :359-368, :662-671, :846-855 (the van Leer integrator has no such term)
#endif
  Real ul[6], ur[6];
  prim_to_cons<NS>(wl, ul, g.Gamma_1, g.rGamma_1);
  prim_to_cons<NS>(wr, ur, g.Gamma_1, g.rGamma_1);
  if (MODE == MODE_CORR) { face_correct<NS, D, GRAV>(g, m, i, j, k, dt, ul, ur); return; }
  Real f[6];
  flux_roe<NS>(ul, ur, wl, wr, 0.0, g.Gamma, g.Gamma_1, f);
  store_sweep<D, NS>(Ff(g, D, 0), g.nc, m, f);
  if (MODE == MODE_BOTH) face_correct<NS, D, GRAV>(g, m, i, j, k, dt, ul, ur);
}

// the marching sweeps' form (the face is zone mb of the fields: the accessor rule at the top of the file); the correct pass of the
// unfused small-Grid chain keeps its 64-bit zone index m
template <int NS, int D, bool GRAV, int MODE>
AA_DEV void face_work(const DevGrid &g, const ZStr &z, unsigned mb, long m, int i, int j, int k, Real dt, Real wl[6], Real wr[6])
{
  if (GRAV && MODE != MODE_VL) {   // integrate_3d_ctu.c:318-342 (x1), :611-628 (x2), :795-812 (x3)
    const Real dtodx = dt/g.dx[D];
    const FBase pc = (FBase)g.phi, pf = fbase(g.phi, z, 1 + D);
    const unsigned o = zsite(mb, pc);
    Real phicr = zp(pc, o)[0], phicl = (D == 0) ? zp(pc, o)[-1] : zp(fdn(pc, zstride<D>(z)), o)[0], phifc = zp(pf, o)[0];
    wl[1] -= dtodx*(phifc - phicl);
    wr[1] -= dtodx*(phicr - phifc);
  }
#if AA_COOLING
  if (MODE != MODE_VL) cool_states(g, dt, wl, wr);       // :359-368, :662-671, :846-855 (the van Leer integrator has no such term)
#endif
  Real ul[6], ur[6];
  prim_to_cons<NS>(wl, ul, g.Gamma_1, g.rGamma_1);
  prim_to_cons<NS>(wr, ur, g.Gamma_1, g.rGamma_1);
  if (MODE == MODE_CORR) { face_correct<NS, D, GRAV>(g, m, i, j, k, dt, ul, ur); return; }
  Real f[6];
  flux_roe<NS>(ul, ur, wl, wr, 0.0, g.Gamma, g.Gamma_1, f);
  store_sweep<D, NS>(fbase(g.F, z, D*6), z, mb, f);
  if (MODE == MODE_BOTH) face_correct<NS, D, GRAV>(g, m, i, j, k, dt, ul, ur);
}

// Workgroups are dealt round-robin over the 8 XCDs (blockIdx b and b+8 share an XCD and its L2).
// Stencil kernels want NEIGHBOURING rows in the same L2, so give each XCD one contiguous 1/8 of
// the linear cell range: logical block = (b % 8)*per + b/8 with the grid rounded up to 8*per.
AA_DEV long xcd_block(unsigned per) { return (long)(blockIdx.x & 7u)*per + (blockIdx.x >> 3); }

// Zone ordering of the stencil kernels.  `strip` > 0 walks the (i,j,k) box strip-major: j is cut
// into strips of `strip` rows and each strip is traversed k-plane by k-plane, so the distance
// between a zone and its k+-1 neighbours is one strip-plane of all streamed fields (tens of MB:
// resident in the 256 MB Infinity Cache) instead of a full plane (~216 MB at 512^3).
struct Order { int strip; int xcd; };
AA_DEV bool decode_zone(const Order o, int ni, int nj, int nk, int &i, int &j, int &k)
{
  const long lin = (o.xcd ? xcd_block(gridDim.x >> 3) : (long)blockIdx.x)*blockDim.x + threadIdx.x;
  if (lin >= (long)ni*nj*nk) return false;
  if (o.strip <= 0 || o.strip >= nj) {
    i = (int)(lin % ni); j = (int)((lin / ni) % nj); k = (int)(lin / ((long)ni*nj));
    return true;
  }
  const long per_full = (long)ni*o.strip*nk;          // zones in a full strip
  const int s = (int)(lin / per_full);
  const int j0 = s*o.strip;
  const int sj = (j0 + o.strip <= nj) ? o.strip : nj - j0;   // last strip may be thinner
  const long r = lin - (long)s*per_full;
  i = (int)(r % ni); j = j0 + (int)((r / ni) % sj); k = (int)(r / ((long)ni*sj));
  return true;
}

// ---- steps 2,3: x2 / x3 sweeps, register sliding window along the sweep direction ---------
// One thread owns one (i, transverse) column and a chunk of `chunk` interfaces; lanes are
// consecutive in i.  Cells reconstructed: l..u = s-2..e+2; interfaces l+1..u (:179-184).
// (the pool puts zone i = 4 of every row on a 128-byte line when the pitch is a multiple of 16 doubles: api.hip)
__host__ __device__ static inline int march_shift(const DevGrid &g) { return (g.sJ & 15) ? 0 : ((g.is - 2 + 12) & 15); }
__host__ __device__ static inline int march_slots(const DevGrid &g)
{
  const int n = march_shift(g) + g.ie - g.is + 5; return (g.sJ & 15) ? n : ((n + 15) & ~15);
}
__host__ __device__ static inline bool march_cell(const DevGrid &g, int q, int &i)      // slot q of a row -> zone i (false: idle lane)
{
  const int sh = march_shift(g);
  i = g.is - 2 - sh + q;
  return q >= sh && i <= g.ie + 2;
}
// The limited slopes along x2 / x3 as a march (the default; AA_SLOPES_MARCH=0: k_slopes): k_slopes reads and converts three cells per zone, two of them
// in other rows, which at 512^3 come back from HBM for blocks on other XCDs; here a thread owns an (i, transverse) column and a
// chunk of cells along D with the three-cell window in registers (every cell read and converted once, lanes on whole 128-byte
// lines as in k_sweep_march).  ONE inlined instance of the conversion serves every cell, so the values do not depend on where
// the chunks start.  Cells [s-3, e+3] along D, [s-2, e+2] across, as k_slopes.
template <int NS, int D>
__global__ void __launch_bounds__(64)
k_slopes_march(DevGrid g, const Real *src, int chunk)
{
  static_assert(D == 1 || D == 2, "march kernel is for the strided directions");
  const int nq = march_slots(g);
  const int nt = (D == 1 ? g.ke - g.ks : g.je - g.js) + 5;
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= (long)nq*nt) return;
  const int q = (int)(lin % nq);
  int i;
  const int t = (D == 1 ? g.ks : g.js) - 2 + (int)(lin / nq);
  if (!march_cell(g, q, i)) return;
  const int lo = (D == 1 ? g.js : g.ks) - 3, hi = (D == 1 ? g.je : g.ke) + 3;
  const int c0 = lo + blockIdx.y*chunk;
  int c1 = c0 + chunk - 1; if (c1 > hi) c1 = hi;
  if (c0 > c1) return;
  const long s = stride<D>(g);
  const long base = (D == 1) ? ((long)t*g.sK + i) : ((long)t*g.sJ + i);
  Real wm[6], w[6], wp[6], u[6], dW[6];
#pragma unroll
  for (int n = 0; n < 6; n++) { w[n] = 1.0; wp[n] = 1.0; }
#pragma nounroll
  for (int c = c0 - 2; c <= c1; c++) {
    long mc = base + (long)c*s;
    asm volatile("" : "+v"(mc));
#pragma unroll
    for (int n = 0; n < 6; n++) { wm[n] = w[n]; w[n] = wp[n]; }
    load_sweep<D, NS>(src, g.nc, mc + s, u); cons_to_prim<NS>(u, wp, g.Gamma_1);
    if (c >= c0) {
      limited_slopes<NS>(wm, w, wp, g.Gamma, dW);
#pragma unroll
      for (int n = 0; n < 5 + NS; n++) Sf(g, D, n)[mc] = dW[n];
    }
  }
}

#ifndef SW_OCC
#define SW_OCC 3
#endif
// aa_run_3d (csrc/run.hip) queues many steps without the host in between: the four kernels of the default CTU chain that take dt --
// k_sweep_march, k_x1_edge_flux, k_correct_all, k_flux2_update -- have a second entry point, *_dc, which takes dt (and the
// StepRatios) from the device clock (hydro3d_launch.h Run3D) instead of kernel arguments.  Each of the four lives in a header of its
// own that this file compiles twice: as it stands, the entry with by-value arguments, and with AA_CLOCK_ENTRY, the *_dc entry.  One
// text, so the two entries of a kernel have the same body token for token, and the by-value entries are instruction for
// instruction what they were before the second ones existed (profiles/compare_device_asm.py).  A body function shared by two
// __global__ wrappers does not give that: k_correct_all, which sits at the 256-register limit, moved by up to ten registers and
// three instantiations went to scratch; k_sweep_march kept its registers but contracted four other multiply-adds in the default
// build, which changes bits.
#include "sweep_march_kernel.h"
#if !AA_COOLING
#define AA_CLOCK_ENTRY 1
#include "sweep_march_kernel.h"
#undef AA_CLOCK_ENTRY
#endif

// ---- x2 / x3 sweeps on an LDS tile (used for the correct pass) ------------------------------------
// A block of 64 x BT threads owns 64 independent columns (consecutive i) and BT consecutive cells
// of each along the sweep direction; W goes through LDS once ([comp][BT+2][64]: a wavefront reads
// 64 consecutive doubles, conflict-free), neighbours and the Wl hand-off come from LDS, blocks
// overlap by one cell.  One cell per thread keeps the correct pass at ~130 VGPRs (3 waves/SIMD)
// where the marching form needs 255 (1 wave/SIMD, latency-bound: 32 ms instead of 9 at 512^3).
template <int NS, int D, bool GRAV, int MODE, int BT, int ORD>
__global__ void __launch_bounds__(64*BT, 4)
k_sweep_tile(DevGrid g, const Real *src, Real dt)
{
  static_assert(D == 1 || D == 2, "tile kernel is for the strided directions");
  extern __shared__ Real sm[];
  const int lane = threadIdx.x, t = threadIdx.y;
  const int ni = g.ie - g.is + 5;
  const int tlo = (D == 1 ? g.ks : g.js) - 2;
  const int nt  = (D == 1 ? g.ke - g.ks : g.je - g.js) + 5;
  const long colid = (long)blockIdx.x*64 + lane;
  const bool colok = colid < (long)ni*nt;
  const int i = g.is - 2 + (int)(colid % ni);
  const int tt = tlo + (int)(colid / ni);
  const int lo = (D == 1 ? g.js : g.ks), hi = (D == 1 ? g.je : g.ke);
  const int c0 = lo - 2 + blockIdx.y*(BT - 1);
  const int c = c0 + t;
  const long s = stride<D>(g);
  const long base = (D == 1) ? ((long)tt*g.sK + i) : ((long)tt*g.sJ + i);
  const Real dtodx = dt/g.dx[D];
  constexpr int P = (BT + 2)*64;                       // LDS pitch per component
  Real u[6], w[6];
  const bool have = colok && (c <= hi + 3);
  if (have) { load_sweep<D, NS>(src, g.nc, base + (long)c*s, u); cons_to_prim<NS>(u, w, g.Gamma_1); }
  else {
#pragma unroll
    for (int n = 0; n < 6; n++) w[n] = 1.0;
  }
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) sm[n*P + (t + 1)*64 + lane] = w[n];
  if (t == 0 || t == BT - 1) {                         // halo cells c0-1 and c0+BT
    const int ch = (t == 0) ? c0 - 1 : c + 1;
    Real uh[6], wh[6];
    if (colok && ch <= hi + 3) { load_sweep<D, NS>(src, g.nc, base + (long)ch*s, uh); cons_to_prim<NS>(uh, wh, g.Gamma_1); }
    else {
#pragma unroll
      for (int n = 0; n < 6; n++) wh[n] = 1.0;
    }
    const int row = (t == 0) ? 0 : BT + 1;
#pragma unroll
    for (int n = 0; n < 5 + NS; n++) sm[n*P + row*64 + lane] = wh[n];
  }
  __syncthreads();
  Real wm[6], wp[6], wl_next[6], wr[6];
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) { wm[n] = sm[n*P + t*64 + lane]; wp[n] = sm[n*P + (t + 2)*64 + lane]; }
  if (!NS) { wm[5] = 0.0; wp[5] = 0.0; }
  const bool recon = colok && (c <= hi + 2);
  if (recon) recon_cell<NS, MODE != MODE_VL, ORD, D>(g, base + (long)c*s, wm, w, wp, dtodx, wl_next, wr);
  else {
#pragma unroll
    for (int n = 0; n < 6; n++) { wl_next[n] = 1.0; wr[n] = 1.0; }
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) sm[n*P + t*64 + lane] = wl_next[n];
  __syncthreads();
  if (t >= 1 && recon) {
    Real wl[6];
#pragma unroll
    for (int n = 0; n < 5 + NS; n++) wl[n] = sm[n*P + (t - 1)*64 + lane];
    if (!NS) wl[5] = 0.0;
    face_work<NS, D, GRAV, MODE>(g, base + (long)c*s, i, D == 1 ? c : tt, D == 1 ? tt : c, dt, wl, wr);
  }
}

// ---- step 1: x1 sweep, neighbours through LDS ------------------------------------------
// A block of B threads reconstructs B consecutive cells of one (j,k) row and solves the B-1
// interfaces between them; blocks overlap by one cell.
// The x1 sweep with the rows of a k-plane laid end to end (the default; AA_X1_FLAT=0 at run time: k_sweep_x1): a plane's (je-js+5) rows of nc = ie-is+5
// cells l..u are ONE line of slots, cut into blocks of B-1 faces wherever they fall, so that only the plane's last block has
// idle lanes (a block per row piece left 576 lanes for 516 cells at 512^3, 128 for 68 at 64^3).  A row's first cell has no
// face to solve and its lower neighbour is not the slot before it: the lanes at a row's (or the block's) ends fetch and convert
// that one neighbour themselves, everybody else finds it in LDS.  slot -> (row, cell) by a multiply-shift with the host's
// reciprocal (exact below 2^30 slots per plane: launch_sweep checks).
template <int NS, bool GRAV, int MODE, int ORD>
__global__ void __launch_bounds__(256, 4)
k_sweep_x1_flat(DevGrid g, const Real *src, Real dt, int koff, unsigned nslots, unsigned rmul, int rsh)
{
  extern __shared__ Real sm[];
  const int B = blockDim.x, t = threadIdx.x;
  const int nc = g.ie - g.is + 5;                      // cells l..u of a row
  const unsigned s = blockIdx.x*(unsigned)(B - 1) + t;
  const bool have = (s < nslots);
  const unsigned r = have ? (unsigned)(((unsigned long long)s*rmul) >> rsh) : 0u;
  const int ci = have ? (int)(s - r*(unsigned)nc) : 1;
  const int j = g.js - 2 + (int)r, k = g.ks - 2 + koff + blockIdx.y;
  const int c = g.is - 2 + ci;
  const long row = (long)k*g.sK + (long)j*g.sJ;
  const Real dtodx = dt/g.dx[0];
  const bool lo_own = have && (t == 0 || ci == 0);          // the lower / upper neighbour is not in this block's LDS line
  const bool hi_own = have && (t == B - 1 || ci == nc - 1 || s + 1 == nslots);
  Real u[6], w[6], wm[6], wp[6], ulo[6], uhi[6];
  if (have) load_sweep<0, NS>(src, g.nc, row + c, u);
  if (lo_own) load_sweep<0, NS>(src, g.nc, row + c - 1, ulo);
  if (hi_own) load_sweep<0, NS>(src, g.nc, row + c + 1, uhi);
  if (have) cons_to_prim<NS>(u, w, g.Gamma_1);
  else {
#pragma unroll
    for (int n = 0; n < 6; n++) w[n] = 1.0;
  }
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) sm[n*B + t] = w[n];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) { wm[n] = sm[n*B + (t > 0 ? t - 1 : 0)]; wp[n] = sm[n*B + (t < B - 1 ? t + 1 : t)]; }
  if (!NS) { wm[5] = 0.0; wp[5] = 0.0; }
  if (lo_own) cons_to_prim<NS>(ulo, wm, g.Gamma_1);
  if (hi_own) cons_to_prim<NS>(uhi, wp, g.Gamma_1);
  Real wl_next[6], wr[6];
  if (have) recon_cell<NS, MODE != MODE_VL, ORD, 0>(g, row + c, wm, w, wp, dtodx, wl_next, wr);
  else {
#pragma unroll
    for (int n = 0; n < 6; n++) { wl_next[n] = 1.0; wr[n] = 1.0; }
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) sm[n*B + t] = wl_next[n];
  __syncthreads();
  if (t >= 1 && ci >= 1 && have) {                     // interface c, between cells c-1 and c
    Real wl[6];
#pragma unroll
    for (int n = 0; n < 5 + NS; n++) wl[n] = sm[n*B + t - 1];
    if (!NS) wl[5] = 0.0;
    face_work<NS, 0, GRAV, MODE>(g, row + c, c, j, k, dt, wl, wr);
  }
}

template <int NS, bool GRAV, int MODE, int ORD>
__global__ void __launch_bounds__(256, 4)
k_sweep_x1(DevGrid g, const Real *src, Real dt, int koff)
{
  extern __shared__ Real sm[];
  const int B = blockDim.x, t = threadIdx.x;
  const int j = g.js - 2 + blockIdx.y, k = g.ks - 2 + koff + blockIdx.z;
  const int c0 = g.is - 2 + blockIdx.x*(B - 1);
  const int cend = c0 + B - 1;
  const int c = c0 + t;
  const long row = (long)k*g.sK + (long)j*g.sJ;
  const Real dtodx = dt/g.dx[0];
  const int P = B + 2;                                 // LDS pitch per component
  Real u[6], w[6];
  const bool have = (c <= g.ie + 3);                   // cells up to ie+3 feed the stencil
  if (have) { load_sweep<0, NS>(src, g.nc, row + c, u); cons_to_prim<NS>(u, w, g.Gamma_1); }
  else {
#pragma unroll
    for (int n = 0; n < 6; n++) w[n] = 1.0;
  }
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) sm[n*P + t + 1] = w[n];
  if (t == 0) {                                        // lower halo cell c0-1 (>= is-3)
    Real uh[6], wh[6];
    load_sweep<0, NS>(src, g.nc, row + c0 - 1, uh); cons_to_prim<NS>(uh, wh, g.Gamma_1);
#pragma unroll
    for (int n = 0; n < 5 + NS; n++) sm[n*P] = wh[n];
  }
  if (t == B - 1) {                                    // upper halo cell c0+B
    Real uh[6], wh[6];
    if (c + 1 <= g.ie + 3) { load_sweep<0, NS>(src, g.nc, row + c + 1, uh); cons_to_prim<NS>(uh, wh, g.Gamma_1); }
    else {
#pragma unroll
      for (int n = 0; n < 6; n++) wh[n] = 1.0;
    }
#pragma unroll
    for (int n = 0; n < 5 + NS; n++) sm[n*P + B + 1] = wh[n];
  }
  __syncthreads();
  Real wm[6], wp[6], wl_next[6], wr[6];
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) { wm[n] = sm[n*P + t]; wp[n] = sm[n*P + t + 2]; }
  if (!NS) { wm[5] = 0.0; wp[5] = 0.0; }
  const bool recon = (c <= g.ie + 2);                  // cells l..u
  if (recon) recon_cell<NS, MODE != MODE_VL, ORD, 0>(g, row + c, wm, w, wp, dtodx, wl_next, wr);
  else {
#pragma unroll
    for (int n = 0; n < 6; n++) { wl_next[n] = 1.0; wr[n] = 1.0; }
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 5 + NS; n++) sm[n*P + t] = wl_next[n];
  __syncthreads();
  if (t >= 1 && recon && c <= cend) {                  // interface c, between cells c-1 and c
    Real wl[6];
#pragma unroll
    for (int n = 0; n < 5 + NS; n++) wl[n] = sm[n*P + t - 1];
    if (!NS) wl[5] = 0.0;
    face_work<NS, 0, GRAV, MODE>(g, row + c, c, j, k, dt, wl, wr);
  }
}

// ---- steps 5-8a, 9a for all three directions in one marching kernel ---------------------------------
// Per CELL instead of per face: the two face states a cell's reconstruction along D produces (left
// state of its upper face, right state of its lower face) take the SAME transverse correction, the
// first-pass flux differences across that cell (integrate_3d_ctu.c:978-1158, :1282-1452, :1691-1863),
// so a thread that owns a zone loads its six first-pass fluxes per variable once and corrects all six
// face states with them.  A thread owns one (i,j) column and marches along x3 with the primitive
// variables of three planes in registers (the x3 stencil) and the upper x3 flux carried over as the next
// zone's lower one; the x1 neighbours come by wavefront shuffle, the x2 neighbours through LDS.  Only
// eta couples neighbouring zones: eta of a face = 0.5 |lambda_r(right state) - lambda_l(left state)|
// needs one scalar from the zone below (shuffle / LDS / carried).  Against the three separate correct
// passes U and the first-pass fluxes are read once instead of three / two times and no flux plane is
// re-read; lane 0 and row 0 of a block repeat the last lane / row of the block before as providers.
// Every expression is face_correct's, in the same order: bit-identical under -ffp-contract=off.
#ifndef CA_TJ
#define CA_TJ 4
#endif
// Primitive variables of one zone for all three sweeps.  cons_to_prim sums the squared momenta in the
// order of the sweep frame, (Mx^2 + My^2) + Mz^2 with x = D, so the pressure differs in the last bit
// between the frames: w (global frame d, V1, V2, V3, P, r) carries the pressure of the x3 sweep, p0 and
// p1 are the pressures the x1 and x2 sweeps see.
template <int NS>
AA_DEV void prim3(const DevGrid &g, const Real u[6], Real w[6], Real &p0, Real &p1)
{
#if AA_FAST_DIV
  const Real di = q_rcp(u[0]);          // as cons_to_prim: the same bits whichever kernel converts the zone
#else
  const Real di = 1.0/u[0];
#endif
  w[0] = u[0]; w[1] = u[1]*di; w[2] = u[2]*di; w[3] = u[3]*di;
  Real pa = u[4] - 0.5*(sqr(u[1]) + sqr(u[2]) + sqr(u[3]))*di;
  Real pb = u[4] - 0.5*(sqr(u[2]) + sqr(u[3]) + sqr(u[1]))*di;
  Real pc = u[4] - 0.5*(sqr(u[3]) + sqr(u[1]) + sqr(u[2]))*di;
  pa *= g.Gamma_1; pb *= g.Gamma_1; pc *= g.Gamma_1;
  p0 = rmax(pa, AA_TINY); p1 = rmax(pb, AA_TINY); w[4] = rmax(pc, AA_TINY);
  w[5] = NS ? u[5]*di : 0.0;
}
template <int NS>
AA_DEV void load_prim3(const DevGrid &g, long m, Real w[6], Real &p0, Real &p1)
{
  Real u[6];
#pragma unroll
  for (int v = 0; v < 5 + NS; v++) u[v] = Uf(g, v)[m];
  if (!NS) u[5] = 0.0;
  prim3<NS>(g, u, w, p0, p1);
}
template <int NS>
AA_DEV void load_prim3(const DevGrid &g, const ZStr &z, long uo, unsigned mb, Real w[6], Real &p0, Real &p1)
{
  Real u[6];
  FBase b = (FBase)g.U + uo;
  mb = zsite(mb, b);
#pragma unroll
  for (int v = 0; v < 6; v++) { u[v] = (v < 5 + NS) ? zp(b, mb)[0] : 0.0; b = fnext(b, z); }
  prim3<NS>(g, u, w, p0, p1);
}
// sweep-frame primitives of a halo zone, exactly as the sweeps load them
template <int NS, int D>
AA_DEV void load_prim_sweep(const DevGrid &g, const ZStr &z, unsigned mb, int dz, Real w[6])
{
  Real u[6];
  load_sweep<D, NS>((FBase)g.U, z, mb, dz, u);
  cons_to_prim<NS>(u, w, g.Gamma_1);
}
// global frame (d, V1, V2, V3, ., r) with the pressure of frame D -> sweep frame of D
template <int D> AA_DEV void to_sweep(const Real wg[6], Real p, Real ws[6])
{
#pragma unroll
  for (int n = 0; n < 6; n++) ws[n] = wg[gv<D>(n)];
  ws[4] = p;
}

struct CellFlux {            // first-pass fluxes across one zone
  Real dF[3][6];             // F_e(upper face) - F_e(lower face), global frame
  Real gm[3], ge[3];         // gravity: q_e (phi_r - phi_l) d   and   q_e (F_lo (phi_c - phi_l) + F_hi (phi_r - phi_c))
  Real kl[3], kr[3];         // gravity kick of the zone's left / right state along e: dt/dx_e (phi_up - phi_c), dt/dx_e (phi_c - phi_lo)
};

// one zone along D, first half: reconstruction + gravity kick = the primitive states the FIRST pass solves its Riemann
// problems with (face_work): the left state belongs to the zone's upper face, the right state to its lower one
// (the zone is offset mb of the fields moved by the uniform byte offset uo: the accessor rule at the top of the file)
template <int NS, int D, bool GRAV, int ORD>
AA_DEV void cell_recon(const DevGrid &g, const ZStr &z, long uo, unsigned mb, Real dt, Real dtodx, const Real wm[6], const Real w[6], const Real wp[6],
                       Real wl[6], Real wr[6])
{
  if (ORD == 3) mb = zsite(mb, (FBase)g.slope + uo);      // (the slopes' loads: recon_cell itself is called from the head of k_sweep_march's iteration)
  recon_cell<NS, true, ORD, D>(g, z, uo, mb, wm, w, wp, dtodx, wl, wr);
  if (GRAV) {
    const FBase pc = (FBase)g.phi + uo, pf = fbase(g.phi, z, 1 + D) + uo;
    mb = zsite(mb, pc);
    const Real phic = zp(pc, mb)[0], phi_up = (D == 0) ? zp(pf, mb)[1] : zp(fup(pf, zstride<D>(z)), mb)[0], phi_lo = zp(pf, mb)[0];
    wl[1] -= dtodx*(phi_up - phic);
    wr[1] -= dtodx*(phic - phi_lo);
  }
#if AA_COOLING
  cool_states(g, dt, wl, wr);
#endif
}
template <int NS, int D, bool GRAV, int ORD>
AA_DEV void cell_recon(const DevGrid &g, const ZStr &z, long uo, unsigned mb, Real dt, const Real wm[6], const Real w[6], const Real wp[6], Real wl[6], Real wr[6])
{ cell_recon<NS, D, GRAV, ORD>(g, z, uo, mb, dt, dt/g.dx[D], wm, w, wp, wl, wr); }
// the same with the kicks of the zone taken from its CellFlux (formed at the head of the iteration from the potential
// values loaded there: a load inside the direction blocks would wait for the stores of the block before it)
template <int NS, int D, bool GRAV, int ORD>
AA_DEV void cell_recon(const DevGrid &g, const ZStr &z, unsigned mb, Real dt, Real dtodx, const CellFlux &cf, const Real wm[6], const Real w[6], const Real wp[6],
                       Real wl[6], Real wr[6])
{
  if (ORD == 3) mb = zsite(mb, (FBase)g.slope);
  recon_cell<NS, true, ORD, D>(g, z, 0L, mb, wm, w, wp, dtodx, wl, wr);
  if (GRAV) { wl[1] -= cf.kl[D]; wr[1] -= cf.kr[D]; }
#if AA_COOLING
  cool_states(g, dt, wl, wr);
#endif
}
// second half: conversion, transverse correction, face states stored; returns the wave speeds eta needs: lam_l of the
// left state the zone gave to its UPPER face, lam_r of the right state it gave to its LOWER face
template <int NS, int D, bool GRAV>
AA_DEV void cell_finish(const DevGrid &g, const ZStr &z, unsigned mb, const Real q[3], const CellFlux &cf, const Real wl[6], const Real wr[6],
                        bool store, Real &lam_l, Real &lam_r)
{
  constexpr int NV = 5 + NS;
  Real sl[6], sr[6], ul[6], ur[6];
  prim_to_cons<NS>(wl, sl, g.Gamma_1, g.rGamma_1);
  prim_to_cons<NS>(wr, sr, g.Gamma_1, g.rGamma_1);
#pragma unroll
  for (int n = 0; n < 6; n++) { ul[gv<D>(n)] = sl[n]; ur[gv<D>(n)] = sr[n]; }   // to the global frame
#pragma unroll
  for (int e = 0; e < 3; e++) {
    if (e == D) continue;
#pragma unroll
    for (int v = 0; v < NV; v++) { ul[v] -= q[e]*cf.dF[e][v]; ur[v] -= q[e]*cf.dF[e][v]; }
  }
  if (GRAV) {
#pragma unroll
    for (int e = 0; e < 3; e++) {
      if (e == D) continue;
      ur[1 + e] -= cf.gm[e]; ur[4] -= cf.ge[e];
      ul[1 + e] -= cf.gm[e]; ul[4] -= cf.ge[e];
    }
  }
  if (store) {
    // the left state belongs to the zone's upper face: one zone up along D, in the immediate (x1) or on the base (x2, x3)
    FBase bl = fbase(g.LR, z, (D*2)*6), br = fbase(g.LR, z, (D*2 + 1)*6);
    if (D != 0) bl = fup(bl, zstride<D>(z));
    mb = zsite(mb, bl);
#pragma unroll
    for (int v = 0; v < NV; v++) {      // written here, read once by the next kernel: non-temporal
      __builtin_nontemporal_store(ul[v], zpw(bl, mb) + (D == 0 ? 1 : 0)); __builtin_nontemporal_store(ur[v], zpw(br, mb));
      bl = fnext(bl, z); br = fnext(br, z);
    }
  }
#pragma unroll
  for (int n = 0; n < 6; n++) { sl[n] = ul[gv<D>(n)]; sr[n] = ur[gv<D>(n)]; }
  lam_r = lambda_face(sr, g.Gamma, g.Gamma_1, 1.0);
  lam_l = lambda_face(sl, g.Gamma, g.Gamma_1, -1.0);
}
template <int NS, int D, bool GRAV, int ORD>
AA_DEV void cell_states(const DevGrid &g, const ZStr &z, unsigned mb, Real dt, Real dtodx, const Real q[3], const CellFlux &cf, const Real wm[6], const Real w[6],
                        const Real wp[6], bool store, Real &lam_l, Real &lam_r)
{
  Real wl[6], wr[6];
  cell_recon<NS, D, GRAV, ORD>(g, z, mb, dt, dtodx, cf, wm, w, wp, wl, wr);
  cell_finish<NS, D, GRAV>(g, z, mb, q, cf, wl, wr, store, lam_l, lam_r);
}

// With the x3 first pass on board (X3F), k_correct_all also does the x1 FIRST pass: a zone's reconstruction along x1 is the
// same for the first pass and for the correct pass, the right state of its upper face is one lane away, and the first-pass
// fluxes it needs are those of its own two faces.  k_sweep_x1_flat is not launched and its fluxes never reach HBM; what a tile
// of 64 zones cannot do alone, the flux of the face it shares with the next tile, comes from k_x1_edge_flux (1/64 of the faces),
// which keeps its result where the x1 flux array was: [variable][edge][k][j].  Same arithmetic, same bits.
__host__ __device__ static inline int x1_edges(const DevGrid &g) { return (g.ie + 2 - (g.is - 16))/64; }   // edge b = 1 .. : face is-16+64b <= ie+2
AA_DEV long x1_edge_index(const DevGrid &g, int nbe, int v, int b, int j, int k) { return (((long)v*nbe + (b - 1))*g.N3 + k)*g.N2 + j; }
// k_x1_edge_flux and k_correct_all live in correct_all_kernels.h, which is compiled twice: as it stands -- the entries that take dt
// and the StepRatios as kernel arguments -- and with AA_CLOCK_ENTRY, the *_dc entries of a queued step (aa_run_3d), which read both
// from the device clock.  One text, so the two entries of a kernel have the same body token for token, and the by-value entries
// are what they were before the second ones existed (k_correct_all sits at the 256-register limit: as a body function shared by
// two entries its allocation moved by up to ten registers and three instantiations went to scratch).
#if !AA_COOLING
// the clock's ratios by uniform loads (the six doubles behind dt): scalar registers, as the by-value StepRatios
AA_DEV StepRatios clock_ratios(const Run3D *rc)
{
  StepRatios sr;
#pragma unroll
  for (int d = 0; d < 3; d++) { sr.dtodx[d] = rc->dtodx[d]; sr.q[d] = rc->q[d]; }
  return sr;
}
#endif
#include "correct_all_kernels.h"
#if !AA_COOLING
#define AA_CLOCK_ENTRY 1
#include "correct_all_kernels.h"
#undef AA_CLOCK_ENTRY
#endif

// eta of the faces on the tile edges of k_correct_all: the face's slot holds lambda_r of the zone above it, the edge
// array lambda_l of the zone below (same expression as inside the tile: integrate_3d_ctu.c:2300-2343)
template <int D>
AA_DEV void eta_edges(const DevGrid &g)
{
  // faces along D at the tile origins after the first; all zones s-1 .. e+1 of the other two directions
  const int n1 = g.ie - g.is + 3, n2 = g.je - g.js + 3, n3 = g.ke - g.ks + 3;
  const int nb = (D == 0) ? (g.ie + 1 - (g.is - 16))/64 : (g.je + 1 - (g.js - 1))/CA_TJ;      // tile origins 1 .. nb
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  int i, j, k;
  if (D == 0) {
    if (lin >= (long)nb*n2*n3) return;
    i = g.is - 16 + 64*(1 + (int)(lin % nb)); j = g.js - 1 + (int)((lin / nb) % n2); k = g.ks - 1 + (int)(lin / ((long)nb*n2));
  } else {
    if (lin >= (long)n1*nb*n3) return;
    i = g.is - 1 + (int)(lin % n1); j = g.js - 1 + CA_TJ*(1 + (int)((lin / n1) % nb)); k = g.ks - 1 + (int)(lin / ((long)n1*nb));
  }
  if (i > g.ie + 1 || j > g.je + 1) return;
  const ZStr z = zone_strides(g);
  const unsigned mb = zone_off((long)k*g.sK + (long)j*g.sJ + i);
  const FBase e = fbase(g.eta, z, D), el = fbase(g.eta, z, 3 + D);
  const Real lam_l = (D == 0) ? zp(el, mb)[-1] : zp(fdn(el, zstride<D>(z)), mb)[0];
  zpw(e, mb)[0] = 0.5*fabs(zp(e, mb)[0] - lam_l);
}
// both directions in one launch (blockIdx.y; they touch different arrays)
__global__ void __launch_bounds__(256)
k_eta_edges(DevGrid g) { if (blockIdx.y == 0) eta_edges<0>(g); else eta_edges<1>(g); }

// ---- steps 9b-d: second-pass fluxes with the H-correction -----------------------------------
template <int NS, int D>
__global__ void __launch_bounds__(256)
k_flux2(DevGrid g, Order ord)
{
  // faces needed by the update: along D [s, e+1], transverse [s, e]
  const int ni = g.ie - g.is + 1 + (D == 0), nj = g.je - g.js + 1 + (D == 1), nk = g.ke - g.ks + 1 + (D == 2);
  int i, j, k;
  if (!decode_zone(ord, ni, nj, nk, i, j, k)) return;
  i += g.is; j += g.js; k += g.ks;
  const long m = (long)k*g.sK + (long)j*g.sJ + i;
  const long sD = stride<D>(g), ml = m - sD;
  // the reference's MAX chain (a > b ? a : b) visits the two transverse directions in
  // ASCENDING order, then the face's own eta (:2354-2363, :2383-2392, :2412-2421); the order
  // matters when an eta is NaN (negative face pressure)
  constexpr int E1 = (D == 0) ? 1 : 0, E2 = (D == 2) ? 1 : 2;
  const long s1 = stride<E1>(g), s2 = stride<E2>(g);
  const Real *e1 = Ef(g, E1), *e2 = Ef(g, E2);
  Real etah = rmax(e1[ml], e1[m]);
  etah = rmax(etah, e1[ml + s1]);
  etah = rmax(etah, e1[m + s1]);
  etah = rmax(etah, e2[ml]);
  etah = rmax(etah, e2[m]);
  etah = rmax(etah, e2[ml + s2]);
  etah = rmax(etah, e2[m + s2]);
  etah = rmax(etah, Ef(g, D)[m]);
  Real ul[6], ur[6], wl[6], wr[6], f[6];
  load_sweep<D, NS>(LRf(g, D, 0, 0), g.nc, m, ul);
  load_sweep<D, NS>(LRf(g, D, 1, 0), g.nc, m, ur);
  cons_to_prim<NS>(ul, wl, g.Gamma_1);
  cons_to_prim<NS>(ur, wr, g.Gamma_1);
  flux_roe<NS>(ul, ur, wl, wr, etah, g.Gamma, g.Gamma_1, f);
  store_sweep<D, NS>(Ff(g, D, 0), g.nc, m, f);
}

// ---- steps 11a, 12: gravity source and conservative update ---------------------------------
AA_DEV void cfl_zone(Real d, Real m1, Real m2, Real m3, Real e, Real Gamma, Real Gamma_1, Real mx[3]);
AA_DEV void atomic_max_pos(unsigned long long *addr, Real v);
template <int NS, bool GRAV, bool CFL>
__global__ void __launch_bounds__(256)
k_update(DevGrid g, const Real *dhalf, Real dt, Order ord, Real *cfl_part, const unsigned char *pinmask)
{
  // CFL (the van Leer integrator's update; the CTU path has it in k_flux2_update): the zone's contribution to new_dt's maxima from the
  // updated state while it is in registers; one zone per thread makes half a million blocks at 512^3, so a block leaves its three
  // maxima in cfl_part[d][block] (k_cfl_fold turns them into the three words) instead of 1.5 M same-address atomics
  __shared__ Real s_red[CFL ? 3 : 1][CFL ? 256 : 1];
  Real cmx[3] = {0.0, 0.0, 0.0};
  const int ni = g.ie - g.is + 1, nj = g.je - g.js + 1, nk = g.ke - g.ks + 1;
  int i, j, k;
  const bool ok = decode_zone(ord, ni, nj, nk, i, j, k);
  if (!CFL && !ok) return;
  if (ok) {
  i += g.is; j += g.js; k += g.ks;
  const long m = (long)k*g.sK + (long)j*g.sJ + i;
  constexpr int NV = 5 + NS;
  Real u[6];
#pragma unroll
  for (int v = 0; v < NV; v++) u[v] = Uf(g, v)[m];
  Real dtodx[3];
#pragma unroll
  for (int d = 0; d < 3; d++) dtodx[d] = dt/g.dx[d];
  if (GRAV) {   // :2741-2782
    const Real phic = Pf(g, 0)[m], dh = dhalf[m];
#pragma unroll
    for (int e = 0; e < 3; e++) {
      const long se = stride_rt(g, e);
      const Real phir = Pf(g, 1 + e)[m + se], phil = Pf(g, 1 + e)[m];
      const Real *fd = Ff(g, e, 0);
      u[1 + e] -= dtodx[e]*(phir - phil)*dh;
      u[4] -= dtodx[e]*(fd[m]*(phic - phil) + fd[m + se]*(phir - phic));
    }
  }
#if AA_COOLING
  u[4] -= dt*cool_koyinut(dhalf[m], g.phalf[m], dt, g.Gamma_1);      // Step 11c, :2943-2953
#endif
#pragma unroll
  for (int d = 0; d < 3; d++) {   // :2981-3050, x1 then x2 then x3
    const long sd = stride_rt(g, d);
#pragma unroll
    for (int v = 0; v < NV; v++) { const Real *f = Ff(g, d, v); u[v] -= dtodx[d]*(f[m + sd] - f[m]); }
  }
#pragma unroll
  for (int v = 0; v < NV; v++) Uf(g, v)[m] = u[v];
  if (CFL && !(pinmask && pinmask[m])) cfl_zone(u[0], u[1], u[2], u[3], u[4], g.Gamma, g.Gamma_1, cmx);
  }
  if (CFL) {
    const int t = threadIdx.x;
#pragma unroll
    for (int d = 0; d < 3; d++) s_red[CFL ? d : 0][CFL ? t : 0] = cmx[d];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) {
#pragma unroll
        for (int d = 0; d < 3; d++) s_red[CFL ? d : 0][CFL ? t : 0] = rmax(s_red[CFL ? d : 0][CFL ? t : 0], s_red[CFL ? d : 0][CFL ? t + w : 0]);
      }
      __syncthreads();
    }
    if (t < 3) cfl_part[(size_t)t*gridDim.x + blockIdx.x] = s_red[CFL ? t : 0][0];
  }
}

#if !AA_COOLING
// k_update of the van Leer integrator with the detection half of the first-order flux correction (aa_set_fofc) on board -- the
// update itself is k_update's, line for line but for the cooling term the van Leer integrator does not have (a kernel of its own, so that k_update stays the code it was): a zone whose new
// density is negative goes onto the candidate list of Step 14 (one ballot and one vector atomic per wavefront that has any; the
// order of the list is whatever the atomics make it: k_fofc_fix sorts), and a NaN among the second-order fluxes the zone read
// raises sc->fofc_nanseen (Step 10 is then made up for: api.hip fofc_finish).
template <int NS, bool GRAV, bool CFL>
__global__ void __launch_bounds__(256)
k_update_fofc(DevGrid g, const Real *dhalf, Real dt, Order ord, Real *cfl_part, const unsigned char *pinmask, DevScalars *sc, long long *list)
{
  // CFL (the van Leer integrator's update; the CTU path has it in k_flux2_update): the zone's contribution to new_dt's maxima from the
  // updated state while it is in registers; one zone per thread makes half a million blocks at 512^3, so a block leaves its three
  // maxima in cfl_part[d][block] (k_cfl_fold turns them into the three words) instead of 1.5 M same-address atomics
  __shared__ Real s_red[CFL ? 3 : 1][CFL ? 256 : 1];
  Real cmx[3] = {0.0, 0.0, 0.0};
  const int ni = g.ie - g.is + 1, nj = g.je - g.js + 1, nk = g.ke - g.ks + 1;
  int i, j, k;
  const bool ok = decode_zone(ord, ni, nj, nk, i, j, k);
  bool bad = false, nanf = false;
  long mbad = 0;
  if (ok) {
  i += g.is; j += g.js; k += g.ks;
  const long m = (long)k*g.sK + (long)j*g.sJ + i;
  constexpr int NV = 5 + NS;
  Real u[6];
#pragma unroll
  for (int v = 0; v < NV; v++) u[v] = Uf(g, v)[m];
  Real dtodx[3];
#pragma unroll
  for (int d = 0; d < 3; d++) dtodx[d] = dt/g.dx[d];
  if (GRAV) {   // :2741-2782
    const Real phic = Pf(g, 0)[m], dh = dhalf[m];
#pragma unroll
    for (int e = 0; e < 3; e++) {
      const long se = stride_rt(g, e);
      const Real phir = Pf(g, 1 + e)[m + se], phil = Pf(g, 1 + e)[m];
      const Real *fd = Ff(g, e, 0);
      u[1 + e] -= dtodx[e]*(phir - phil)*dh;
      u[4] -= dtodx[e]*(fd[m]*(phic - phil) + fd[m + se]*(phir - phic));
    }
  }
#pragma unroll
  for (int d = 0; d < 3; d++) {   // :2981-3050, x1 then x2 then x3
    const long sd = stride_rt(g, d);
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const Real *f = Ff(g, d, v);
      if (v < 5) { const Real fh = f[m + sd], fl = f[m]; nanf = nanf || (fh != fh) || (fl != fl); }      // (the scalar flux is not part of the reference's test)
      u[v] -= dtodx[d]*(f[m + sd] - f[m]);
    }
  }
#pragma unroll
  for (int v = 0; v < NV; v++) Uf(g, v)[m] = u[v];
  if (CFL && !(pinmask && pinmask[m])) cfl_zone(u[0], u[1], u[2], u[3], u[4], g.Gamma, g.Gamma_1, cmx);
  bad = u[0] < 0.0; mbad = m;
  }
  {
    const int lane = __lane_id();
    const unsigned long long b = __ballot(bad);
    if (b) {
      const int first = __ffsll((long long)b) - 1;
      int base = 0;
      if (lane == first) base = atomicAdd(&sc->fofc_n, __popcll(b));
      base = __shfl(base, first);
      const int pos = base + __popcll(b & ((1ULL << lane) - 1ULL));
      if (bad && pos < AA_FOFC_MAX) list[pos] = mbad;          // (beyond the list only the count goes on: the caller fails the step)
    }
    const unsigned long long bn = __ballot(nanf);
    if (bn && lane == __ffsll((long long)bn) - 1) atomicAdd(&sc->fofc_nanseen, 1);
  }
  if (CFL) {
    const int t = threadIdx.x;
#pragma unroll
    for (int d = 0; d < 3; d++) s_red[CFL ? d : 0][CFL ? t : 0] = cmx[d];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) {
#pragma unroll
        for (int d = 0; d < 3; d++) s_red[CFL ? d : 0][CFL ? t : 0] = rmax(s_red[CFL ? d : 0][CFL ? t : 0], s_red[CFL ? d : 0][CFL ? t + w : 0]);
      }
      __syncthreads();
    }
    if (t < 3) cfl_part[(size_t)t*gridDim.x + blockIdx.x] = s_red[CFL ? t : 0][0];
  }
}
#endif

// the blocks' maxima of k_update<CFL> -> the three words of new_dt (MAX of non-negative doubles on their bit patterns: order-free)
__global__ void __launch_bounds__(256)
k_cfl_fold(const Real *part, int nb, DevScalars *sc)
{
  __shared__ Real red[3][256];
  Real mx[3] = {0.0, 0.0, 0.0};
  for (int b = blockIdx.x*256 + threadIdx.x; b < nb; b += gridDim.x*256) {
#pragma unroll
    for (int d = 0; d < 3; d++) mx[d] = rmax(mx[d], part[(size_t)d*nb + b]);
  }
#pragma unroll
  for (int d = 0; d < 3; d++) red[d][threadIdx.x] = mx[d];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int d = 0; d < 3; d++) red[d][threadIdx.x] = rmax(red[d][threadIdx.x], red[d][threadIdx.x + w]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) atomic_max_pos(&sc->max_v[threadIdx.x], red[threadIdx.x][0]);
}

// ---- steps 9b-d + 11a + 12 in one marching kernel --------------------------------------------
// The second-pass fluxes never go to HBM: a thread owns one (i,j) column and marches along x3; at every
// zone it solves the Riemann problems of the zone's LOWER x1 and x2 faces and of its UPPER x3 face.
// The upper x1 (x2) face is the lower face of the next lane (row) and arrives by a wavefront shuffle
// (through LDS); the lower x3 face is the upper one of the previous step and stays in registers.  Lane 63
// and row FU_TJ-1 of a block only provide fluxes (63 x 7 zones per 64 x 8 threads: 16 % more Riemann
// solves than faces), and a chunk of `kchunk` zones starts with one extra x3 solve.  Against
// k_flux2 x3 + k_update this drops 18 stores and ~20 loads of doubles per zone.  Expressions and their
// order per zone are those of k_flux2 / k_update, so results are bit-identical to the unfused chain.
// Levels of a Mesh (KEEP): RestrictCorrect reads the second-pass fluxes on the level boundaries, so the
// faces on those planes (KeepPlanes: a few planes per direction) are stored as well.
#ifndef FU_TJ
#define FU_TJ 8
#endif
// operands of one second-pass Riemann problem: the corrected face states (sweep frame) and the 9 etas
struct FaceIn { Real ul[6], ur[6], eta[9]; };
// eta of direction E beside the face along D of zone mb: of the zone below the face (lo) or above it, at its lower face along E or
// (up) at its upper one -- the hops along x1 in the immediate, those along x2 / x3 on the base
template <int D, int E>
AA_DEV Real eta_at(FBase e, const ZStr &z, unsigned mb, bool lo, bool up)
{
  int dz = 0;
  if (lo) { if (D == 0) dz -= 1; else e = fdn(e, zstride<D>(z)); }
  if (up) { if (E == 0) dz += 1; else e = fup(e, zstride<E>(z)); }
  return zp(e, mb)[dz];
}
// (the face is zone mb of the fields moved by the uniform byte offset uo: the accessor rule at the top of the file)
template <int NS, int D>
AA_DEV void face_load(const DevGrid &g, const ZStr &z, long uo, unsigned mb, FaceIn &in)
{
  constexpr int E1 = (D == 0) ? 1 : 0, E2 = (D == 2) ? 1 : 2;
  const FBase e1 = fbase(g.eta, z, E1) + uo, e2 = fbase(g.eta, z, E2) + uo, eD = fbase(g.eta, z, D) + uo;
  const unsigned o = zsite(mb, eD);
  in.eta[8] = zp(eD, o)[0];
  in.eta[0] = eta_at<D, E1>(e1, z, o, true, false); in.eta[1] = eta_at<D, E1>(e1, z, o, false, false);
  in.eta[2] = eta_at<D, E1>(e1, z, o, true, true);  in.eta[3] = eta_at<D, E1>(e1, z, o, false, true);
  in.eta[4] = eta_at<D, E2>(e2, z, o, true, false); in.eta[5] = eta_at<D, E2>(e2, z, o, false, false);
  in.eta[6] = eta_at<D, E2>(e2, z, o, true, true);  in.eta[7] = eta_at<D, E2>(e2, z, o, false, true);
  load_sweep<D, NS>(fbase(g.LR, z, (D*2)*6) + uo, z, mb, 0, in.ul);
  load_sweep<D, NS>(fbase(g.LR, z, (D*2 + 1)*6) + uo, z, mb, 0, in.ur);
}
template <int NS>
AA_DEV void face_solve(const DevGrid &g, const FaceIn &in, Real f[6])
{
  Real etah = rmax(in.eta[0], in.eta[1]);
#pragma unroll
  for (int n = 2; n < 9; n++) etah = rmax(etah, in.eta[n]);
  Real wl[6], wr[6];
  cons_to_prim<NS>(in.ul, wl, g.Gamma_1);
  cons_to_prim<NS>(in.ur, wr, g.Gamma_1);
  flux_roe<NS>(in.ul, in.ur, wl, wr, etah, g.Gamma, g.Gamma_1, f);      // (the scaling-free quotients pay here since the x3 flux is parked in LDS: k_flux2_update)
}
template <int NS, int D>
AA_DEV void face_flux2(const DevGrid &g, const ZStr &z, unsigned mb, Real f[6])
{
  FaceIn in;
  face_load<NS, D>(g, z, 0L, mb, in);
  face_solve<NS>(g, in, f);
}

// new_dt.c:72-140 for one zone: max(|v_d| + a) per direction (the operands and their order as in k_cfl)
// (no multiply-add contraction in here, in either build: the same zone must give the same bits whether it is visited by
//  k_cfl, by k_pinned_cfl or inside the update kernel, so that AA_CFL_FUSED changes no bit of dt in the default build either)
AA_DEV void cfl_zone(Real d, Real m1, Real m2, Real m3, Real e, Real Gamma, Real Gamma_1, Real mx[3])
{
#pragma clang fp contract(off)
  const Real di = 1.0/d;
  const Real v1 = m1*di, v2 = m2*di, v3 = m3*di;
  const Real qsq = v1*v1 + v2*v2 + v3*v3;
  const Real p = rmax(Gamma_1*(e - 0.5*d*qsq), AA_TINY);
  const Real a = sqrt(Gamma*p*di);
  mx[0] = rmax(mx[0], fabs(v1) + a); mx[1] = rmax(mx[1], fabs(v2) + a); mx[2] = rmax(mx[2], fabs(v3) + a);
}
AA_DEV void atomic_max_pos(unsigned long long *addr, Real v)
{ if (v == v) atomicMax(addr, (unsigned long long)__double_as_longlong(v)); }   // v >= 0; NaN skipped

AA_DEV bool on_plane(const KeepPlanes &kp, int d, int x)
{
  return x == kp.p[d][0] || x == kp.p[d][1] || x == kp.p[d][2] || x == kp.p[d][3] ||
         x == kp.p[d][4] || x == kp.p[d][5] || x == kp.p[d][6] || x == kp.p[d][7];
}

// CFL: the zone's contribution to new_dt's maxima is taken from the updated state while it is in registers (k_cfl would
// read the five fields again: 0.9 ms at 512^3); zones marked in `pinmask` are left out, the caller adds them after it
// has overwritten them (k_pinned_cfl).
#include "flux2_update_kernel.h"
#if !AA_COOLING
#define AA_CLOCK_ENTRY 1
#include "flux2_update_kernel.h"      // (k_flux2_update_dc: instantiated without kept planes, with new_dt's maxima)
#undef AA_CLOCK_ENTRY
#define AA_CLOCK_ENTRY 2
#include "flux2_update_kernel.h"      // (k_flux2_update_keep_dc: a level of a Mesh -- kept planes, with or without the maxima)
#undef AA_CLOCK_ENTRY
#endif

// the zones Userwork has just overwritten (k_pinned) join the maxima k_flux2_update<CFL> left them out of
__global__ void k_pinned_cfl(DevGrid g, long long n, const long long *idx, DevScalars *sc)
{
  // grid-stride: a few hundred same-address atomics per launch instead of one per 64 pinned zones (1.5e5 zones at 512^3 made
  // 7000 atomics on three words, ~0.1 ms of this kernel's 0.13; the MAX is order-free)
  Real mx[3] = {0.0, 0.0, 0.0};
  for (long lin = (long)blockIdx.x*blockDim.x + threadIdx.x; lin < n; lin += (long)gridDim.x*blockDim.x) {
    const long long c = idx[lin];
    const int i = (int)(c % g.N1), j = (int)((c / g.N1) % g.N2), k = (int)(c / ((long)g.N1*g.N2));
    if (i >= g.is && i <= g.ie && j >= g.js && j <= g.je && k >= g.ks && k <= g.ke) {      // new_dt looks at active zones only
      const long m = (long)k*g.sK + (long)j*g.sJ + i;
      cfl_zone(Uf(g, 0)[m], Uf(g, 1)[m], Uf(g, 2)[m], Uf(g, 3)[m], Uf(g, 4)[m], g.Gamma, g.Gamma_1, mx);
    }
  }
  // one atomic per wavefront and direction (NaN maxima are dropped by atomic_max_pos, as in k_cfl)
#pragma unroll
  for (int d = 0; d < 3; d++) {
    Real v = mx[d];
    for (int o = 32; o > 0; o >>= 1) { const Real w = __shfl_xor(v, o); v = (w > v || v != v) ? w : v; }
    if ((threadIdx.x & 63) == 0) atomic_max_pos(&sc->max_v[d], v);
  }
}
// byte mask of the pinned zones over the device array
__global__ void k_pin_mask(DevGrid g, long long n, const long long *idx, unsigned char *mask)
{
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= n) return;
  const long long c = idx[lin];
  const int i = (int)(c % g.N1), j = (int)((c / g.N1) % g.N2), k = (int)(c / ((long)g.N1*g.N2));
  mask[(long)k*g.sK + (long)j*g.sJ + i] = 1;
}

// ---- van Leer integrator (integrators/integrate_3d_vl.c, NO_H_CORRECTION) --------------------
// Predictor on small Grids: k_vl_flux1 x3 + k_vl_uhalf below; on big ones k_vl_predict further down does both.
// steps 1-3: first-order (donor-cell) fluxes, Wl = W[c-1], Wr = W[c], over the whole ghost range
template <int NS, int D>
__global__ void __launch_bounds__(256)
k_vl_flux1(DevGrid g)
{
  // faces along D: [s-3, e+4]; transverse: all zones incl. ghosts (:153-305)
  const int N[3] = {g.N1, g.N2, g.N3};
  int n[3] = {N[0], N[1], N[2]};
  n[D] = N[D] - 1;                                         // faces 1 .. N-1  (= s-3 .. e+4)
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= (long)n[0]*n[1]*n[2]) return;
  int idx[3];
  idx[0] = (int)(lin % n[0]); idx[1] = (int)((lin / n[0]) % n[1]); idx[2] = (int)(lin / ((long)n[0]*n[1]));
  idx[D] += 1;
  const long m = (long)idx[2]*g.sK + (long)idx[1]*g.sJ + idx[0];
  const long s = stride<D>(g);
  Real u[6], wl[6], wr[6], ul[6], ur[6], f[6];
  load_sweep<D, NS>(g.U, g.nc, m - s, u); cons_to_prim<NS>(u, wl, g.Gamma_1);
  load_sweep<D, NS>(g.U, g.nc, m, u);     cons_to_prim<NS>(u, wr, g.Gamma_1);
  prim_to_cons<NS>(wl, ul, g.Gamma_1, g.rGamma_1);                     // the reference round-trips through W (:166-169)
  prim_to_cons<NS>(wr, ur, g.Gamma_1, g.rGamma_1);
  flux_roe<NS>(ul, ur, wl, wr, 0.0, g.Gamma, g.Gamma_1, f);
  store_sweep<D, NS>(Ff(g, D, 0), g.nc, m, f);
}

// steps 5-6: U^{n+1/2} over [s-3, e+3]^3 (x1, x2, x3 flux differences in that order, then the
// gravity predictor); stored in the first six face-state arrays
// ---- van Leer predictor in one marching kernel: donor-cell fluxes + U^{n+1/2} (integrate_3d_vl.c:153-510) --
// The first-order fluxes only feed U^{n+1/2}, so they never go to HBM: thread = (i,j) column marching along
// x3 as in k_flux2_update.  The state of a zone is converted once for all three sweeps: d, V and r are the
// same in every frame, the pressure (cons_to_prim) and the round-tripped energy (prim_to_cons, the reference
// converts W back to U, :166-169) sum the squared velocities in sweep-frame order, so both come in three
// variants.  The lower x1 face takes its left state from the previous lane (shuffle), the lower x2 face
// from the row below (loaded), the lower x3 face from the previous step (registers); the upper fluxes come
// from the next lane / row / step.  Lane 63 and row VP_TJ-1 only provide fluxes.
#ifndef VP_TJ
#define VP_TJ 8
#endif
struct VlState { Real w[6], p[3], e[3]; };       // w: d, V1, V2, V3, (unused), r;  p, e per sweep frame
template <int NS>
AA_DEV void vl_state(const DevGrid &g, long m, VlState &q)
{
  Real u[6];
#pragma unroll
  for (int v = 0; v < 5 + NS; v++) u[v] = Uf(g, v)[m];
  if (!NS) u[5] = 0.0;
#pragma unroll
  for (int D = 0; D < 3; D++) {
    // exactly cons_to_prim / prim_to_cons on the state rotated into the frame of D
    Real us[6], ws[6], ub[6];
    us[0] = u[0]; us[1] = u[1 + D]; us[2] = u[1 + (D + 1) % 3]; us[3] = u[1 + (D + 2) % 3]; us[4] = u[4]; us[5] = u[5];
    cons_to_prim<NS>(us, ws, g.Gamma_1);
    prim_to_cons<NS>(ws, ub, g.Gamma_1, g.rGamma_1);
    q.p[D] = ws[4]; q.e[D] = ub[4];
    if (D == 0) { q.w[0] = ws[0]; q.w[1] = ws[1]; q.w[2] = ws[2]; q.w[3] = ws[3]; q.w[4] = 0.0; q.w[5] = ws[5]; }
  }
}
// sweep-frame primitive and (round-tripped) conserved state of direction D
template <int NS, int D>
AA_DEV void vl_rotate(const VlState &q, Real w[6], Real u[6])
{
  w[0] = q.w[0]; w[1] = q.w[1 + D]; w[2] = q.w[1 + (D + 1) % 3]; w[3] = q.w[1 + (D + 2) % 3]; w[4] = q.p[D]; w[5] = q.w[5];
  u[0] = w[0]; u[1] = w[0]*w[1]; u[2] = w[0]*w[2]; u[3] = w[0]*w[3]; u[4] = q.e[D]; u[5] = NS ? w[5]*w[0] : 0.0;
}
template <int NS, int D>
AA_DEV void vl_face(const DevGrid &g, const VlState &lo, const VlState &hi, Real f[6])
{
  Real wl[6], wr[6], ul[6], ur[6];
  vl_rotate<NS, D>(lo, wl, ul);
  vl_rotate<NS, D>(hi, wr, ur);
  flux_roe<NS>(ul, ur, wl, wr, 0.0, g.Gamma, g.Gamma_1, f);
}

template <int NS, bool GRAV>
__global__ void __launch_bounds__(64*VP_TJ)
k_vl_predict(DevGrid g, Real dt, int kchunk)
{
  __shared__ Real s_f2[VP_TJ][6][64];
  constexpr int NV = 5 + NS;
  const int lane = threadIdx.x, row = threadIdx.y;
  const int lo[3] = {g.is - 3, g.js - 3, g.ks - 3}, hi[3] = {g.ie + 3, g.je + 3, g.ke + 3};   // zones that get U^{n+1/2}
  const int i = lo[0] + blockIdx.x*63 + lane, j = lo[1] + blockIdx.y*(VP_TJ - 1) + row;
  const int k0 = lo[2] + blockIdx.z*kchunk;
  int k1 = k0 + kchunk - 1; if (k1 > hi[2]) k1 = hi[2];
  const bool cell = (lane < 63) && (row < VP_TJ - 1) && (i <= hi[0]) && (j <= hi[1]);
  const bool need1 = (row < VP_TJ - 1) && (j <= hi[1]) && (i <= hi[0] + 1);      // lower x1 face of (i,j)
  const bool need2 = (lane < 63) && (i <= hi[0]) && (j <= hi[1] + 1);            // lower x2 face of (i,j)
  const int ic = (i <= hi[0] + 1) ? i : hi[0] + 1, jc = (j <= hi[1] + 1) ? j : hi[1] + 1;
  const long mcol = (long)jc*g.sJ + ic;
  Real q[3];
#pragma unroll
  for (int d = 0; d < 3; d++) q[d] = 0.5*(dt/g.dx[d]);
  VlState below, here;
  Real f3lo[6];
#pragma unroll
  for (int n = 0; n < 6; n++) f3lo[n] = 0.0;
  vl_state<NS>(g, (long)(k0 - 1)*g.sK + mcol, below);
  vl_state<NS>(g, (long)k0*g.sK + mcol, here);
  if (cell) vl_face<NS, 2>(g, below, here, f3lo);                                // face k0
  for (int k = k0; k <= k1; k++) {
    long m = (long)k*g.sK + mcol;
    asm volatile("" : "+v"(m));                   // one index for all fields (see k_flux2_update)
    VlState above;
    vl_state<NS>(g, m + g.sK, above);
    Real d1[6], d2[6], d3[6], m1lo, m1hi, m2lo, m2hi = 0.0, m3lo, m3hi;
#pragma unroll
    for (int n = 0; n < 6; n++) d2[n] = 0.0;
    __builtin_amdgcn_sched_barrier(0);
    {   // ---- x1: left state from the previous lane ----
      VlState left;
#pragma unroll
      for (int n = 0; n < 6; n++) left.w[n] = __shfl_up(here.w[n], 1);
      left.p[0] = __shfl_up(here.p[0], 1); left.e[0] = __shfl_up(here.e[0], 1);
      left.p[1] = left.p[2] = left.e[1] = left.e[2] = 0.0;
      if (lane == 0) vl_state<NS>(g, m - 1, left);
      Real f[6];
#pragma unroll
      for (int n = 0; n < 6; n++) f[n] = 0.0;
      if (need1) vl_face<NS, 0>(g, left, here, f);
#pragma unroll
      for (int n = 0; n < NV; n++) d1[n] = __shfl_down(f[n], 1) - f[n];
      m1lo = f[0]; m1hi = __shfl_down(f[0], 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    {   // ---- x2: left state = the zone of the row below (converted here: it is in L1/L2) ----
      VlState left;
      vl_state<NS>(g, m - g.sJ, left);
      Real f[6];
#pragma unroll
      for (int n = 0; n < 6; n++) f[n] = 0.0;
      if (need2) vl_face<NS, 1>(g, left, here, f);
#pragma unroll
      for (int n = 0; n < NV; n++) s_f2[row][n][lane] = f[n];
      __syncthreads();
      if (row < VP_TJ - 1) {
#pragma unroll
        for (int n = 0; n < NV; n++) d2[n] = s_f2[row + 1][n][lane] - f[n];
        m2hi = s_f2[row + 1][0][lane];
      }
      m2lo = f[0];
      __syncthreads();
    }
    __builtin_amdgcn_sched_barrier(0);
    if (cell) {
      Real f[6];
      vl_face<NS, 2>(g, here, above, f);                                         // face k+1
#pragma unroll
      for (int n = 0; n < NV; n++) d3[n] = f[n] - f3lo[n];
      m3lo = f3lo[0]; m3hi = f[0];
#pragma unroll
      for (int n = 0; n < NV; n++) f3lo[n] = f[n];
      Real u[6];
#pragma unroll
      for (int v = 0; v < NV; v++) u[v] = Uf(g, v)[m];
      const Real d0 = u[0];
      // :436-478 flux differences x1, x2, x3; sweep component n of direction D is global variable gv<D>(n)
#pragma unroll
      for (int n = 0; n < NV; n++) u[gv<0>(n)] -= q[0]*d1[n];
#pragma unroll
      for (int n = 0; n < NV; n++) u[gv<1>(n)] -= q[1]*d2[n];
#pragma unroll
      for (int n = 0; n < NV; n++) u[gv<2>(n)] -= q[2]*d3[n];
      if (GRAV) {   // :480-510
        const Real phic = Pf(g, 0)[m];
        { const Real phir = Pf(g, 1)[m + 1], phil = Pf(g, 1)[m];
          u[1] -= q[0]*(phir - phil)*d0;
          u[4] -= q[0]*(m1lo*(phic - phil) + m1hi*(phir - phic)); }
        { const Real phir = Pf(g, 2)[m + g.sJ], phil = Pf(g, 2)[m];
          u[2] -= q[1]*(phir - phil)*d0;
          u[4] -= q[1]*(m2lo*(phic - phil) + m2hi*(phir - phic)); }
        { const Real phir = Pf(g, 3)[m + g.sK], phil = Pf(g, 3)[m];
          u[3] -= q[2]*(phir - phil)*d0;
          u[4] -= q[2]*(m3lo*(phic - phil) + m3hi*(phir - phic)); }
      }
#pragma unroll
      for (int v = 0; v < NV; v++) LRf(g, 0, 0, v)[m] = u[v];
    }
    below = here; here = above;
  }
}

template <int NS, bool GRAV>
__global__ void __launch_bounds__(256)
k_vl_uhalf(DevGrid g, Real dt)
{
  const int ni = g.ie - g.is + 7, nj = g.je - g.js + 7, nk = g.ke - g.ks + 7;
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= (long)ni*nj*nk) return;
  const int i = g.is - 3 + (int)(lin % ni), j = g.js - 3 + (int)((lin / ni) % nj), k = g.ks - 3 + (int)(lin / ((long)ni*nj));
  const long m = (long)k*g.sK + (long)j*g.sJ + i;
  constexpr int NV = 5 + NS;
  Real u[6], q[3];
#pragma unroll
  for (int v = 0; v < NV; v++) u[v] = Uf(g, v)[m];
  const Real d0 = u[0];
#pragma unroll
  for (int d = 0; d < 3; d++) q[d] = 0.5*(dt/g.dx[d]);
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const long sd = stride_rt(g, d);
#pragma unroll
    for (int v = 0; v < NV; v++) { const Real *f = Ff(g, d, v); u[v] -= q[d]*(f[m + sd] - f[m]); }
  }
  if (GRAV) {   // :480-510
    const Real phic = Pf(g, 0)[m];
#pragma unroll
    for (int e = 0; e < 3; e++) {
      const long se = stride_rt(g, e);
      const Real phir = Pf(g, 1 + e)[m + se], phil = Pf(g, 1 + e)[m];
      const Real *fd = Ff(g, e, 0);
      u[1 + e] -= q[e]*(phir - phil)*d0;
      u[4] -= q[e]*(fd[m]*(phic - phil) + fd[m + se]*(phir - phic));
    }
  }
#pragma unroll
  for (int v = 0; v < NV; v++) LRf(g, 0, 0, v)[m] = u[v];
}

#if !AA_COOLING
// ---- first-order flux correction (integrate_3d_vl.c, FIRST_ORDER_FLUX_CORRECTION) ---------------------------------------------
// The reference keeps a copy of the predictor fluxes (Step 5d, 3 x nvar doubles per zone) for the few faces Steps 10 and 14 ever
// look at.  Here they are recomputed for those faces from U^n (`un`, copied before the predictor: a third of that traffic, and
// k_vl_predict never has its fluxes in HBM): the donor-cell flux of face m along D exactly as k_vl_flux1 forms it, sweep frame.
template <int NS, int D>
AA_DEV void fofc_pred_flux(const DevGrid &g, const Real *un, long m, Real f[6])
{
  const long s = stride<D>(g);
  Real u[6], wl[6], wr[6], ul[6], ur[6];
  load_sweep<D, NS>(un, g.nc, m - s, u); cons_to_prim<NS>(u, wl, g.Gamma_1);
  load_sweep<D, NS>(un, g.nc, m, u);     cons_to_prim<NS>(u, wr, g.Gamma_1);
  prim_to_cons<NS>(wl, ul, g.Gamma_1, g.rGamma_1);
  prim_to_cons<NS>(wr, ur, g.Gamma_1, g.rGamma_1);
  flux_roe<NS>(ul, ur, wl, wr, 0.0, g.Gamma, g.Gamma_1, f);
}
// second-order minus predictor flux of face m along DP, sweep-frame components d, Mx, My, Mz, E; the second-order flux is taken
// from the array of direction D2 (D2 != DP only where the reference does so: fofc_fix_cell)
template <int NS, int D2, int DP>
AA_DEV void fofc_flux_diff(const DevGrid &g, const Real *un, long m, Real fd[5])
{
  Real f2[6], fp[6];
  load_sweep<D2, NS>(Ff(g, D2, 0), g.nc, m, f2);
  fofc_pred_flux<NS, DP>(g, un, m, fp);
#pragma unroll
  for (int n = 0; n < 5; n++) fd[n] = f2[n] - fp[n];
}
// U[m] (+/-)= dtodx * fd, the momenta taking the sweep-frame components (c1, c2, c3) of fd
AA_DEV void fofc_add(const DevGrid &g, long m, Real sign, Real dtodx, const Real fd[5], int c1, int c2, int c3)
{
  const int c[5] = {0, c1, c2, c3, 4};
#pragma unroll
  for (int v = 0; v < 5; v++) {
    Real *u = Uf(g, v) + m;
    if (sign > 0.0) *u += dtodx*(fd[c[v]]); else *u -= dtodx*(fd[c[v]]);
  }
}
// FixCell (integrate_3d_vl.c:1995-2232), hydro: the zone trades the second-order fluxes of its six faces for the predictor
// fluxes; so does each neighbour for the face it shares, if it lies strictly inside the Grid's index range in that direction
// as the reference tests it (ix.i > is, ix.i < ie, ...: the periodic image of a zone across the boundary is NOT corrected, and
// the run is no longer conservative there -- the reference's behaviour, kept).  Passive scalars are not corrected (no s[n]
// lines in FixCell).  Two things in the reference's x3 lines look like slips and are reproduced because parity is the bar:
//   * the flux difference of the UPPER x3 face is x2Flux[k+1] - x3FluxP[k+1] (:2014-2047): the x2 array, every field;
//   * the x3 differences go to the momenta in the x2 rotation (M1 <- Mz, M2 <- Mx, M3 <- My; :2085-2090, :2139-2157), where
//     Step 13c uses M1 <- My, M2 <- Mz, M3 <- Mx.
template <int NS>
AA_DEV void fofc_fix_cell(const DevGrid &g, const Real *un, Real dt, long m, int i, int j, int k)
{
  const Real dtodx1 = dt/g.dx[0], dtodx2 = dt/g.dx[1], dtodx3 = dt/g.dx[2];
  Real x1_i[5], x1_ip1[5], x2_j[5], x2_jp1[5], x3_k[5], x3_kp1[5], c[5];
  fofc_flux_diff<NS, 0, 0>(g, un, m, x1_i);
  fofc_flux_diff<NS, 1, 1>(g, un, m, x2_j);
  fofc_flux_diff<NS, 2, 2>(g, un, m, x3_k);
  fofc_flux_diff<NS, 0, 0>(g, un, m + 1, x1_ip1);
  fofc_flux_diff<NS, 1, 1>(g, un, m + g.sJ, x2_jp1);
  fofc_flux_diff<NS, 1, 2>(g, un, m + g.sK, x3_kp1);       // x2Flux[k+1] - x3FluxP[k+1]: as the reference has it
#pragma unroll
  for (int n = 0; n < 5; n++) c[n] = x1_ip1[n] - x1_i[n];
  fofc_add(g, m, 1.0, dtodx1, c, 1, 2, 3);
#pragma unroll
  for (int n = 0; n < 5; n++) c[n] = x2_jp1[n] - x2_j[n];
  fofc_add(g, m, 1.0, dtodx2, c, 3, 1, 2);
#pragma unroll
  for (int n = 0; n < 5; n++) c[n] = x3_kp1[n] - x3_k[n];
  fofc_add(g, m, 1.0, dtodx3, c, 3, 1, 2);
  if (i > g.is) fofc_add(g, m - 1, 1.0, dtodx1, x1_i, 1, 2, 3);
  if (i < g.ie) fofc_add(g, m + 1, -1.0, dtodx1, x1_ip1, 1, 2, 3);
  if (j > g.js) fofc_add(g, m - g.sJ, 1.0, dtodx2, x2_j, 3, 1, 2);
  if (j < g.je) fofc_add(g, m + g.sJ, -1.0, dtodx2, x2_jp1, 3, 1, 2);
  if (k > g.ks) fofc_add(g, m - g.sK, 1.0, dtodx3, x3_k, 3, 1, 2);
  if (k < g.ke) fofc_add(g, m + g.sK, -1.0, dtodx3, x3_kp1, 3, 1, 2);
}
// Step 14 (:1255-1279) is a sequential scan in k, j, i order: a fix changes the +i, +j, +k neighbours BEFORE the scan examines
// them (they may turn bad, or good again) and the -i, -j, -k neighbours after it did (never looked at again), so fixing all
// flagged zones at once is not the same thing.  The scan is replayed over the only zones it can flag: the candidates of the
// update (d < 0 in a zone no fix touched is what the update saw) and the upper neighbours of the zones fixed so far, in
// ascending zone index -- which is scan order.  One wavefront: the lanes sort the candidates (rank sort: they are distinct),
// lane 0 walks.  buf: AA_FOFC_MAX candidates | sorted | pending upper neighbours (sorted, distinct).
template <int NS>
__global__ void __launch_bounds__(64)
k_fofc_fix(DevGrid g, const Real *un, Real dt, DevScalars *sc, long long *buf)
{
  const long long *cand = buf;
  long long *sorted = buf + AA_FOFC_MAX, *pend = buf + 2*AA_FOFC_MAX;
  const int n = sc->fofc_n;               // (<= AA_FOFC_MAX: the host has looked)
  for (int e = threadIdx.x; e < n; e += 64) {
    const long long v = cand[e];
    int r = 0;
    for (int q = 0; q < n; q++) r += cand[q] < v;
    sorted[r] = v;
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x != 0) return;
  int negd = 0, negP = 0, ci = 0, pi = 0, pn = 0, ovf = 0;
  while (ci < n || pi < pn) {
    const long long a = ci < n ? sorted[ci] : 0x7fffffffffffffffLL, b = pi < pn ? pend[pi] : 0x7fffffffffffffffLL;
    const long m = (long)(a < b ? a : b);
    if (a == m) ci++;
    if (b == m) pi++;
    const int k = (int)(m / g.sK), j = (int)((m % g.sK) / g.sJ), i = (int)(m % g.sJ);
    Real u[6], w[6];
#pragma unroll
    for (int v = 0; v < 5; v++) u[v] = Uf(g, v)[m];
    u[5] = 0.0;
    cons_to_prim<0>(u, w, g.Gamma_1);      // Cons_to_Prim of the CURRENT state (convert_var.c:104: Cons1D_to_Prim1D, which floors P)
    bool flag = false;
    if (w[0] < 0.0) { flag = true; negd++; }
    if (w[4] < 0.0) { flag = true; negP++; }
    if (!flag) continue;
    fofc_fix_cell<NS>(g, un, dt, m, i, j, k);
    const long up[3] = {i < g.ie ? m + 1 : -1L, j < g.je ? m + g.sJ : -1L, k < g.ke ? m + g.sK : -1L};   // ascending
    for (int a3 = 0; a3 < 3; a3++) {
      if (up[a3] < 0) continue;
      int q = pn;
      while (q > pi && pend[q - 1] > up[a3]) q--;
      if (q > pi && pend[q - 1] == up[a3]) continue;
      if (pn >= AA_FOFC_MAX) { ovf = 1; continue; }
      for (int r = pn; r > q; r--) pend[r] = pend[r - 1];
      pend[q] = up[a3]; pn++;
    }
  }
  sc->fofc_negd = negd; sc->fofc_negP = negP; sc->fofc_ovf = ovf;
}
// Step 10 (:775-791, :825-841, :875-891): a second-order flux with a NaN in d, Mx, My, Mz or E becomes the predictor flux of its
// face, all components (the scalar flux is part of the struct copy).  Faces as the reference loops: [s, e+1] along D, [s-1, e+1]
// across (the sweeps fill at least that).
template <int NS, int D>
__global__ void __launch_bounds__(256)
k_fofc_nanfix(DevGrid g, const Real *un, DevScalars *sc)
{
  const int ni = g.ie - g.is + 3 - (D == 0), nj = g.je - g.js + 3 - (D == 1), nk = g.ke - g.ks + 3 - (D == 2);
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= (long)ni*nj*nk) return;
  const int i = g.is - (D != 0) + (int)(lin % ni), j = g.js - (D != 1) + (int)((lin / ni) % nj), k = g.ks - (D != 2) + (int)(lin / ((long)ni*nj));
  const long m = (long)k*g.sK + (long)j*g.sJ + i;
  Real f[6];
  load_sweep<D, NS>(Ff(g, D, 0), g.nc, m, f);
  if (f[0] == f[0] && f[1] == f[1] && f[2] == f[2] && f[3] == f[3] && f[4] == f[4]) return;
  fofc_pred_flux<NS, D>(g, un, m, f);
  store_sweep<D, NS>(Ff(g, D, 0), g.nc, m, f);
  atomicAdd(&sc->fofc_nan, 1);
}
#endif

// ---- physical boundary conditions: bvals_mhd.c reflect :959, outflow :1319, periodic :1637 ---
// dir d, side 0/1; transverse extents: x1 -> active j,k; x2 -> all i, active k; x3 -> all i,j.
// side < 0: both sides in one launch, blockIdx.y = side, (flag, flag1) = the two flags (0 = leave alone)
__global__ void k_bc(DevGrid g, int nvar, int d, int side, int flag, int flag1)
{
  if (side < 0) { side = blockIdx.y; if (side) flag = flag1; if (!flag) return; }
  const int lo3[3] = {g.is, g.js, g.ks}, hi3[3] = {g.ie, g.je, g.ke}, N[3] = {g.N1, g.N2, g.N3};
  int r0[3], n[3];
  for (int a = 0; a < 3; a++) {
    if (a == d) { r0[a] = 0; n[a] = AA_NGHOST_; continue; }
    if (a < d) { r0[a] = 0; n[a] = N[a]; } else { r0[a] = lo3[a]; n[a] = hi3[a] - lo3[a] + 1; }
  }
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= (long)n[0]*n[1]*n[2]) return;
  int idx[3];
  idx[0] = r0[0] + (int)(lin % n[0]);
  idx[1] = r0[1] + (int)((lin / n[0]) % n[1]);
  idx[2] = r0[2] + (int)(lin / ((long)n[0]*n[1]));
  const int gl = idx[d] + 1;                                    // ghost layer 1..4
  int dst, src;
  if (side == 0) { dst = lo3[d] - gl; src = (flag == 1) ? lo3[d] + (gl - 1) : (flag == 2) ? lo3[d] : hi3[d] - (gl - 1); }
  else           { dst = hi3[d] + gl; src = (flag == 1) ? hi3[d] - (gl - 1) : (flag == 2) ? hi3[d] : lo3[d] + (gl - 1); }
  idx[d] = 0;
  const long base = (long)idx[2]*g.sK + (long)idx[1]*g.sJ + idx[0];
  const long sd = stride_rt(g, d);
  for (int v = 0; v < nvar; v++) {
    Real x = Uf(g, v)[base + src*sd];
    if (flag == 1 && v == 1 + d) x = -x;
    Uf(g, v)[base + dst*sd] = x;
  }
}

// bvals_mhd in ONE launch.  The three passes x1 -> x2 -> x3 are copies along one coordinate each (k_bc), so what a ghost zone ends up
// with is the value of ONE source zone, found by walking its ghost coordinates from x3 down: a pass d writes the zones whose
// coordinate d is a ghost one (flag != 0), for every value of the coordinates below d and ACTIVE coordinates above it, from the
// zone with coordinate d mapped into the active range -- whose lower ghost coordinates were filled by the passes before, the same
// way.  So: map x3 if it is a ghost coordinate with a boundary function, then x2, then x1; stop at the first ghost coordinate whose
// side has none (flag 0: a neighbour Grid's or a parent's data; the passes below never touch a zone with that coordinate outside
// the active range).  A zone is written iff its HIGHEST ghost coordinate has a boundary function; no source zone is itself a
// target, so the launch needs no ordering.  Reflecting sides negate their normal momentum once per mapped coordinate.  Same bits
// as the three passes (copies and sign flips only).
__global__ void __launch_bounds__(256)
k_bc_shell(DevGrid g, int nvar, int f0, int f1, int f2, int f3, int f4, int f5)
{
  const int flag[3][2] = {{f0, f1}, {f2, f3}, {f4, f5}};
  const int lo3[3] = {g.is, g.js, g.ks}, hi3[3] = {g.ie, g.je, g.ke}, N[3] = {g.N1, g.N2, g.N3};
  const int G2 = 2*AA_NGHOST_;
  // the shell in three pieces: ghost k (all i, j); ghost j, active k (all i); ghost i, active j and k
  const long n3 = (long)G2*N[1]*N[0], n2 = (long)G2*N[0]*(hi3[2] - lo3[2] + 1), n1 = (long)G2*(hi3[1] - lo3[1] + 1)*(hi3[2] - lo3[2] + 1);
  long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  int c[3];
  auto ghost = [&](int q, int d) { return q < AA_NGHOST_ ? q : hi3[d] + 1 + (q - AA_NGHOST_); };      // q-th ghost index of direction d
  if (lin < n3) {
    c[0] = (int)(lin % N[0]); c[1] = (int)((lin / N[0]) % N[1]); c[2] = ghost((int)(lin / ((long)N[0]*N[1])), 2);
  } else if ((lin -= n3) < n2) {
    c[0] = (int)(lin % N[0]); c[1] = ghost((int)((lin / N[0]) % G2), 1); c[2] = lo3[2] + (int)(lin / ((long)N[0]*G2));
  } else if ((lin -= n2) < n1) {
    c[0] = ghost((int)(lin % G2), 0); c[1] = lo3[1] + (int)((lin / G2) % (hi3[1] - lo3[1] + 1)); c[2] = lo3[2] + (int)(lin / ((long)G2*(hi3[1] - lo3[1] + 1)));
  } else return;
  const long mdst = (long)c[2]*g.sK + (long)c[1]*g.sJ + c[0];
  bool neg[3] = {false, false, false}, any = false;
#pragma unroll
  for (int d = 2; d >= 0; d--) {
    const int x = c[d];
    if (x >= lo3[d] && x <= hi3[d]) continue;
    const int side = (x < lo3[d]) ? 0 : 1, fl = flag[d][side];
    if (!fl) { if (!any) return; break; }              // (highest ghost coordinate without a boundary function: not ours; a lower one: stop)
    const int gl = side ? x - hi3[d] : lo3[d] - x;       // ghost layer 1..4
    if (side == 0) c[d] = (fl == 1) ? lo3[d] + (gl - 1) : (fl == 2) ? lo3[d] : hi3[d] - (gl - 1);
    else           c[d] = (fl == 1) ? hi3[d] - (gl - 1) : (fl == 2) ? hi3[d] : lo3[d] + (gl - 1);
    if (fl == 1) neg[d] = true;
    any = true;
  }
  const long msrc = (long)c[2]*g.sK + (long)c[1]*g.sJ + c[0];
  for (int v = 0; v < nvar; v++) {
    Real x = Uf(g, v)[msrc];
    if (v >= 1 && v <= 3 && neg[v - 1]) x = -x;
    Uf(g, v)[mdst] = x;
  }
}

// ---- CFL reduction: new_dt.c:72-170 -----------------------------------------------------
__global__ void __launch_bounds__(256)
k_cfl(DevGrid g, DevScalars *sc)
{
  const int ni = g.ie - g.is + 1, nj = g.je - g.js + 1, nk = g.ke - g.ks + 1;
  const long ntot = (long)ni*nj*nk;
  Real mx[3] = {0.0, 0.0, 0.0};
  for (long lin = (long)blockIdx.x*blockDim.x + threadIdx.x; lin < ntot; lin += (long)gridDim.x*blockDim.x) {
    const int i = g.is + (int)(lin % ni);
    const int j = g.js + (int)((lin / ni) % nj);
    const int k = g.ks + (int)(lin / ((long)ni*nj));
    const long m = (long)k*g.sK + (long)j*g.sJ + i;
    cfl_zone(Uf(g, 0)[m], Uf(g, 1)[m], Uf(g, 2)[m], Uf(g, 3)[m], Uf(g, 4)[m], g.Gamma, g.Gamma_1, mx);
  }
  __shared__ Real red[3][256];
  for (int d = 0; d < 3; d++) red[d][threadIdx.x] = mx[d];
  __syncthreads();
  for (int s = blockDim.x/2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) for (int d = 0; d < 3; d++) red[d][threadIdx.x] = rmax(red[d][threadIdx.x], red[d][threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) for (int d = 0; d < 3; d++) atomic_max_pos(&sc->max_v[d], red[d][0]);
}

// ---- history sums (dump_history.c:157-200): mass, E, momenta, kinetic energies, scalar; one
// partial row per block, added up on the host in block order (deterministic) ------------------
__global__ void __launch_bounds__(256)
k_history(DevGrid g, int nscal, Real *partial)
{
  const int ni = g.ie - g.is + 1, nj = g.je - g.js + 1, nk = g.ke - g.ks + 1;
  const long ntot = (long)ni*nj*nk;
  Real acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long lin = (long)blockIdx.x*blockDim.x + threadIdx.x; lin < ntot; lin += (long)gridDim.x*blockDim.x) {
    const int i = g.is + (int)(lin % ni);
    const int j = g.js + (int)((lin / ni) % nj);
    const int k = g.ks + (int)(lin / ((long)ni*nj));
    const long m = (long)k*g.sK + (long)j*g.sJ + i;
    const Real d = Uf(g, 0)[m], d1 = 1.0/d, M1 = Uf(g, 1)[m], M2 = Uf(g, 2)[m], M3 = Uf(g, 3)[m];
    acc[0] += d; acc[1] += Uf(g, 4)[m]; acc[2] += M1; acc[3] += M2; acc[4] += M3;
    acc[5] += 0.5*M1*M1*d1; acc[6] += 0.5*M2*M2*d1; acc[7] += 0.5*M3*M3*d1;
    if (nscal) acc[8] += Uf(g, 5)[m];
  }
  __shared__ Real red[9][256];
  for (int q = 0; q < 9; q++) red[q][threadIdx.x] = acc[q];
  __syncthreads();
  for (int s = blockDim.x/2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) for (int q = 0; q < 9; q++) red[q][threadIdx.x] += red[q][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < 9) partial[(long)blockIdx.x*9 + threadIdx.x] = red[threadIdx.x][0];
}

// ---- layout conversion, pinned cells, x3 halo pack/unpack ----------------------------------
__global__ void k_aos_to_soa(DevGrid g, int nvar, const Real *aos)
{
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  const long ntot = (long)g.N1*g.N2*g.N3;
  if (lin >= ntot) return;
  const int i = (int)(lin % g.N1), j = (int)((lin / g.N1) % g.N2), k = (int)(lin / ((long)g.N1*g.N2));
  const long m = (long)k*g.sK + (long)j*g.sJ + i;
  for (int v = 0; v < nvar; v++) Uf(g, v)[m] = aos[lin*nvar + v];
}
__global__ void k_soa_to_aos(DevGrid g, int nvar, Real *aos)
{
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  const long ntot = (long)g.N1*g.N2*g.N3;
  if (lin >= ntot) return;
  const int i = (int)(lin % g.N1), j = (int)((lin / g.N1) % g.N2), k = (int)(lin / ((long)g.N1*g.N2));
  const long m = (long)k*g.sK + (long)j*g.sJ + i;
  for (int v = 0; v < nvar; v++) aos[lin*nvar + v] = Uf(g, v)[m];
}
// the same with the zones' contribution to new_dt's maxima from the values just written (what k_pinned_cfl reads back): one launch
__global__ void k_pinned_with_cfl(DevGrid g, int nvar, long long n, const long long *idx, const Real *vals, DevScalars *sc)
{
  Real mx[3] = {0.0, 0.0, 0.0};
  for (long lin = (long)blockIdx.x*blockDim.x + threadIdx.x; lin < n; lin += (long)gridDim.x*blockDim.x) {
    const long long c = idx[lin];
    const int i = (int)(c % g.N1), j = (int)((c / g.N1) % g.N2), k = (int)(c / ((long)g.N1*g.N2));
    const long m = (long)k*g.sK + (long)j*g.sJ + i;
    const Real *q = vals + lin*nvar;
    for (int v = 0; v < nvar; v++) Uf(g, v)[m] = q[v];
    if (i >= g.is && i <= g.ie && j >= g.js && j <= g.je && k >= g.ks && k <= g.ke)      // new_dt looks at active zones only
      cfl_zone(q[0], q[1], q[2], q[3], q[4], g.Gamma, g.Gamma_1, mx);
  }
#pragma unroll
  for (int d = 0; d < 3; d++) {
    Real v = mx[d];
    for (int o = 32; o > 0; o >>= 1) { const Real w = __shfl_xor(v, o); v = (w > v || v != v) ? w : v; }
    if ((threadIdx.x & 63) == 0) atomic_max_pos(&sc->max_v[d], v);
  }
}
__global__ void k_pinned(DevGrid g, int nvar, long long n, const long long *idx, const Real *vals)
{
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= n) return;
  const long long c = idx[lin];                       // linear [k][j][i] index of the host block
  const int i = (int)(c % g.N1), j = (int)((c / g.N1) % g.N2), k = (int)(c / ((long)g.N1*g.N2));
  const long m = (long)k*g.sK + (long)j*g.sJ + i;
  for (int v = 0; v < nvar; v++) Uf(g, v)[m] = vals[lin*nvar + v];
}
// 4 k-planes starting at k0, all i and j (x3 is exchanged last, so corners travel: bvals_mhd.c:170)
// buffer layout [v][kk][j][i]
__global__ void k_pack_x3(DevGrid g, int nvar, int k0, Real *buf)
{
  const long plane = (long)g.N1*g.N2, ntot = plane*AA_NGHOST_;
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= ntot) return;
  const int i = (int)(lin % g.N1), j = (int)((lin / g.N1) % g.N2), kk = (int)(lin / plane);
  const long m = (long)(k0 + kk)*g.sK + (long)j*g.sJ + i;
  for (int v = 0; v < nvar; v++) buf[(long)v*ntot + lin] = Uf(g, v)[m];
}
// bvals_mhd.c:2462 pack_ix2 / pack_ox2 and :2896 unpack_ix2 / unpack_ox2: four rows j0 .. j0+3, all i incl. the x1 ghost
// zones (x1 comes first, so the x1-x2 corners travel), the active k-planes only (x3 comes after)
__global__ void k_pack_x2(DevGrid g, int nvar, int j0, Real *buf)
{
  const long nk = g.ke - g.ks + 1, ntot = (long)g.N1*AA_NGHOST_*nk;
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= ntot) return;
  const int i = (int)(lin % g.N1), jj = (int)((lin / g.N1) % AA_NGHOST_), kk = (int)(lin / ((long)g.N1*AA_NGHOST_));
  const long m = (long)(g.ks + kk)*g.sK + (long)(j0 + jj)*g.sJ + i;
  for (int v = 0; v < nvar; v++) buf[(long)v*ntot + lin] = Uf(g, v)[m];
}
__global__ void k_unpack_x2(DevGrid g, int nvar, int j0, const Real *buf)
{
  const long nk = g.ke - g.ks + 1, ntot = (long)g.N1*AA_NGHOST_*nk;
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= ntot) return;
  const int i = (int)(lin % g.N1), jj = (int)((lin / g.N1) % AA_NGHOST_), kk = (int)(lin / ((long)g.N1*AA_NGHOST_));
  const long m = (long)(g.ks + kk)*g.sK + (long)(j0 + jj)*g.sJ + i;
  for (int v = 0; v < nvar; v++) Uf(g, v)[m] = buf[(long)v*ntot + lin];
}
__global__ void k_unpack_x3(DevGrid g, int nvar, int k0, const Real *buf)
{
  const long plane = (long)g.N1*g.N2, ntot = plane*AA_NGHOST_;
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= ntot) return;
  const int i = (int)(lin % g.N1), j = (int)((lin / g.N1) % g.N2), kk = (int)(lin / plane);
  const long m = (long)(k0 + kk)*g.sK + (long)j*g.sJ + i;
  for (int v = 0; v < nvar; v++) Uf(g, v)[m] = buf[(long)v*ntot + lin];
}

// ---- function-level test kernels ------------------------------------------------------------
template <int NS>
__global__ void k_test_fluxes(Real Gamma, int n, const Real *Ul, const Real *Ur, const Real *eta, Real *F)
{
  const int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  constexpr int NV = 5 + NS;
  Real ul[6] = {0, 0, 0, 0, 0, 0}, ur[6] = {0, 0, 0, 0, 0, 0}, wl[6], wr[6], f[6];
  for (int v = 0; v < NV; v++) { ul[v] = Ul[(long)t*NV + v]; ur[v] = Ur[(long)t*NV + v]; }
  cons_to_prim<NS>(ul, wl, Gamma - 1.0); cons_to_prim<NS>(ur, wr, Gamma - 1.0);
  flux_roe<NS>(ul, ur, wl, wr, eta[t], Gamma, Gamma - 1.0, f);
  for (int v = 0; v < NV; v++) F[(long)t*NV + v] = f[v];
}
// x_div / x_sqrt / x_div_r (hydro_dev.h) beside hipcc's own a/b and sqrt(a): out = [5][n]
__global__ void k_test_xdiv(int n, const Real *a, const Real *b, Real *out)
{
  const int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Real x = a[t], y = b[t];
  out[t] = x_div(x, y); out[(long)n + t] = x/y;
  out[2L*n + t] = x_sqrt(x); out[3L*n + t] = sqrt(x);
  out[4L*n + t] = x_div_r(x, y, 1.0/y);                 // with the correctly rounded reciprocal (what the host supplies for gamma-1)
}
// The marching kernels' accessors (top of the file) at the ends of the 32-bit offset's range: lane l < 4 takes byte offset t.off[l],
// phase 0 stores a word there through the accessors -- on `base` and on `base` moved up by the scalar stride -- and phase 1, a launch
// of its own so that nothing is forwarded, loads the words back the same way, and once more from the zone below through the
// immediate.  out[3][4]: base, base + stride, immediate.
struct ZoneOffTest { unsigned off[4]; };
__global__ void k_test_zone_offsets(Real *base, ZoneOffTest t, unsigned stride, int phase, Real *out)
{
  const int l = threadIdx.x;
  if (l >= 4) return;
  unsigned mb = (l == 0) ? t.off[0] : (l == 1) ? t.off[1] : (l == 2) ? t.off[2] : t.off[3];
  asm volatile("" : "+v"(mb));
  asm volatile("" : "+s"(stride));
  const FBase b = (FBase)base, b2 = fup(b, stride);
  if (phase == 0) {
    zstore(b, mb, 1000.0 + l);
    zstore(b2, mb, 2000.0 + l);
  } else {
    const unsigned o = zsite(mb, b);
    out[l] = zp(b, o)[0];
    out[4 + l] = zp(b2, o)[0];
    const unsigned lo = zsite(mb >= 8u ? mb - 8u : mb, b2);
    const Real up = zp(b, lo)[1], here = zp(b, lo)[0];      // (both inside the field)
    out[8 + l] = (mb >= 8u) ? up : here;
  }
}
template <int NS>
__global__ void k_test_lr_ppm(Real Gamma, int n, const Real *W, Real dt, Real dx, int il, int iu, Real *Wl, Real *Wr)
{
  const int c = il - 1 + blockIdx.x*blockDim.x + threadIdx.x;     // cells il-1 .. iu+1
  if (c > iu + 1) return;
  constexpr int NV = 5 + NS;
  Real w5[5][6], D[3][6], a[6], b[6];
  for (int q = 0; q < 5; q++) for (int v = 0; v < 6; v++) w5[q][v] = (v < NV) ? W[(long)(c - 2 + q)*NV + v] : 0.0;
  for (int q = 0; q < 3; q++) limited_slopes<NS>(w5[q], w5[q + 1], w5[q + 2], Gamma, D[q]);
  ppm_cell<NS>(w5[1], w5[2], w5[3], D[0], D[1], D[2], dt/dx, Gamma, a, b);
  for (int v = 0; v < NV; v++) { Wl[(long)(c + 1)*NV + v] = a[v]; Wr[(long)c*NV + v] = b[v]; }
}
template <int NS>
__global__ void k_test_lr(Real Gamma, int n, const Real *W, Real dt, Real dx, int il, int iu, Real *Wl, Real *Wr)
{
  const int c = il - 1 + blockIdx.x*blockDim.x + threadIdx.x;     // cells il-1 .. iu+1
  if (c > iu + 1) return;
  constexpr int NV = 5 + NS;
  Real wm[6] = {0, 0, 0, 0, 0, 0}, w[6] = {0, 0, 0, 0, 0, 0}, wp[6] = {0, 0, 0, 0, 0, 0}, a[6], b[6];
  for (int v = 0; v < NV; v++) { wm[v] = W[(long)(c - 1)*NV + v]; w[v] = W[(long)c*NV + v]; wp[v] = W[(long)(c + 1)*NV + v]; }
  plm_cell<NS, true>(wm, w, wp, dt/dx, Gamma, a, b);
  for (int v = 0; v < NV; v++) { Wl[(long)(c + 1)*NV + v] = a[v]; Wr[(long)c*NV + v] = b[v]; }
}

// =============================================================================================
// host-side launchers
// =============================================================================================
void launch_test_zone_offsets(Real *base, const unsigned off[4], unsigned stride, int phase, Real *out, hipStream_t st)
{
  ZoneOffTest t; for (int l = 0; l < 4; l++) t.off[l] = off[l];
  hipLaunchKernelGGL(k_test_zone_offsets, dim3(1), dim3(64), 0, st, base, t, stride, phase, out);
}
void launch_test_xdiv(int n, const Real *a, const Real *b, Real *out, hipStream_t st)
{ hipLaunchKernelGGL(k_test_xdiv, dim3((n + 255)/256), dim3(256), 0, st, n, a, b, out); }
static inline unsigned nblk(long n, int b) { return (unsigned)((n + b - 1)/b); }
static Order zone_order(const HostGrid &g) { Order o = {g.cfg.strip, g.cfg.xcd}; return o; }      // (AA_STRIP / AA_XCD as aa_create found them: grid.h LaunchCfg)
// Grid-stride reduction kernels end in a few same-address atomics per block (one word sustains ~90
// atomics/us): at least 8 zones per thread, between 256 and 4096 blocks.
unsigned reduce_blocks(long n)
{ long nb = (n + 256L*8 - 1)/(256L*8); if (nb < 256) nb = 256; if (nb > 4096) nb = 4096; if (nb*256 > n) nb = (n + 255)/256; return (unsigned)nb; }
static inline unsigned nblk8(long n, int b) { unsigned x = nblk(n, b); return ((x + 7u)/8u)*8u; }   // for xcd_block()

template <int NS, bool GRAV, int MODE, int ORD>
static void sweep_impl_o(const HostGrid &g, const Real *src, int dir, Real dt, hipStream_t st, int koff = 0, int kcnt = -1, const Run3D *rc = nullptr)
{
  // (rc: the x2 first pass of a queued step -- the same launch, the entry that reads dt from the device clock)
  // (koff, kcnt): for the x1 and x2 sweeps, the k-planes ks-2+koff .. +kcnt-1 only (every pencil is on its own: any
  // partition of the planes gives the same bits)
  const int nk_all = g.ke - g.ks + 5;
  if (kcnt < 0) kcnt = nk_all - koff;
  if (kcnt <= 0) return;
  if (dir == 0) {
    const int flat = g.cfg.x1_flat;
    const long nc = g.ie - g.is + 5, nslots = nc*(g.je - g.js + 5);
    if (flat && nslots < (1L << 30)) {
      int rsh = 31; while ((2L << (rsh - 31)) <= nc) rsh++;            // 31 + floor(log2 nc)
      const unsigned long long rmul = ((1ULL << rsh) + nc - 1)/nc;      // <= 2^31; exact quotients for slots < 2^30
      int Bf = (int)((nslots + 63)/64)*64; if (Bf > 256 || nslots > 256) Bf = 256;
      dim3 gridf((unsigned)((nslots - 1 + Bf - 2)/(Bf - 1)), kcnt);
      if (gridf.x < 1) gridf.x = 1;
      hipLaunchKernelGGL((k_sweep_x1_flat<NS, GRAV, MODE, ORD>), gridf, dim3(Bf), (size_t)(5 + NS)*Bf*sizeof(Real), st, g, src, dt,
                         koff, (unsigned)nslots, (unsigned)rmul, rsh);
      return;
    }
    const int nfaces = (g.ie - g.is + 1) + 3;          // interfaces l+1..u
    int nb = (nfaces + 254)/255;
    int B = (nfaces + nb - 1)/nb + 1;                  // B-1 interfaces per block
    B = ((B + 63)/64)*64; if (B > 256) B = 256;
    nb = (nfaces + (B - 1) - 1)/(B - 1);
    dim3 grid(nb, g.je - g.js + 5, kcnt);
    size_t lds = (size_t)(5 + NS)*(B + 2)*sizeof(Real);
    hipLaunchKernelGGL((k_sweep_x1<NS, GRAV, MODE, ORD>), grid, dim3(B), lds, st, g, src, dt, koff);
  } else if constexpr (MODE == MODE_CORR) {
    constexpr int BT = 8;     // 8 beats 16 (12.0 ms) despite the 10-rows-for-7-faces halo: more blocks in flight
    const long ni = g.ie - g.is + 5;
    const long nt = (dir == 1 ? g.ke - g.ks : g.je - g.js) + 5;
    const int nfaces = (dir == 1 ? g.je - g.js : g.ke - g.ks) + 1 + 3;
    dim3 grid(nblk(ni*nt, 64), (nfaces + BT - 2)/(BT - 1)), blk(64, BT);
    const size_t lds = (size_t)(5 + NS)*(BT + 2)*64*sizeof(Real);
    with_dir12(dir, [&](auto D) { hipLaunchKernelGGL((k_sweep_tile<NS, D, GRAV, MODE, BT, ORD>), grid, blk, lds, st, g, src, dt); });
  } else if constexpr (MODE == MODE_FLUX1 || MODE == MODE_VL) {
    const long ni = march_slots(g);
    const long nt = (dir == 1 ? kcnt : g.je - g.js + 5);
    const int toff = (dir == 1 ? koff : 0);
    const int nfaces = (dir == 1 ? g.je - g.js : g.ke - g.ks) + 1 + 3;
    // 32 interfaces per thread amortise the 3-cell start-up of a chunk on big Grids; small Grids need the
    // parallelism more (80^3 has only 110 wavefronts of columns): halve the chunk until the launch has
    // a few wavefronts per SIMD (1024 SIMDs)
#ifndef SW_CHUNK
#define SW_CHUNK 32
#endif
    int chunk = g.cfg.sw_chunk > 0 ? g.cfg.sw_chunk : SW_CHUNK;          // (AA_SW_CHUNK overrides)
    if (g.cfg.sw_chunk <= 0) while (chunk > 4 && (long)nblk(ni*nt, 64)*((nfaces + chunk - 1)/chunk) < 4096) chunk >>= 1;
    dim3 grid(nblk(ni*nt, 64), (nfaces + chunk - 1)/chunk);
#if !AA_COOLING
    if constexpr (MODE == MODE_FLUX1) if (rc && dir == 1) {
      hipLaunchKernelGGL((k_sweep_march_dc<NS, 1, GRAV, MODE_FLUX1, ORD>), grid, dim3(64), 0, st, g, src, rc, chunk, toff, (int)nt);
      return;
    }
#endif
    with_dir12(dir, [&](auto D) { hipLaunchKernelGGL((k_sweep_march<NS, D, GRAV, MODE, ORD>), grid, dim3(64), 0, st, g, src, dt, chunk, toff, (int)nt); });
  }
}
template <int NS, bool GRAV, int MODE>
static void sweep_impl(const HostGrid &g, const Real *src, int dir, Real dt, hipStream_t st, int koff = 0, int kcnt = -1, const Run3D *rc = nullptr)
{
  // third order: the slope arrays were filled from the state the sweep reconstructs (U; U^{n+1/2} for the van Leer corrector)
  with_ord(g.slope != nullptr, [&](auto ORD) { sweep_impl_o<NS, GRAV, MODE, ORD>(g, src, dir, dt, st, koff, kcnt, rc); });
}
template <int NS>
static void slopes_impl(const HostGrid &g, int dir, hipStream_t st, const Real *src)
{
  long n = 1;
  const int lo[3] = {g.is, g.js, g.ks}, hi[3] = {g.ie, g.je, g.ke};
  for (int d = 0; d < 3; d++) n *= hi[d] - lo[d] + 1 + (d == dir ? 6 : 4);
  dim3 grid(nblk(n, 256)), blk(256);
  const int march = g.cfg.slopes_march;
  if (march && dir != 0) {
    const long nq = march_slots(g), nt = (dir == 1 ? g.ke - g.ks : g.je - g.js) + 5;
    const int ncell = (dir == 1 ? g.je - g.js : g.ke - g.ks) + 7;
    int chunk = g.cfg.sw_chunk > 0 ? g.cfg.sw_chunk : 32;                // (AA_SW_CHUNK overrides)
    if (g.cfg.sw_chunk <= 0) while (chunk > 4 && (long)nblk(nq*nt, 64)*((ncell + chunk - 1)/chunk) < 4096) chunk >>= 1;
    dim3 gm(nblk(nq*nt, 64), (ncell + chunk - 1)/chunk);
    with_dir12(dir, [&](auto D) { hipLaunchKernelGGL((k_slopes_march<NS, D>), gm, dim3(64), 0, st, g, src, chunk); });
    return;
  }
  with_dir(dir, [&](auto D) { hipLaunchKernelGGL((k_slopes<NS, D>), grid, blk, 0, st, g, src); });
}
// the first-pass x1 fluxes of the faces between the tiles of k_correct_all (needs U only: the caller may run it beside the x2 sweep)
template <int NS, bool GRAV>
static void x1_edges_impl(const HostGrid &g, Real dt, hipStream_t st, const Run3D *rc = nullptr)
{
  if (x1_edges(g) <= 0) return;
  const int nj = g.je - g.js + 3, nk = g.ke - g.ks + 3;
  dim3 ge(nblk(nj, 64), nk, x1_edges(g));
#if !AA_COOLING
  if (rc) { with_ord(g.slope != nullptr, [&](auto ORD) { hipLaunchKernelGGL((k_x1_edge_flux_dc<NS, GRAV, ORD>), ge, dim3(64), 0, st, g, rc); }); return; }
#endif
  with_ord(g.slope != nullptr, [&](auto ORD) { hipLaunchKernelGGL((k_x1_edge_flux<NS, GRAV, ORD>), ge, dim3(64), 0, st, g, dt); });
}
void launch_x1_edges(const HostGrid &g, int nscal, Real dt, bool grav, hipStream_t st)
{ with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { x1_edges_impl<NS, GRAV>(g, dt, st); }); }
// the correct passes of all three directions in one kernel (after the three first passes; x3f: after those of x2 and the tile-edge x1 fluxes)
template <int NS, bool GRAV>
static void correct_all_impl(const HostGrid &g, Real dt, bool x3f, hipStream_t st, bool edges_done, const Run3D *rc = nullptr)
{
  // (rc: a queued step, x3f only -- the same three launches, dt and the ratios from the device clock)
  const int ni = g.ie - g.is + 3, nj = g.je - g.js + 3, nk = g.ke - g.ks + 3;    // zones s-1 .. e+1
  // planes per block: with the x3 first pass on board a chunk starts three planes early (two of first-pass work only and the
  // provider plane), so longer chunks pay: 64 planes 19.7 against 20.0 - 20.6 ms for 32 at 512^3 (128: 20.4, 16: 20.2);
  // AA_CA_KC overrides
  const int kc_env = g.cfg.ca_kc;
  int kc = kc_env > 0 ? kc_env : (x3f ? 64 : 32);
  // ... on Grids with fewer columns shorter chunks pay more than their start-up planes cost: the launch should hold about
  // eight rounds of the 512 blocks that are resident at a time (measured, profiles/microbench/kc_small.sh: 128^3 and 192^3 best
  // with 8 planes, 1.30 against 1.65 ms at 192^3; 256^3 with 16, 2.80 against 3.09; 320^3 with 32; from 384^3 on with 64)
  if (kc_env <= 0) while (kc > 8 && (long)nblk(ni + 15, 64)*nblk(nj, CA_TJ)*((nk + kc - 1)/kc) < 4096) kc >>= 1;
  dim3 grid(nblk(ni + 15, 64), nblk(nj, CA_TJ), (nk + kc - 1)/kc), blk(64, CA_TJ);
  if (x3f && !edges_done) x1_edges_impl<NS, GRAV>(g, dt, st, rc);
#if !AA_COOLING
  if (rc) {
    // (a combination correct_all_dc_built() names is not instantiated: aa_run_3d steps such a Grid one aa_step at a time)
    if constexpr (AA_FAST_DIV || !(NS && GRAV))
      with_ord(g.slope != nullptr, [&](auto ORD) { hipLaunchKernelGGL((k_correct_all_dc<NS, GRAV, ORD, true>), grid, blk, 0, st, g, rc, kc); });
    else abort();
  } else
#endif
  {
  const StepRatios sr = step_ratios(g, dt);
  with_flag(x3f, [&](auto X3F) { with_ord(g.slope != nullptr, [&](auto ORD) {
    hipLaunchKernelGGL((k_correct_all<NS, GRAV, ORD, X3F>), grid, blk, 0, st, g, dt, kc, sr); }); });
  }
  const long nb1 = (g.ie + 1 - (g.is - 16))/64, nb2 = (g.je + 1 - (g.js - 1))/CA_TJ;
  {
    const long c0 = nb1 > 0 ? nb1*nj*nk : 0, c1 = nb2 > 0 ? (long)ni*nb2*nk : 0;      // (a direction without inner tile edges returns at once)
    if (c0 > 0 || c1 > 0) hipLaunchKernelGGL(k_eta_edges, dim3(nblk(c0 > c1 ? c0 : c1, 256), 2), dim3(256), 0, st, g);
  }
}
void launch_correct_all(const HostGrid &g, int nscal, Real dt, bool grav, bool x3f, hipStream_t st, bool edges_done)
{ with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { correct_all_impl<NS, GRAV>(g, dt, x3f, st, edges_done); }); }
#if !AA_COOLING
// In the strict build (-ffp-contract=off) the 6-variable gravity k_correct_all<1, true, *, true> holds 256 registers WITH 20 bytes of
// scratch per lane, in either entry (profiles/run3d_kernel_budget.md; the default build holds 256 without).  A spilling kernel is
// not built a second time: with a passive scalar and a static potential the strict library has no entry on the device clock.
bool correct_all_dc_built(int nscal, bool grav) { return AA_FAST_DIV || !(nscal && grav); }
void launch_correct_all_dc(const HostGrid &g, int nscal, const Run3D *rc, bool grav, hipStream_t st)
{ with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { correct_all_impl<NS, GRAV>(g, 0.0, true, st, false, rc); }); }
void launch_sweep_x2_dc(const HostGrid &g, int nscal, const Run3D *rc, bool grav, hipStream_t st)
{ with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { sweep_impl<NS, GRAV, MODE_FLUX1>(g, g.U, 1, 0.0, st, 0, -1, rc); }); }
#endif

void launch_slopes(const HostGrid &g, int nscal, int dir, hipStream_t st, const Real *src)
{ if (!src) src = g.U; with_ns(nscal, [&](auto NS) { slopes_impl<NS>(g, dir, st, src); }); }

void launch_sweep(const HostGrid &g, int nscal, int dir, Real dt, bool grav, hipStream_t st, int koff, int kcnt)
{ with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { sweep_impl<NS, GRAV, MODE_FLUX1>(g, g.U, dir, dt, st, koff, kcnt); }); }
// x1 first pass + x1 correct pass in one sweep (must run after the x2 and x3 first passes)
void launch_sweep_correct_x1(const HostGrid &g, int nscal, Real dt, bool grav, hipStream_t st)
{ with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { sweep_impl<NS, GRAV, MODE_BOTH>(g, g.U, 0, dt, st); }); }
// CTU steps 5-7, 8a, 9a for the faces of one direction (after all three first-pass sweeps)
void launch_correct(const HostGrid &g, int nscal, int dir, Real dt, bool grav, hipStream_t st)
{ with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { sweep_impl<NS, GRAV, MODE_CORR>(g, g.U, dir, dt, st); }); }
// VL second-order fluxes: PLM without tracing on U^{n+1/2} (kept in LR[0][L]), etah = 0
void launch_vl_flux2(const HostGrid &g, int nscal, int dir, Real dt, hipStream_t st)
{ with_ns(nscal, [&](auto NS) { sweep_impl<NS, false, MODE_VL>(g, g.LR, dir, dt, st); }); }      // (no gravity kick in the states: GRAV = false only)
void launch_vl_flux1(const DevGrid &g, int nscal, int dir, hipStream_t st)
{
  long n[3] = {g.N1, g.N2, g.N3}; n[dir] -= 1;
  dim3 grid(nblk(n[0]*n[1]*n[2], 256)), blk(256);
  with_ns(nscal, [&](auto NS) { with_dir(dir, [&](auto D) { hipLaunchKernelGGL((k_vl_flux1<NS, D>), grid, blk, 0, st, g); }); });
}
// donor-cell fluxes + U^{n+1/2} in one kernel (what launch_vl_flux1 x3 + launch_vl_uhalf do)
void launch_vl_predict(const HostGrid &g, int nscal, Real dt, bool grav, hipStream_t st)
{
  const int ni = g.ie - g.is + 7, nj = g.je - g.js + 7, nk = g.ke - g.ks + 7;
  int kc = g.cfg.vp_kc > 0 ? g.cfg.vp_kc : 32;                             // (AA_VP_KC overrides)
  if (g.cfg.vp_kc <= 0) while (kc > 4 && (long)nblk(ni, 63)*nblk(nj, VP_TJ - 1)*((nk + kc - 1)/kc) < 1024) kc >>= 1;
  dim3 grid(nblk(ni, 63), nblk(nj, VP_TJ - 1), (nk + kc - 1)/kc), blk(64, VP_TJ);
  with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { hipLaunchKernelGGL((k_vl_predict<NS, GRAV>), grid, blk, 0, st, g, dt, kc); });
}
void launch_vl_uhalf(const DevGrid &g, int nscal, Real dt, bool grav, hipStream_t st)
{
  const long n = (long)(g.ie - g.is + 7)*(g.je - g.js + 7)*(g.ke - g.ks + 7);
  dim3 grid(nblk(n, 256)), blk(256);
  with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { hipLaunchKernelGGL((k_vl_uhalf<NS, GRAV>), grid, blk, 0, st, g, dt); });
}

void launch_flux2(const HostGrid &g, int nscal, int dir, hipStream_t st)
{
  const long n = (long)(g.ie - g.is + 1 + (dir == 0))*(g.je - g.js + 1 + (dir == 1))*(g.ke - g.ks + 1 + (dir == 2));
  dim3 grid(nblk8(n, 256)), blk(256);
  with_ns(nscal, [&](auto NS) { with_dir(dir, [&](auto D) { hipLaunchKernelGGL((k_flux2<NS, D>), grid, blk, 0, st, g, zone_order(g)); }); });
}

void launch_pinned_cfl(const DevGrid &g, long long n, const long long *idx, DevScalars *sc, hipStream_t st)
{ if (n > 0) { unsigned nb = nblk(n, 256*8); if (nb > 256) nb = 256; if (nb < 1) nb = 1;
               hipLaunchKernelGGL(k_pinned_cfl, dim3(nb), dim3(256), 0, st, g, n, idx, sc); } }
void launch_pin_mask(const DevGrid &g, long long n, const long long *idx, unsigned char *mask, hipStream_t st)
{ if (n > 0) hipLaunchKernelGGL(k_pin_mask, dim3(nblk(n, 256)), dim3(256), 0, st, g, n, idx, mask); }
// fused second-pass fluxes + update (CTU); `keep`: the face planes whose fluxes are stored as well; sc: and new_dt's maxima
// The instances of k_flux2_update_keep_dc this build has: one that needs scratch is not built (flux2_update_keep_dc_built; the
// figures are in profiles/mesh_run3d_kernel_budget.md), and a Mesh with such a level steps one aa_mesh_step at a time.
#define AA_FLUX2_KEEP_DC_BUILT(NS, GRAV) true
static void flux2_update_impl(const HostGrid &g, int nscal, Real dt, bool grav, const KeepPlanes *keep, hipStream_t st, DevScalars *sc, const unsigned char *pinmask,
                              const Run3D *rc)
{
  // (rc: a queued step -- the same launch, dt and the ratios from the device clock; no pinned zones.  A stand-alone Grid: no kept
  //  planes, always sc; a level of a Mesh: `keep`, sc only where the Grid has no child)
  const int ni = g.ie - g.is + 1, nj = g.je - g.js + 1, nk = g.ke - g.ks + 1;
  const int kc_env = g.cfg.fu_kc;
  int kc = kc_env > 0 ? kc_env : 32;
  if (kc_env <= 0) while (kc > 4 && (long)nblk(ni, 64)*nblk(nj, FU_TJ - 1)*((nk + kc - 1)/kc) < 1024) kc >>= 1;
  dim3 grid(nblk(ni, 64), nblk(nj, FU_TJ - 1), (nk + kc - 1)/kc), blk(64, FU_TJ);
#if !AA_COOLING
  if (rc && keep) {
    const KeepPlanes kpd = *keep;
    with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { with_flag(sc != nullptr, [&](auto CFL) {
      // (a combination flux2_update_keep_dc_built() names is not instantiated: aa_mesh_run_3d steps such a Mesh one aa_mesh_step at a time)
      if constexpr (AA_FLUX2_KEEP_DC_BUILT(NS, GRAV))
        hipLaunchKernelGGL((k_flux2_update_keep_dc<NS, GRAV, true, CFL>), grid, blk, 0, st, g, g.dhalf, rc, kc, sc, kpd);
      else abort(); }); });
    return;
  }
  if (rc) { with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { hipLaunchKernelGGL((k_flux2_update_dc<NS, GRAV, false, true>), grid, blk, 0, st, g, g.dhalf, rc, kc, sc); }); return; }
#endif
  const bool keeps = keep && keep->n;
  const KeepPlanes kp = keeps ? *keep : KeepPlanes{0, {{0}}};
  with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { with_flag(keeps, [&](auto KEEP) { with_flag(sc != nullptr, [&](auto CFL) {
    hipLaunchKernelGGL((k_flux2_update<NS, GRAV, KEEP, CFL>), grid, blk, 0, st, g, g.dhalf, dt, kc, kp, sc, pinmask, step_ratios(g, dt)); }); }); });
}
void launch_flux2_update(const HostGrid &g, int nscal, Real dt, bool grav, const KeepPlanes *keep, hipStream_t st, DevScalars *sc, const unsigned char *pinmask)
{ flux2_update_impl(g, nscal, dt, grav, keep, st, sc, pinmask, nullptr); }
#if !AA_COOLING
void launch_flux2_update_dc(const HostGrid &g, int nscal, const Run3D *rc, bool grav, DevScalars *sc, hipStream_t st)
{ flux2_update_impl(g, nscal, 0.0, grav, nullptr, st, sc, nullptr, rc); }
// ... of a level of a Mesh: the second-pass fluxes on the planes of `kp` stay in F; sc == nullptr: without new_dt's maxima
bool flux2_update_keep_dc_built(int nscal, bool grav) { return nscal ? (grav ? AA_FLUX2_KEEP_DC_BUILT(1, true) : AA_FLUX2_KEEP_DC_BUILT(1, false)) : (grav ? AA_FLUX2_KEEP_DC_BUILT(0, true) : AA_FLUX2_KEEP_DC_BUILT(0, false)); }
void launch_flux2_update_keep_dc(const HostGrid &g, int nscal, const Run3D *rc, bool grav, DevScalars *sc, const KeepPlanes &kp, hipStream_t st)
{ flux2_update_impl(g, nscal, 0.0, grav, &kp, st, sc, nullptr, rc); }
#endif

long update_blocks(const DevGrid &g)
{ return (long)nblk8((long)(g.ie - g.is + 1)*(g.je - g.js + 1)*(g.ke - g.ks + 1), 256); }
// the per-block maxima of an update with CFL -> sc (one launch behind it)
static void cfl_fold(Real *cfl_part, unsigned nblocks, DevScalars *sc, hipStream_t st)
{
  unsigned nf = nblk(nblocks, 256*8); if (nf > 256) nf = 256;
  hipLaunchKernelGGL(k_cfl_fold, dim3(nf), dim3(256), 0, st, cfl_part, (int)nblocks, sc);
}
// sc != nullptr: new_dt's maxima ride on the update (cfl_part: 3 * update_blocks(g) doubles of scratch; pinmask: zones left out)
void launch_update(const HostGrid &g, int nscal, const Real *dhalf, Real dt, bool grav, hipStream_t st, DevScalars *sc, Real *cfl_part,
                   const unsigned char *pinmask)
{
  const long n = (long)(g.ie - g.is + 1)*(g.je - g.js + 1)*(g.ke - g.ks + 1);
  dim3 grid(nblk8(n, 256)), blk(256);
  const bool cfl = sc && cfl_part;
  if (!cfl) { cfl_part = nullptr; pinmask = nullptr; }
  with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { with_flag(cfl, [&](auto CFL) {
    hipLaunchKernelGGL((k_update<NS, GRAV, CFL>), grid, blk, 0, st, g, dhalf, dt, zone_order(g), cfl_part, pinmask); }); });
  if (cfl) cfl_fold(cfl_part, grid.x, sc, st);
}

#if !AA_COOLING
void launch_update_fofc(const HostGrid &g, int nscal, const Real *dhalf, Real dt, bool grav, hipStream_t st, DevScalars *sc_cfl,
                        Real *cfl_part, const unsigned char *pinmask, DevScalars *sc, long long *list)
{
  const long n = (long)(g.ie - g.is + 1)*(g.je - g.js + 1)*(g.ke - g.ks + 1);
  dim3 grid(nblk8(n, 256)), blk(256);
  const bool cfl = sc_cfl && cfl_part;
  if (!cfl) { cfl_part = nullptr; pinmask = nullptr; }
  with_ns_grav(nscal, grav, [&](auto NS, auto GRAV) { with_flag(cfl, [&](auto CFL) {
    hipLaunchKernelGGL((k_update_fofc<NS, GRAV, CFL>), grid, blk, 0, st, g, dhalf, dt, zone_order(g), cfl_part, pinmask, sc, list); }); });
  if (cfl) cfl_fold(cfl_part, grid.x, sc_cfl, st);
}
void launch_fofc_fix(const DevGrid &g, int nscal, const Real *un, Real dt, DevScalars *sc, long long *list, hipStream_t st)
{ with_ns(nscal, [&](auto NS) { hipLaunchKernelGGL(k_fofc_fix<NS>, dim3(1), dim3(64), 0, st, g, un, dt, sc, list); }); }
void launch_fofc_nanfix(const DevGrid &g, int nscal, int dir, const Real *un, DevScalars *sc, hipStream_t st)
{
  long n[3] = {g.ie - g.is + 3, g.je - g.js + 3, g.ke - g.ks + 3}; n[dir] -= 1;
  dim3 grid(nblk(n[0]*n[1]*n[2], 256)), blk(256);
  with_ns(nscal, [&](auto NS) { with_dir(dir, [&](auto D) { hipLaunchKernelGGL((k_fofc_nanfix<NS, D>), grid, blk, 0, st, g, un, sc); }); });
}
#endif

void launch_bc(const DevGrid &g, int nscal, int dir, int side, int flag, hipStream_t st)
{
  const int lo3[3] = {g.is, g.js, g.ks}, hi3[3] = {g.ie, g.je, g.ke}, N[3] = {g.N1, g.N2, g.N3};
  long n = 1;
  for (int a = 0; a < 3; a++) n *= (a == dir) ? 4 : (a < dir ? N[a] : hi3[a] - lo3[a] + 1);
  hipLaunchKernelGGL(k_bc, dim3(nblk(n, 256)), dim3(256), 0, st, g, 5 + nscal, dir, side, flag, 0);
}
// the two sides of one direction never read each other's ghost zones (sources are active zones along
// `dir`, bvals_mhd.c:959-2317): one launch for both
void launch_bc_dir(const DevGrid &g, int nscal, int dir, int flag_in, int flag_out, hipStream_t st)
{
  if (!flag_in && !flag_out) return;
  const int lo3[3] = {g.is, g.js, g.ks}, hi3[3] = {g.ie, g.je, g.ke}, N[3] = {g.N1, g.N2, g.N3};
  long n = 1;
  for (int a = 0; a < 3; a++) n *= (a == dir) ? 4 : (a < dir ? N[a] : hi3[a] - lo3[a] + 1);
  hipLaunchKernelGGL(k_bc, dim3(nblk(n, 256), 2), dim3(256), 0, st, g, 5 + nscal, dir, -1, flag_in, flag_out);
}

void launch_bc_shell(const DevGrid &g, int nscal, const int flags[6], hipStream_t st)
{
  const long G2 = 2*AA_NGHOST_, nk = g.ke - g.ks + 1, nj = g.je - g.js + 1;
  const long n = G2*g.N2*g.N1 + G2*g.N1*nk + G2*nj*nk;
  hipLaunchKernelGGL(k_bc_shell, dim3(nblk(n, 256)), dim3(256), 0, st, g, 5 + nscal, flags[0], flags[1], flags[2], flags[3], flags[4], flags[5]);
}
void launch_cfl(const DevGrid &g, DevScalars *sc, hipStream_t st)
{
  const long n = (long)(g.ie - g.is + 1)*(g.je - g.js + 1)*(g.ke - g.ks + 1);
  const unsigned nb = reduce_blocks(n);
  hipLaunchKernelGGL(k_cfl, dim3(nb), dim3(256), 0, st, g, sc);
}

int launch_history(const DevGrid &g, int nscal, Real *partial, hipStream_t st)
{
  const long n = (long)(g.ie - g.is + 1)*(g.je - g.js + 1)*(g.ke - g.ks + 1);
  unsigned nb = nblk(n, 256); if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(k_history, dim3(nb), dim3(256), 0, st, g, nscal, partial);
  return (int)nb;
}

void launch_aos_to_soa(const DevGrid &g, int nvar, const Real *aos, hipStream_t st)
{ const long n = (long)g.N1*g.N2*g.N3; hipLaunchKernelGGL(k_aos_to_soa, dim3(nblk(n, 256)), dim3(256), 0, st, g, nvar, aos); }
void launch_soa_to_aos(const DevGrid &g, int nvar, Real *aos, hipStream_t st)
{ const long n = (long)g.N1*g.N2*g.N3; hipLaunchKernelGGL(k_soa_to_aos, dim3(nblk(n, 256)), dim3(256), 0, st, g, nvar, aos); }
void launch_pinned(const DevGrid &g, int nvar, long long n, const long long *idx, const Real *vals, hipStream_t st, DevScalars *sc)
{
  if (n <= 0) return;
  if (sc) { unsigned nb = nblk(n, 256*8); if (nb > 256) nb = 256; if (nb < 1) nb = 1;
            hipLaunchKernelGGL(k_pinned_with_cfl, dim3(nb), dim3(256), 0, st, g, nvar, n, idx, vals, sc); }
  else hipLaunchKernelGGL(k_pinned, dim3(nblk(n, 256)), dim3(256), 0, st, g, nvar, n, idx, vals);
}
void launch_pack_x3(const DevGrid &g, int nvar, int k0, Real *buf, hipStream_t st)
{ const long n = (long)g.N1*g.N2*4; hipLaunchKernelGGL(k_pack_x3, dim3(nblk(n, 256)), dim3(256), 0, st, g, nvar, k0, buf); }
void launch_unpack_x3(const DevGrid &g, int nvar, int k0, const Real *buf, hipStream_t st)
{ const long n = (long)g.N1*g.N2*4; hipLaunchKernelGGL(k_unpack_x3, dim3(nblk(n, 256)), dim3(256), 0, st, g, nvar, k0, buf); }
void launch_pack_x2(const DevGrid &g, int nvar, int j0, Real *buf, hipStream_t st)
{ const long n = (long)g.N1*4*(g.ke - g.ks + 1); hipLaunchKernelGGL(k_pack_x2, dim3(nblk(n, 256)), dim3(256), 0, st, g, nvar, j0, buf); }
void launch_unpack_x2(const DevGrid &g, int nvar, int j0, const Real *buf, hipStream_t st)
{ const long n = (long)g.N1*4*(g.ke - g.ks + 1); hipLaunchKernelGGL(k_unpack_x2, dim3(nblk(n, 256)), dim3(256), 0, st, g, nvar, j0, buf); }

void launch_test_fluxes(int nscal, Real gamma, int n, const Real *Ul, const Real *Ur, const Real *eta, Real *F, hipStream_t st)
{
  with_ns(nscal, [&](auto NS) { hipLaunchKernelGGL((k_test_fluxes<NS>), dim3(nblk(n, 128)), dim3(128), 0, st, gamma, n, Ul, Ur, eta, F); });
}
void launch_test_lr_ppm(int nscal, Real gamma, int n, const Real *W, Real dt, Real dx, int il, int iu, Real *Wl, Real *Wr, hipStream_t st)
{
  const int nc = iu - il + 3;
  with_ns(nscal, [&](auto NS) { hipLaunchKernelGGL((k_test_lr_ppm<NS>), dim3(nblk(nc, 128)), dim3(128), 0, st, gamma, n, W, dt, dx, il, iu, Wl, Wr); });
}
void launch_test_lr(int nscal, Real gamma, int n, const Real *W, Real dt, Real dx, int il, int iu, Real *Wl, Real *Wr, hipStream_t st)
{
  (void)n;
  const int nc = iu - il + 3;
  with_ns(nscal, [&](auto NS) { hipLaunchKernelGGL((k_test_lr<NS>), dim3(nblk(nc, 128)), dim3(128), 0, st, gamma, n, W, dt, dx, il, iu, Wl, Wr); });
}

}  // namespace aa / aa_cool
