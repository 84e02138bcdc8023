// correct_all_kernels.h -- k_x1_edge_flux and k_correct_all of hydro_kernels.hip (which says what they do, in front of its two
// #include lines).  No include guard: the file is compiled twice, for the two entry points of either kernel --
//   as it stands          k_x1_edge_flux(g, dt), k_correct_all(g, dt, kchunk, sr): dt and the StepRatios are kernel arguments
//   AA_CLOCK_ENTRY        k_x1_edge_flux_dc(g, rc), k_correct_all_dc(g, rc, kchunk): one uniform load of `live` and dt from the
//                         device clock (hydro3d_launch.h Run3D) at the top, then the ratios by uniform loads; a step queued behind
//                         the stop returns there, before any store and before any barrier (the whole grid takes the same branch).
//                         Only X3F = true is instantiated: the queued chain is the default one.
// Below the opening brace the two are one text.
template <int NS, bool GRAV, int ORD>
__global__ void __launch_bounds__(64)
#ifdef AA_CLOCK_ENTRY
k_x1_edge_flux_dc(DevGrid g, const Run3D *rc)
{
  if (!rc->c.live) return;
  const Real dt = rc->c.dt;
#else
k_x1_edge_flux(DevGrid g, Real dt)
{
#endif
  // lanes along j: the stores on whole lines (the loads are one sector per zone pair either way)
  const int j = g.js - 1 + blockIdx.x*64 + threadIdx.x, k = g.ks - 1 + blockIdx.y, b = 1 + blockIdx.z;
  if (j > g.je + 1) return;
  const int nbe = x1_edges(g), i0 = g.is - 16 + 64*b;
  // (zone i0-1 as the fields moved one zone down: its x1 neighbours stay in the immediates)
  const ZStr z = zone_strides(g);
  const unsigned mb = zone_off((long)k*g.sK + (long)j*g.sJ + i0);
  Real wa[6], wb[6], wc[6], wd[6], wl[6], wr[6], wx[6];
  load_prim_sweep<NS, 0>(g, z, mb, -2, wa); load_prim_sweep<NS, 0>(g, z, mb, -1, wb);
  load_prim_sweep<NS, 0>(g, z, mb, 0, wc);  load_prim_sweep<NS, 0>(g, z, mb, 1, wd);
  cell_recon<NS, 0, GRAV, ORD>(g, z, -8L, mb, dt, wa, wb, wc, wl, wx);      // zone i0-1: its left state belongs to face i0
  cell_recon<NS, 0, GRAV, ORD>(g, z, 0L, mb, dt, wb, wc, wd, wx, wr);       // zone i0: its right state
  Real ul[6], ur[6], f[6];
  prim_to_cons<NS>(wl, ul, g.Gamma_1, g.rGamma_1);
  prim_to_cons<NS>(wr, ur, g.Gamma_1, g.rGamma_1);
  flux_roe<NS>(ul, ur, wl, wr, 0.0, g.Gamma, g.Gamma_1, f);
  // (the edge array is [variable][edge][k][j]: the variable on the base, the rest -- 1/64 of a field -- in the offset)
  unsigned ev8 = (unsigned)nbe*(unsigned)g.N3*(unsigned)g.N2*8u;
  asm volatile("" : "+s"(ev8));
  const unsigned eb = zone_off(x1_edge_index(g, nbe, 0, b, j, k));
  Real fg[6];
#pragma unroll
  for (int n = 0; n < 6; n++) fg[gv<0>(n)] = f[n];
  FBase fb = (FBase)g.F;
#pragma unroll
  for (int v = 0; v < 5 + NS; v++) { zpw(fb, eb)[0] = fg[v]; fb = fup(fb, ev8); }
}
template <int NS, bool GRAV, int ORD, bool X3F>
__global__ void __launch_bounds__(64*CA_TJ, (X3F && NS && GRAV) ? 2 : 1)
#ifdef AA_CLOCK_ENTRY
k_correct_all_dc(DevGrid g, const Run3D *rc, int kchunk)
{
  if (!rc->c.live) return;
  const Real dt = rc->c.dt;
  const StepRatios sr = clock_ratios(rc);
#else
k_correct_all(DevGrid g, Real dt, int kchunk, StepRatios sr)
{
#endif
  __shared__ Real s_w[CA_TJ][6][64];
  __shared__ Real s_l[CA_TJ][64];
  // X3F: the x3 states of zone k+1 wait here while zone k is corrected (each thread its own slots, no barrier): 24
  // registers that the 6-variable gravity kernel does not have at 2 waves per SIMD (it spilled 16 to scratch)
  // (with the x1 first pass on board: two sets of 12 slots taken in turn, so that the states of zone k need no registers
  //  between the iterations nor under the x1 Riemann problem: they are read where they are used)
  __shared__ Real s_park[X3F ? 24 : 1][CA_TJ][64];
  // ... and in the 6-variable gravity kernel, which spilled three registers, the x1 / x2 frame pressures of planes k+1 and k+2 wait
  // there too (each thread its own slots): no scratch, 18.53 -> 18.18 ms at 512^3 (same-box ABAB x 3 against keeping them in registers)
  constexpr bool PARK2 = X3F && NS && GRAV;
  __shared__ Real s_pp[PARK2 ? 4 : 1][CA_TJ][64];
  // The zones a tile needs from its neighbours (lane 0's lower / lane 63's upper x1 neighbour, row 0's lower / row CA_TJ-1's
  // upper x2 neighbour) are requested at the head of the iteration with everything else and wait here for their block: a load
  // issued inside a block would have to wait for the face-state stores of the block before it (loads and stores retire
  // through one counter).  s_h1: per wave, the 6 + 6 conserved variables of the two x1 neighbours, fetched by lanes 0..11.
  // X1F: and behind them the first-pass x1 fluxes of the tile's two edge faces (lanes 12..23)
  constexpr bool X1F = X3F;      // the x1 first pass comes with the x3 one; the name marks what belongs to which
  __shared__ Real s_h1[CA_TJ][X1F ? 24 : 12];
  __shared__ Real s_h2[2][6][64];
  constexpr int NV = 5 + NS;
  const int lane = threadIdx.x, row = threadIdx.y;
  // Zones s-1 .. e+1 in every direction get their face states.  Tiles do NOT overlap in x1 / x2 (round 1's did by one
  // provider lane / row: 64x4 threads for 63x3 zones, 35 % more threads, loads and arithmetic than zones) and start on a
  // 128-byte line (zone is - 16: the rows' first active zone is line-aligned).  What a tile cannot do alone is the eta of
  // its own lowest x1 / x2 faces (lane 0, row 0), which needs lambda_l of the zone in the tile before: there the zone
  // stores its lambda_r in the face's eta slot, the zone before (lane 63 / row CA_TJ-1) its lambda_l in an edge array,
  // and k_eta_edges turns the pairs into etas afterwards (1/64 + 1/CA_TJ of the faces, < 10 B/zone).
  // (Tried and dropped: an XCD-aware blockIdx -> tile map that gives each XCD one contiguous run of tiles, so that the tiles
  //  either side of an edge share an L2.  Measured ABAB at 512^3: 21.3 vs 20.3 ms here, 15.1 vs 14.9 ms in k_flux2_update —
  //  the plain map, which spreads neighbouring tiles over all eight XCDs and memory channels, is the faster one.)
  const int i = g.is - 16 + blockIdx.x*64 + lane, j = g.js - 1 + blockIdx.y*CA_TJ + row;
  const int k0 = g.ks - 1 + blockIdx.z*kchunk;
  int k1 = k0 + kchunk - 1; if (k1 > g.ke + 1) k1 = g.ke + 1;
  const int kstart = (blockIdx.z == 0) ? k0 : k0 - 1;          // one provider plane below a later chunk
  // idle threads beyond the Grid keep valid addresses (their neighbours may read what they load)
  // (X1F: zone ie+2 gives its right state to the first-pass flux of face ie+2, so the lane of zone ie+3 holds that zone)
  const int imax = g.ie + (X1F ? 3 : 2);
  const int ic = (i <= imax) ? (i < 0 ? 0 : i) : imax, jc = (j <= g.je + 2) ? j : g.je + 2;
  const long mcol = (long)jc*g.sJ + ic;
  const int iW = i - lane, iE = i - lane + 63;                 // lane 0's and lane 63's zone, clamped like ic
  const int icW = (iW <= imax) ? (iW < 0 ? 0 : iW) : imax, icE = (iE <= imax) ? (iE < 0 ? 0 : iE) : imax;
  const int nbe = x1_edges(g);
  const bool in = (i >= g.is - 1) && (i <= g.ie + 1) && (j <= g.je + 1);
  const bool do1 = in, do2 = in, do3 = in;
  Real q[3];
#pragma unroll
  for (int d = 0; d < 3; d++) q[d] = sr.q[d];

  // X3F: the x3 FIRST pass rides on the march (k_sweep_march<2> is not launched, its fluxes never reach HBM): the
  // transverse differences a zone needs of the x3 first-pass flux are those of its own column, and the reconstruction
  // + gravity kick of a zone along x3 is the same for the first pass and for the correct pass.  Iteration k
  // reconstructs zone k+1 (A), solves face k+1 from the left state zone k kept and the right state of zone k+1 (B),
  // and then corrects zone k in all three directions (C).  A chunk starts two planes early with A only, then A + B: one
  // instance of every piece of arithmetic, whatever the chunking (see k_sweep_march).
  // The window: wc = zone k, wn = k+1 (and wm3 = k-1 without X3F, wn2 = k+2 with it).
  Real wm3[6], wc[6], wn[6], wn2[6], pc0 = 0.0, pc1 = 0.0, pn0, pn1, pn20 = 0.0, pn21 = 0.0, f3[6], lam3 = 0.0;
  Real wl3[6], wr3[6];                                          // X3F: kicked x3 states of zone k (left -> face k+1, right -> face k)
  const int kbeg = X3F ? kstart - 2 : kstart;
  if (X3F) {
    load_prim3<NS>(g, (long)kbeg*g.sK + mcol, wn, pn0, pn1);
    load_prim3<NS>(g, (long)(kbeg + 1)*g.sK + mcol, wn2, pn20, pn21);
    if constexpr (PARK2) { s_pp[0][row][lane] = pn0; s_pp[1][row][lane] = pn1; s_pp[2][row][lane] = pn20; s_pp[3][row][lane] = pn21; }
#pragma unroll
    for (int v = 0; v < 6; v++) { f3[v] = 0.0; wl3[v] = 1.0; wr3[v] = 1.0; wc[v] = 1.0; }
  } else {
    load_prim3<NS>(g, (long)(kstart - 1)*g.sK + mcol, wc, pn0, pn1);
    load_prim3<NS>(g, (long)kstart*g.sK + mcol, wn, pn0, pn1);
#pragma unroll
    for (int v = 0; v < 6; v++) f3[v] = (v < NV) ? Ff(g, 2, v)[(long)kstart*g.sK + mcol] : 0.0;
  }
#pragma nounroll
  for (int k = kbeg; k <= k1; k++) {
    const ZStr z = zone_strides(g);               // the scalar-base accessors (hydro_kernels.hip, field accessors)
    const unsigned mb = zone_off((long)k*g.sK + mcol);      // one 32-bit offset for all fields (see k_flux2_update)
    const bool full = (k >= k0);                  // block-uniform; the provider plane does x3 only
    const int pk = (k & 1) ? 12 : 0;              // X3F: the s_park slots of zone k (those of zone k+1: 12 - pk)
    const bool zone = (k >= kstart);              // block-uniform; X3F: the two planes before do the first pass only
    Real f3n[6], wlN[6], wrN[6];
#pragma unroll
    for (int v = 0; v < 6; v++) { f3n[v] = 0.0; wlN[v] = 1.0; wrN[v] = 1.0; }
    // first-pass fluxes across the zone
    CellFlux cf;
#pragma unroll
    for (int v = 0; v < 6; v++) { cf.dF[0][v] = 0.0; cf.dF[1][v] = 0.0; cf.dF[2][v] = 0.0; }
    Real mlo[3], mhi[3];
    Real hv1 = 0.0;
    // What the zone needs behind its x1 Riemann problem is requested in front of it where the registers allow: the wait would
    // otherwise come behind it with nothing left to do.  So the x2 first-pass fluxes are: k_correct_all 22.6 -> 20.2 ms at 512^3, three
    // registers in scratch.  (The potentials and the x2 neighbour rows as well: tens of registers in scratch, a loss -- also with the
    // potentials parked in LDS; profiles/r04_x1f_ab.txt.)  The scalar kernel without gravity (ifront) has no room for it at two waves
    // per SIMD and requests them where they are used.
    constexpr bool EARLY_F = X1F && !(NS && !GRAV);
    Real hv2[6];
#pragma unroll
    for (int v = 0; v < 6; v++) hv2[v] = 0.0;
    const bool edge_row = (row == 0) || (row == CA_TJ - 1);
    // the x1 neighbour zones and edge fluxes of plane kk (lanes 0..23 of every wave)
    auto x1_halo = [&](int kk) -> Real {
      Real h = 0.0;
      if (lane < 12) {
        const int v = lane % 6, east = lane / 6;
        if (v < NV) h = Uf(g, v)[(long)kk*g.sK + (long)jc*g.sJ + (east ? icE + 1 : icW - 1)];
      } else if (lane < 24) {
        const int v = (lane - 12) % 6, b = (int)blockIdx.x + (lane - 12)/6;      // the tile's lower edge face, then its upper one
        if (v < NV && b >= 1 && b <= nbe) h = g.F[x1_edge_index(g, nbe, v, b, jc, kk)];
      }
      return h;
    };
    // requested here, used behind the x3 first pass (the provider plane too: its x3 states take x1 fluxes made here)
    if (X1F && zone) hv1 = x1_halo(k);
    if (X3F) {
#pragma unroll
      for (int n = 0; n < 6; n++) { wc[n] = wn[n]; wn[n] = wn2[n]; }
      if constexpr (PARK2) { pc0 = s_pp[0][row][lane]; pc1 = s_pp[1][row][lane]; s_pp[0][row][lane] = s_pp[2][row][lane]; s_pp[1][row][lane] = s_pp[3][row][lane]; }
      else { pc0 = pn0; pc1 = pn1; pn0 = pn20; pn1 = pn21; }
      load_prim3<NS>(g, z, 2L*z.sK8, mb, wn2, pn20, pn21);
      if constexpr (PARK2) { s_pp[2][row][lane] = pn20; s_pp[3][row][lane] = pn21; }
      if (do3) {
        {   // (A) zone k+1 along x3
          Real wm[6], ws[6], wp[6];
          to_sweep<2>(wc, wc[4], wm); to_sweep<2>(wn, wn[4], ws); to_sweep<2>(wn2, wn2[4], wp);
          cell_recon<NS, 2, GRAV, ORD>(g, z, (long)z.sK8, mb, dt, sr.dtodx[2], wm, ws, wp, wlN, wrN);
        }
        // (the states of zone k+1 go to their slots before (B): the left one is not needed in it)
#pragma unroll
        for (int n = 0; n < NV; n++) { s_park[12 - pk + n][row][lane] = wlN[n]; s_park[12 - pk + 6 + n][row][lane] = wrN[n]; }
        if (k >= kstart - 1) {   // (B) first-pass flux of face k+1 (face_work<MODE_FLUX1>), sweep frame -> global variables
          Real ul[6], ur[6], f[6];
#pragma unroll
          for (int n = 0; n < 6; n++) wl3[n] = (n < NV) ? s_park[pk + n][row][lane] : 0.0;
          prim_to_cons<NS>(wl3, ul, g.Gamma_1, g.rGamma_1);
          prim_to_cons<NS>(wrN, ur, g.Gamma_1, g.rGamma_1);
          flux_roe<NS>(ul, ur, wl3, wrN, 0.0, g.Gamma, g.Gamma_1, f);
#pragma unroll
          for (int n = 0; n < NV; n++) f3n[gv<2>(n)] = f[n];
        }
      }
      if (!do3) {
#pragma unroll
        for (int n = 0; n < NV; n++) { s_park[12 - pk + n][row][lane] = wlN[n]; s_park[12 - pk + 6 + n][row][lane] = wrN[n]; }
      }
      __builtin_amdgcn_sched_barrier(0);
    } else {
#pragma unroll
      for (int n = 0; n < 6; n++) { wm3[n] = wc[n]; wc[n] = wn[n]; }
      pc0 = pn0; pc1 = pn1;
      load_prim3<NS>(g, z, (long)z.sK8, mb, wn, pn0, pn1);
    }
    if (!X1F && full) {
      if (lane < 12) {
        const int v = lane % 6, east = lane / 6;
        if (v < NV) hv1 = Uf(g, v)[(long)k*g.sK + (long)jc*g.sJ + (east ? icE + 1 : icW - 1)];
      }
    }
    Real wl1[6], wr1[6];                          // X1F: the zone's kicked x1 states
#pragma unroll
    for (int v = 0; v < 6; v++) { wl1[v] = 1.0; wr1[v] = 1.0; }
    // X1F: what the zone needs behind its x1 Riemann problem (x2 first-pass fluxes, potentials, the x2 neighbour rows) is requested
    // in front of it -- the wait would otherwise come after it with nothing left to do (EARLY_F; without it: requested where it is used)
    Real eb0[6], eb1[6];
#pragma unroll
    for (int v = 0; v < 6; v++) { eb0[v] = 0.0; eb1[v] = 0.0; }
    if (EARLY_F && zone) {
      FBase b = fbase(g.F, z, 6);
      const unsigned o = zsite(mb, b);
#pragma unroll
      for (int v = 0; v < NV; v++) { eb0[v] = zp(b, o)[0]; eb1[v] = zp(fup(b, z.sJ8), o)[0]; b = fnext(b, z); }
    }
    if (X1F && zone) {   // ---- the x1 first pass, before anything else of the zone is formed: its fluxes correct the x2 and x3 states ----
      if (lane < 24) s_h1[row][lane] = hv1;
      __builtin_amdgcn_sched_barrier(0);
      Real wm[6], wp[6], ws[6];
      to_sweep<0>(wc, pc0, ws);
#pragma unroll
      for (int n = 0; n < 6; n++) { wm[n] = __shfl_up(ws[n], 1); wp[n] = __shfl_down(ws[n], 1); }
      if (lane == 0 || lane == 63) {      // the neighbour zone of the tile before / after, exactly as the sweeps convert it
        Real u[6];
#pragma unroll
        for (int v = 0; v < 6; v++) u[v] = (v < NV) ? s_h1[row][(lane ? 6 : 0) + v] : 0.0;
        Real wh[6];
        cons_to_prim<NS>(u, wh, g.Gamma_1);
#pragma unroll
        for (int v = 0; v < 6; v++) { if (lane == 0) wm[v] = wh[v]; else wp[v] = wh[v]; }
      }
      if (GRAV) {      // (the zone's kicks along x1; formed again with the others below)
        const FBase p1 = fbase(g.phi, z, 1);
        const unsigned o = zsite(mb, p1);
        const Real phic = zp((FBase)g.phi, o)[0], phir = zp(p1, o)[1], phil = zp(p1, o)[0], dtodx = sr.dtodx[0];
        cf.kl[0] = dtodx*(phir - phic); cf.kr[0] = dtodx*(phic - phil);
      }
      cell_recon<NS, 0, GRAV, ORD>(g, z, mb, dt, sr.dtodx[0], cf, wm, ws, wp, wl1, wr1);
      {   // first-pass flux of the zone's upper face (face_work<MODE_FLUX1>): its right state is the lane above's
        Real wrE[6], ul[6], ur[6], f[6];
#pragma unroll
        for (int n = 0; n < 6; n++) wrE[n] = __shfl_down(wr1[n], 1);
        prim_to_cons<NS>(wl1, ul, g.Gamma_1, g.rGamma_1);
        prim_to_cons<NS>(wrE, ur, g.Gamma_1, g.rGamma_1);
        flux_roe<NS>(ul, ur, wl1, wrE, 0.0, g.Gamma, g.Gamma_1, f);
#pragma unroll
        for (int n = 0; n < NV; n++) {
          const Real fu = (lane == 63) ? s_h1[row][18 + gv<0>(n)] : f[n];      // the tile's edge faces: k_x1_edge_flux
          Real flo = __shfl_up(fu, 1);
          if (lane == 0) flo = s_h1[row][12 + gv<0>(n)];
          cf.dF[0][gv<0>(n)] = fu - flo;
          if (gv<0>(n) == 0) { mlo[0] = flo; mhi[0] = fu; }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (full) {
      if (edge_row) {
        // (a wavefront is one thread row: which neighbour row it fetches is uniform and goes on the base)
        FBase b = __builtin_amdgcn_readfirstlane(row) == 0 ? fdn((FBase)g.U, z.sJ8) : fup((FBase)g.U, z.sJ8);
        Real t[6];
        const unsigned o = zsite(mb, b);
#pragma unroll
        for (int v = 0; v < 6; v++) { t[v] = (v < NV) ? zp(b, o)[0] : 0.0; b = fnext(b, z); }
#pragma unroll
        for (int v = 0; v < NV; v++) hv2[v] = t[gv<1>(v)];
      }
    }
    if (zone) {
    FBase fa = (FBase)g.F, fb2 = fbase(g.F, z, 6), fc = fup(fbase(g.F, z, 12), z.sK8);
    const unsigned o = zsite(mb, fb2);
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const Real a0 = X1F ? 0.0 : zp(fa, o)[0], a1 = X1F ? 0.0 : zp(fa, o)[1];
      const Real b0 = EARLY_F ? eb0[v] : zp(fb2, o)[0], b1 = EARLY_F ? eb1[v] : zp(fup(fb2, z.sJ8), o)[0];
      const Real c0 = f3[v], c1 = X3F ? f3n[v] : zp(fc, o)[0];
      fa = fnext(fa, z); fb2 = fnext(fb2, z); fc = fnext(fc, z);
      if (!X1F) cf.dF[0][v] = a1 - a0;
      cf.dF[1][v] = b1 - b0; cf.dF[2][v] = c1 - c0;
      if (v == 0) { if (!X1F) { mlo[0] = a0; mhi[0] = a1; } mlo[1] = b0; mhi[1] = b1; mlo[2] = c0; mhi[2] = c1; }
      if (!X3F) f3[v] = c1;
    }
    if (GRAV) {
      const Real dc = wc[0], phic = zp((FBase)g.phi, o)[0];
      FBase pf = (FBase)g.phi;
#pragma unroll
      for (int e = 0; e < 3; e++) {
        pf = fnext(pf, z);
        const Real phir = (e == 0) ? zp(pf, o)[1] : zp(fup(pf, e == 1 ? z.sJ8 : z.sK8), o)[0], phil = zp(pf, o)[0];
        cf.gm[e] = q[e]*(phir - phil)*dc;
        cf.ge[e] = q[e]*(mlo[e]*(phic - phil) + mhi[e]*(phir - phic));
        const Real dtodx = sr.dtodx[e];
        cf.kl[e] = dtodx*(phir - phic); cf.kr[e] = dtodx*(phic - phil);
      }
    }
    // the neighbour zones go to their (wave-private) LDS slots HERE, before the first face-state store of the iteration: the
    // wait for these loads would otherwise sit behind the x3 block's twelve stores and drain them (loads and stores retire
    // through ONE in-order counter: the ISA had an s_waitcnt vmcnt(0) in the middle of every iteration; 18.5 -> 18.3 ms).
    // (Tried on top and dropped, round 3: the x2 block's -- and the x1 block's -- twelve face states parked in LDS and stored at
    //  the head of the NEXT iteration behind its loads, so that no load wait sits behind fresh stores: 18.6-18.9 / 19.5-19.7
    //  against 18.3-18.5 ms.  The write latency is not what this kernel waits for; it moves its 92 GB at 5 TB/s.)
    if (full) {
      if (!X1F && lane < 12) s_h1[row][lane] = hv1;
      if (edge_row) {
#pragma unroll
        for (int v = 0; v < NV; v++) s_h2[row ? 1 : 0][v][lane] = hv2[v];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (X1F && full) {   // ---- x1: the states reconstructed above take their corrections ----
      Real ll = 0.0, lr = 0.0;
      if (do1) cell_finish<NS, 0, GRAV>(g, z, mb, q, cf, wl1, wr1, true, ll, lr);
      const Real lprev = __shfl_up(ll, 1);
      if (do1) {
        // (lane 0 is the tile edge: k_eta_edges finishes this face)
        if (lane == 0 || i > g.is - 1) zstore((FBase)g.eta, mb, lane > 0 ? 0.5*fabs(lr - lprev) : lr);
        if (lane == 63) zstore(fbase(g.eta, z, 3), mb, ll);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (do3) {   // ---- x3 in front of x2 (and of x1 where the x1 first pass is not on board): what only this block needs (the plane below / the states zone k kept) is dead under the others ----
      Real ll, lr;
      if (X3F) {
#pragma unroll
        for (int n = 0; n < 6; n++) { wl3[n] = (n < NV) ? s_park[pk + n][row][lane] : 0.0; wr3[n] = (n < NV) ? s_park[pk + 6 + n][row][lane] : 0.0; }
      }
      if (X3F) cell_finish<NS, 2, GRAV>(g, z, mb, q, cf, wl3, wr3, full, ll, lr);
      else {
        Real wm[6], ws[6], wp[6];
        to_sweep<2>(wm3, wm3[4], wm); to_sweep<2>(wc, wc[4], ws); to_sweep<2>(wn, wn[4], wp);
        cell_states<NS, 2, GRAV, ORD>(g, z, mb, dt, sr.dtodx[2], q, cf, wm, ws, wp, full, ll, lr);
      }
      if (full && k > g.ks - 1) zstore(fbase(g.eta, z, 2), mb, 0.5*fabs(lr - lam3));      // lam3 = lambda_l the zone below gave to this zone's lower face
      lam3 = ll;
      if ((GRAV || AA_COOLING) && full) {   // d^{n+1/2}, :2104-2125
        const Real dh = wc[0] - q[0]*cf.dF[0][0] - q[1]*cf.dF[1][0] - q[2]*cf.dF[2][0];
        zstore((FBase)g.dhalf, mb, dh);
#if AA_COOLING
        {   // P^{n+1/2}, :2133-2266
          FBase b = fbase(g.U, z, 1);
          Real um[3], ue;
          const unsigned o = zsite(mb, b);
#pragma unroll
          for (int e = 0; e < 3; e++) { um[e] = zp(b, o)[0]; b = fnext(b, z); }
          ue = zp(b, o)[0];
          zpw((FBase)g.phalf, o)[0] = p_half(um, ue, q, cf.dF, GRAV, cf.gm, dh, g.Gamma_1);
        }
#endif
      }
    }
    if (full) {
      if (!X1F) {   // ---- x1: neighbours by shuffle ----
        Real wm[6], wp[6], ws[6], ll = 0.0, lr = 0.0;
        to_sweep<0>(wc, pc0, ws);
#pragma unroll
        for (int n = 0; n < 6; n++) { wm[n] = __shfl_up(ws[n], 1); wp[n] = __shfl_down(ws[n], 1); }
        if (lane == 0 || lane == 63) {      // the neighbour zone of the tile before / after, exactly as the sweeps convert it
          Real u[6];
#pragma unroll
          for (int v = 0; v < 6; v++) u[v] = (v < NV) ? s_h1[row][(lane ? 6 : 0) + v] : 0.0;
          Real wh[6];
          cons_to_prim<NS>(u, wh, g.Gamma_1);
#pragma unroll
          for (int v = 0; v < 6; v++) { if (lane == 0) wm[v] = wh[v]; else wp[v] = wh[v]; }
        }
        if (do1) cell_states<NS, 0, GRAV, ORD>(g, z, mb, dt, sr.dtodx[0], q, cf, wm, ws, wp, true, ll, lr);
        const Real lprev = __shfl_up(ll, 1);
        if (do1) {
          // (lane 0 is the tile edge: k_eta_edges finishes this face)
          if (lane == 0 || i > g.is - 1) zstore((FBase)g.eta, mb, lane > 0 ? 0.5*fabs(lr - lprev) : lr);
          if (lane == 63) zstore(fbase(g.eta, z, 3), mb, ll);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      {   // ---- x2: neighbours through LDS ----
        Real wm[6], wp[6], ws[6], ll = 0.0, lr = 0.0;
        to_sweep<1>(wc, pc1, ws);
#pragma unroll
        for (int n = 0; n < NV; n++) s_w[row][n][lane] = ws[n];
        __syncthreads();
        if (row == 0) {
          Real u[6];
#pragma unroll
          for (int v = 0; v < 6; v++) u[v] = (v < NV) ? s_h2[0][v][lane] : 0.0;
          cons_to_prim<NS>(u, wm, g.Gamma_1);
        } else {
#pragma unroll
          for (int n = 0; n < NV; n++) wm[n] = s_w[row - 1][n][lane];
          if (!NS) wm[5] = 0.0;
        }
        if (row == CA_TJ - 1) {
          Real u[6];
#pragma unroll
          for (int v = 0; v < 6; v++) u[v] = (v < NV) ? s_h2[1][v][lane] : 0.0;
          cons_to_prim<NS>(u, wp, g.Gamma_1);
        } else {
#pragma unroll
          for (int n = 0; n < NV; n++) wp[n] = s_w[row + 1][n][lane];
          if (!NS) wp[5] = 0.0;
        }
        if (do2) cell_states<NS, 1, GRAV, ORD>(g, z, mb, dt, sr.dtodx[1], q, cf, wm, ws, wp, true, ll, lr);
        s_l[row][lane] = ll;
        __syncthreads();
        if (do2) {
          // (row 0 is the tile edge, as lane 0 for x1)
          if (row > 0 || j > g.js - 1) zstore(fbase(g.eta, z, 1), mb, row > 0 ? 0.5*fabs(lr - s_l[row - 1][lane]) : lr);
          if (row == CA_TJ - 1) zstore(fbase(g.eta, z, 4), mb, ll);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    }
    if (X3F) {
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int n = 0; n < 6; n++) f3[n] = f3n[n];
    }
  }
}
