// flux2_update_kernel.h -- k_flux2_update of hydro_kernels.hip (which says in front of k_sweep_march's #include lines why the kernel
// lives here).  No include guard: compiled three times --
//   as it stands          k_flux2_update(g, dhalf, dt, kchunk, kp, sc, pinmask, sr): dt and the StepRatios are kernel arguments
//   AA_CLOCK_ENTRY 1      k_flux2_update_dc(g, dhalf, rc, kchunk, sc): one uniform load of `live` and dt from the device clock
//                         (hydro3d_launch.h Run3D) at the top, then the ratios by uniform loads; a step queued behind the stop
//                         returns there, before any store and before any barrier (the whole grid takes the same branch).  A
//                         step queued by aa_run_3d keeps no flux planes and has no pinned zones (it refuses a level of a Mesh and
//                         a Grid with pinned zones): instantiated with KEEP = false, CFL = true only.
//   AA_CLOCK_ENTRY 2      k_flux2_update_keep_dc(g, dhalf, rc, kchunk, sc, kp): the same entry for a level of a Mesh
//                         (aa_mesh_run_3d, smr.hip mesh_queue_step_3d) -- the KeepPlanes a kernel argument beside the clock, as in
//                         the by-value entry.  An entry of its own, so that the kernel arguments and with them the device code of
//                         k_flux2_update_dc stay what they were.  Instantiated with KEEP = true; CFL = true for a Grid without
//                         children, CFL = false for one whose new_dt maxima k_cfl takes behind RestrictCorrect.
// Below the opening brace the three are one text.
template <int NS, bool GRAV, bool KEEP, bool CFL>
__global__ void __launch_bounds__(64*FU_TJ)
#ifdef AA_CLOCK_ENTRY
#if AA_CLOCK_ENTRY == 2
k_flux2_update_keep_dc(DevGrid g, const Real *dhalf, const Run3D *rc, int kchunk, DevScalars *sc, KeepPlanes kp)
{
  if (!rc->c.live) return;
#else
k_flux2_update_dc(DevGrid g, const Real *dhalf, const Run3D *rc, int kchunk, DevScalars *sc)
{
  if (!rc->c.live) return;
  const KeepPlanes kp = {0, {{0}}};
#endif
  const Real dt = rc->c.dt;
  const StepRatios sr = clock_ratios(rc);
  const unsigned char *const pinmask = nullptr;
#else
k_flux2_update(DevGrid g, const Real *dhalf, Real dt, int kchunk, KeepPlanes kp, DevScalars *sc, const unsigned char *pinmask, StepRatios sr)
{
#endif
  // (two copies of the exchange arrays, used in turn: ONE barrier per plane instead of a second one that only kept the
  //  next plane's writers off this plane's readers -- 8 wavefronts, a whole CU, wait at every barrier of this block)
  __shared__ Real s_f2[2][FU_TJ][6][64];
  __shared__ Real s_f1e[2][FU_TJ - 1][6], s_f1s[2][FU_TJ - 1][6];
  // The lower x3 flux of the zone -- live across the whole iteration in 12 registers -- waits in the thread's own LDS slots: the
  // 6-variable gravity kernel then holds 246 registers without scratch, and the scaling-free quotients / square roots of the
  // solver (x_div, x_sqrt: hydro_dev.h), which cost it three spilled registers and 4 % before, pay: 13.77 -> 13.45 ms at 512^3
  // (same-box ABAB x 3; parked alone 13.70).
  __shared__ Real s_f3[6][FU_TJ][64];
  const int lane = threadIdx.x, row = threadIdx.y;
  // Tiles of 64 x (FU_TJ - 1) zones; the rows start on a 128-byte line (zone is) and do not overlap in x1: with a stride
  // of 63 zones every 512-byte row request touched a fifth line and 512 zones took 9 tiles (rocprofv3: 559 B/zone fetched
  // for 400 needed).  Every lane solves the LOWER x1 face of its zone; the one face a row lacks, the upper face of lane
  // 63, is solved by the wavefront of the last thread row (which owns no zones: it solves the x2 faces above the tile and
  // would idle during the x1 phase), lane r for zone row r, with the same software pipeline, and handed over through LDS
  // behind the barrier the x2 phase has anyway.
  const int i0 = g.is + blockIdx.x*64;
  const int i = i0 + lane, j0 = g.js + blockIdx.y*(FU_TJ - 1), j = j0 + row;
  const int k0 = g.ks + blockIdx.z*kchunk;
  int k1 = k0 + kchunk - 1; if (k1 > g.ke) k1 = g.ke;
  constexpr int NV = 5 + NS;
  const bool cell = (row < FU_TJ - 1) && (i <= g.ie) && (j <= g.je);
  const bool edge = (row == FU_TJ - 1) && (lane < FU_TJ - 1) && (j0 + lane <= g.je) && (i0 + 64 <= g.ie + 1);   // x1 face i0+64 of row `lane`
  const bool need1 = ((row < FU_TJ - 1) && (j <= g.je) && (i <= g.ie + 1)) || edge;     // lower x1 face of (i,j) / the edge face
  const bool need2 = (i <= g.ie) && (j <= g.je + 1);                                     // lower x2 face of (i,j)
  const bool last = (row < FU_TJ - 1) && (lane == 63) && (i < g.ie + 1);                 // its upper x1 face comes from the edge wavefront
  // clamp the column of idle threads into the Grid so that shuffles / barriers stay uniform
  const int ic = (i <= g.ie + 1) ? i : g.ie + 1, jc = (j <= g.je + 1) ? j : g.je + 1;
  const long mcol = (long)jc*g.sJ + ic;
  // where this thread's x1 face is, relative to its zone: 0, or for the edge wavefront the hop to (i0 + 64, j0 + lane)
  const long m1off = edge ? ((long)(j0 + lane)*g.sJ + (i0 + 64)) - mcol : 0L;
  Real dtodx[3];
#pragma unroll
  for (int d = 0; d < 3; d++) dtodx[d] = sr.dtodx[d];
  // per direction: flux differences (hi - lo) of all components + the two mass fluxes (gravity)
  Real f3lo[6], d1[6], d2[6], d3[6], m1lo = 0.0, m1hi = 0.0, m2lo = 0.0, m2hi = 0.0, m3hi = 0.0;
  // CFL: the thread's running maxima live in LDS (its own three slots), not in registers carried round the loop: the
  // 6-variable gravity kernel has none to spare (6 spilled, 16.1 against 14.0 ms)
  __shared__ Real s_cmx[CFL ? 3 : 1][CFL ? FU_TJ : 1][CFL ? 64 : 1];
  if (CFL) { s_cmx[0][row][lane] = 0.0; s_cmx[1][row][lane] = 0.0; s_cmx[2][row][lane] = 0.0; }
#pragma unroll
  for (int n = 0; n < 6; n++) f3lo[n] = 0.0;
  const bool keep1 = KEEP && need1 && on_plane(kp, 0, edge ? i0 + 64 : i), keep2 = KEEP && need2 && on_plane(kp, 1, j);
  if (cell) {                                                                   // face k0
    const ZStr z = zone_strides(g);               // the scalar-base accessors (hydro_kernels.hip, field accessors)
    const unsigned mb = zone_off((long)k0*g.sK + mcol);
    face_flux2<NS, 2>(g, z, mb, f3lo);
    // (only the first chunk keeps its face k0: every later chunk's is face k1+1 of the chunk below, kept there by the loop's instance of
    //  the solver -- in the default build this instance may contract its multiply-adds differently, and two writers of one word with
    //  last-bit-different values made the flux a level's parent reads depend on which block finished last: round 4, found as a
    //  run-to-run difference of 1e-16 on the levels of a Mesh in the default build)
    if (KEEP && blockIdx.z == 0 && on_plane(kp, 2, k0)) store_sweep<2, NS>(fbase(g.F, z, 12), z, mb, f3lo);
  }
#pragma unroll
  for (int n = 0; n < NV; n++) s_f3[n][row][lane] = f3lo[n];
  // Software pipeline: the operands of the NEXT Riemann problem are requested before the current one is
  // solved (x2's during the x1 solve, x3's during x2's, the next zone's x1's during x3's), so that with two
  // wavefronts per SIMD the memory pipe is not idle while a wavefront computes.
  FaceIn in1, in2;
  {
    const ZStr z = zone_strides(g);
    if (need1) face_load<NS, 0>(g, z, 0L, zone_off((long)k0*g.sK + mcol + m1off), in1);
  }
  for (int k = k0; k <= k1; k++) {
    // (opaque to the optimiser: otherwise every one of the ~60 field pointers becomes its own
    //  strength-reduced 64-bit induction variable and the kernel spills)
    // One 32-bit byte offset for all fields, and the strides by which the fields' scalar bases are formed where they are used
    // (hydro_kernels.hip, field accessors); mb1: the offset of this thread's x1 face (the edge wavefront's is in another row)
    const ZStr z = zone_strides(g);
    const unsigned mb = zone_off((long)k*g.sK + mcol), mb1 = zone_off((long)k*g.sK + mcol + m1off);
    const int pb = k & 1;
    if (need2) face_load<NS, 1>(g, z, 0L, mb, in2);
    __builtin_amdgcn_sched_barrier(0);
    {
      Real f[6];
#pragma unroll
      for (int n = 0; n < 6; n++) f[n] = 0.0;
      if (need1) face_solve<NS>(g, in1, f);
      if (keep1) store_sweep<0, NS>((FBase)g.F, z, mb1, f);
#pragma unroll
      for (int n = 0; n < NV; n++) d1[n] = __shfl_down(f[n], 1) - f[n];
      m1lo = f[0]; m1hi = __shfl_down(f[0], 1);
      if (edge) {
#pragma unroll
        for (int n = 0; n < NV; n++) s_f1e[pb][lane][n] = f[n];
      }
      if (last) {
#pragma unroll
        for (int n = 0; n < NV; n++) s_f1s[pb][row][n] = f[n];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (cell) face_load<NS, 2>(g, z, (long)z.sK8, mb, in1);          // (in1 is free: reused for the x3 face)
    __builtin_amdgcn_sched_barrier(0);
    {
      Real f[6];
#pragma unroll
      for (int n = 0; n < 6; n++) f[n] = 0.0;
      if (need2) face_solve<NS>(g, in2, f);
      if (keep2) store_sweep<1, NS>(fbase(g.F, z, 6), z, mb, f);
#pragma unroll
      for (int n = 0; n < NV; n++) s_f2[pb][row][n][lane] = f[n];
      __syncthreads();
      if (row < FU_TJ - 1) {
#pragma unroll
        for (int n = 0; n < NV; n++) d2[n] = s_f2[pb][row + 1][n][lane] - f[n];
        m2hi = s_f2[pb][row + 1][0][lane];
      }
      m2lo = f[0];
      if (last) {           // the same subtraction as in the other lanes, operands through LDS
#pragma unroll
        for (int n = 0; n < NV; n++) d1[n] = s_f1e[pb][row][n] - s_f1s[pb][row][n];
        m1hi = s_f1e[pb][row][0];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // The potentials and d^{n+1/2} of the zone's update are requested in front of the x3 Riemann problem
    // instead of behind it (same-box, 512^3: 13.45 -> 13.15 ms; the conserved variables instead 13.26, both 14.57: four registers in
    // scratch -- profiles/r04_x1f_ab.txt item 7)
    Real ep[7], edh = 0.0;
#pragma unroll
    for (int v = 0; v < 7; v++) ep[v] = 0.0;
    if (GRAV && cell) {
      FBase pf = (FBase)g.phi;
      const unsigned o = zsite(mb, pf);
      ep[0] = zp(pf, o)[0]; edh = zp((FBase)dhalf, o)[0];
      pf = fnext(pf, z); ep[1] = zp(pf, o)[1]; ep[2] = zp(pf, o)[0];
      pf = fnext(pf, z); ep[3] = zp(fup(pf, z.sJ8), o)[0]; ep[4] = zp(pf, o)[0];
      pf = fnext(pf, z); ep[5] = zp(fup(pf, z.sK8), o)[0]; ep[6] = zp(pf, o)[0];
    }
    Real f3[6];
#pragma unroll
    for (int n = 0; n < 6; n++) f3[n] = 0.0;
    if (cell) face_solve<NS>(g, in1, f3);
    __builtin_amdgcn_sched_barrier(0);
    if (need1 && k < k1) face_load<NS, 0>(g, z, (long)z.sK8, mb1, in1);  // the next zone's x1 face
    __builtin_amdgcn_sched_barrier(0);
    if (cell) {
      if (KEEP && on_plane(kp, 2, k + 1)) store_sweep<2, NS>(fup(fbase(g.F, z, 12), z.sK8), z, mb, f3);
#pragma unroll
      for (int n = 0; n < NV; n++) { f3lo[n] = s_f3[n][row][lane]; d3[n] = f3[n] - f3lo[n]; }
      m3hi = f3[0];
      const Real m3lo = f3lo[0];
#pragma unroll
      for (int n = 0; n < NV; n++) s_f3[n][row][lane] = f3[n];
      Real u[6];
      const unsigned o = zsite(mb, (FBase)g.U);
      {
        FBase b = (FBase)g.U;
#pragma unroll
        for (int v = 0; v < NV; v++) { u[v] = zp(b, o)[0]; b = fnext(b, z); }
      }
      // (the mask byte with the zone's other operands, not behind the stores of U: a load that is consumed at once waits
      //  for everything issued before it, i.e. the wave sat out the six stores' round trip in every plane)
      unsigned char pinned = 0;
      if (CFL && pinmask) pinned = pinmask[zsite(mb, (FBase)pinmask) >> 3];      // (a byte per zone)
      if (GRAV) {   // :2741-2782, with the mass fluxes (sweep component 0) of the faces just solved
        const Real phic = ep[0], dh = edh;
        { const Real phir = ep[1], phil = ep[2];
          u[1] -= dtodx[0]*(phir - phil)*dh;
          u[4] -= dtodx[0]*(m1lo*(phic - phil) + m1hi*(phir - phic)); }
        { const Real phir = ep[3], phil = ep[4];
          u[2] -= dtodx[1]*(phir - phil)*dh;
          u[4] -= dtodx[1]*(m2lo*(phic - phil) + m2hi*(phir - phic)); }
        { const Real phir = ep[5], phil = ep[6];
          u[3] -= dtodx[2]*(phir - phil)*dh;
          u[4] -= dtodx[2]*(m3lo*(phic - phil) + m3hi*(phir - phic)); }
      }
#if AA_COOLING
      u[4] -= dt*cool_koyinut(zp((FBase)dhalf, o)[0], zp((FBase)g.phalf, o)[0], dt, g.Gamma_1);      // Step 11c, :2943-2953
#endif
      // :2981-3050, x1 then x2 then x3; sweep component n of direction D is global variable gv<D>(n)
#pragma unroll
      for (int n = 0; n < NV; n++) u[gv<0>(n)] -= dtodx[0]*d1[n];
#pragma unroll
      for (int n = 0; n < NV; n++) u[gv<1>(n)] -= dtodx[1]*d2[n];
#pragma unroll
      for (int n = 0; n < NV; n++) u[gv<2>(n)] -= dtodx[2]*d3[n];
      {
        FBase b = (FBase)g.U;
        const unsigned os = zsite(mb, fnext(b, z));      // (behind the branch on the mask byte: a block of its own)
#pragma unroll
        for (int v = 0; v < NV; v++) { zpw(b, os)[0] = u[v]; b = fnext(b, z); }
      }
      if (CFL) {
        if (!pinned) {
          Real cmx[3] = {s_cmx[0][row][lane], s_cmx[1][row][lane], s_cmx[2][row][lane]};
          cfl_zone(u[0], u[1], u[2], u[3], u[4], g.Gamma, g.Gamma_1, cmx);
          s_cmx[0][row][lane] = cmx[0]; s_cmx[1][row][lane] = cmx[1]; s_cmx[2][row][lane] = cmx[2];
        }
      }
    }
  }
  if (CFL) {       // block maximum -> 3 atomics (MAX of non-negative doubles on their bit patterns: order-free)
    Real *red = &s_cmx[0][0][0];           // [d][row][lane] = [d*64*FU_TJ + t]
    const int t = row*64 + lane;
    __syncthreads();
    for (int w = 32*FU_TJ; w > 0; w >>= 1) {
      if (t < w) {
#pragma unroll
        for (int d = 0; d < 3; d++) red[d*64*FU_TJ + t] = rmax(red[d*64*FU_TJ + t], red[d*64*FU_TJ + t + w]);
      }
      __syncthreads();
    }
    if (t == 0) for (int d = 0; d < 3; d++) atomic_max_pos(&sc->max_v[d], red[d*64*FU_TJ]);
  }
}
