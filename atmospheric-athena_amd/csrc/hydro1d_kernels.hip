// hydro1d_kernels.hip -- the hydro hot path of a 1-D Grid (Nx2 = Nx3 = 1; gfx950): integrate_1d_ctu.c and integrate_1d_vl.c of
// the reference for HYDRO, ADIABATIC, CARTESIAN, second or third order, no gravity, no cooling, no passive scalar.  The per-cell
// and per-face arithmetic is that of hydro_dev.h, unchanged; this file only restates the 1-D loop nests.  M2 and M3 ride along
// as the reference carries them (My, Mz of the 1-D vectors).
//
// Layout (api.hip aa_create): one row of N1 = Nx1 + 8 zones per field, no ghost zones along x2 and x3 (js = je = ks = ke = 0),
// fields nc = sJ apart, the first active zone (i = 4) on a 128-byte line:
//   U   5 fields  d, M1, M2, M3, E
//   LR  5 fields  the second U buffer (also the staging area of the transfers, as in the other layouts)
//
// One step is step_core(): a workgroup holds a run of zones with four halo zones either side in LDS and walks the reference's
// stages with a workgroup barrier between them, every array a row per field in LDS:
//   sU  the conserved state, updated in place at the end
//   sA  W = Cons1D_to_Prim1D(U) (van Leer: later W of U^{n+1/2}), then the second-pass fluxes
//   sB  third order: the monotonised slopes of lr_states_ppm.c; van Leer: before that the donor-cell predictor fluxes
//   CTU (Steps 1a-1d, 12a): W | slopes | per face: reconstruct the zone below and the zone above, Riemann solve | update
//   VL  (Steps 1-7, 10-13):  W | predictor fluxes | U^{n+1/2} -> W | slopes | the same face stage without tracing | update
// A thread owns a face: it reconstructs both zones beside it (plm_cell / ppm_cell give Wl of the upper and Wr of the lower face
// of ONE zone, so every zone is reconstructed twice) instead of passing face states through ten more LDS rows; the flux waits in
// registers for the barrier behind which it may overwrite W.  Neighbour values come from LDS only, fluxes never reach HBM, and
// the update folds new_dt's maximum of |v1| + a (new_dt.c:126-127: max_v1 alone on a 1-D Grid).
//
// (a) k1d_step<VL, ORD>: one launch per step, any Nx1.  S1_NT = 256 threads, one zone each; a block covers S1_B = 248 active zones
//     and RECOMPUTES the four halo zones either side instead of exchanging them (3 % more zones loaded, the stages on them are
//     skipped where the reference's ranges end).  Blocks read U and write a SECOND buffer, which then becomes U (api1d.hip swaps
//     the two pointers): a block's halo is its neighbour's active run, and nothing orders two blocks of one launch, so an update
//     in place would hand some block a mixture of U^n and U^{n+1}.  The other choice, fluxes in an array of their own and a
//     second launch for the update, costs the launch this path has least to spare and puts the fluxes in HBM.  The first and the
//     last block copy the ghost zones across, so that a side without a boundary function keeps its values; bvals_mhd is the
//     step's second launch (aa_bvals_mhd, the x1 pass of k_bc).
// (b) k1d_run<VL, ORD>: whole passes of the main loop (main.c:519-669) in ONE launch for Grids of up to R1_CAP = 1272 active
//     zones (the largest deck of tst/1D-hydro has 1200): ONE workgroup of R1_NT = 512 threads, up to three zones each, keeps
//     the 15 rows of 1280 doubles = 153,600 B of the CU's 160 KiB LDS.  Per pass: step_core, nstep++, time += dt, the x1
//     boundary in LDS, the block's maximum (wavefront shuffles, then one LDS row of eight), new_dt's dt with the factor-two
//     limit and the clip at tlim.  It ends when time >= t_stop, nstep == nstep_stop or dt <= 0; the state and time / dt / nstep
//     go back to HBM once.  Workgroup barriers only: no global atomic, no wait on another workgroup, no cooperative launch;
//     the host bounds nstep_stop - nstep by 2^20, so the launch ends.
// Both kernels run step_core on the same numbers in the same order, so the two paths give the same bits in either build.
// None of these shapes has been timed against an alternative: the block of 248 + 8 is "a whole number of wavefronts, several
// blocks per CU", the resident group of 512 is "two waves per SIMD, 256 registers each"; profiles/rate_1d.py measures what
// they reach.
#include <hip/hip_runtime.h>
#include "hydro1d_launch.h"
#include "hydro_dev.h"

namespace aa {

#define S1_NT 256
#define S1_LD 256            /* zones of a block's tile: S1_B active + 2 x 4 halo */
#define S1_B  (S1_LD - 2*AA_NGHOST_)
#define R1_NT 512
#define R1_LD 1280
#define R1_CAP (R1_LD - 2*AA_NGHOST_)
#define R1_K  ((R1_LD + R1_NT - 1)/R1_NT)

AA_DEV void lds_get(const Real *s, int ld, int c, Real u[6])
{
#pragma unroll
  for (int v = 0; v < 5; v++) u[v] = s[v*ld + c];
  u[5] = 0.0;
}
AA_DEV void lds_put(Real *s, int ld, int c, const Real u[6])
{
#pragma unroll
  for (int v = 0; v < 5; v++) s[v*ld + c] = u[v];
}

// Wl of the upper and Wr of the lower face of zone c from the W row (and the slope row)
template <int ORD, bool TRACE>
AA_DEV void recon_1d(const Real *sW, const Real *sD, int ld, int c, Real dtodx, Real Gamma, Real wl_next[6], Real wr_here[6])
{
  Real wm[6], w[6], wp[6];
  lds_get(sW, ld, c - 1, wm); lds_get(sW, ld, c, w); lds_get(sW, ld, c + 1, wp);
  if (ORD == 3) {
    Real dm[6], d0[6], dp[6];
    lds_get(sD, ld, c - 1, dm); lds_get(sD, ld, c, d0); lds_get(sD, ld, c + 1, dp);
    ppm_cell<0, TRACE>(wm, w, wp, dm, d0, dp, dtodx, Gamma, wl_next, wr_here);
  } else
    plm_cell<0, TRACE>(wm, w, wp, dtodx, Gamma, wl_next, wr_here);
}

// new_dt.c:72-127 for one zone of a 1-D Grid (the operands and their order as in cfl_zone of the 3-D path; never contracted)
AA_DEV Real cfl_zone1(Real d, Real m1, Real m2, Real m3, Real e, Real Gamma, Real Gamma_1, Real mx)
{
#pragma clang fp contract(off)
  const Real di = 1.0/d;
  const Real v1 = m1*di, v2 = m2*di, v3 = m3*di;
  const Real qsq = v1*v1 + v2*v2 + v3*v3;
  const Real p = rmax(Gamma_1*(e - 0.5*d*qsq), AA_TINY);
  const Real a = sqrt(Gamma*p*di);
  return rmax(mx, fabs(v1) + a);
}

// One step of the zones 4 .. n-5 of a tile of n zones (rows ld apart).  Every thread of the workgroup calls it (barriers); thread
// t owns the zones / faces t, t + NT, .. (K of them at the most).  Returns the thread's maximum of |v1| + a over the zones it updated.
template <bool VL, int ORD, int NT, int K>
AA_DEV Real step_core(Real *sU, Real *sA, Real *sB, const int ld, const int n, const Real dt, const Real dx,
                      const Real Gamma, const Real Gamma_1, const Real rGamma_1)
{
  const int tid = threadIdx.x;
  const Real dtodx = dt/dx, hdtodx = 0.5*dt/dx;
  // Step 1a-b: W of every zone
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int c = tid + k*NT;
    if (c < n) { Real u[6], w[6]; lds_get(sU, ld, c, u); cons_to_prim<0>(u, w, Gamma_1); lds_put(sA, ld, c, w); }
  }
  __syncthreads();
  if (VL) {
    // Steps 1b-d: donor-cell fluxes of the faces il .. ie + nghost (Ul = U1d[i-1], Ur = U1d[i] as they are)
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int f = tid + k*NT;
      if (f >= 1 && f < n) {
        Real ul[6], ur[6], wl[6], wr[6], fx[6];
        lds_get(sU, ld, f - 1, ul); lds_get(sU, ld, f, ur); lds_get(sA, ld, f - 1, wl); lds_get(sA, ld, f, wr);
        flux_roe<0>(ul, ur, wl, wr, 0.0, Gamma, Gamma_1, fx);
        lds_put(sB, ld, f, fx);
      }
    }
    __syncthreads();
    // Steps 5a, 7a-b: U^{n+1/2} of the zones il .. iu and its W (the W row is not read in this stage)
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int c = tid + k*NT;
      if (c >= 1 && c <= n - 2) {
        Real u[6], fm[6], fp[6], w[6];
        lds_get(sU, ld, c, u); lds_get(sB, ld, c, fm); lds_get(sB, ld, c + 1, fp);
#pragma unroll
        for (int v = 0; v < 5; v++) u[v] -= hdtodx*(fp[v] - fm[v]);
        cons_to_prim<0>(u, w, Gamma_1);
        lds_put(sA, ld, c, w);
      }
    }
    __syncthreads();
  }
  if (ORD == 3) {
    // lr_states_ppm.c Steps 1-5: the slopes of the zones is-2 .. ie+2
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int c = tid + k*NT;
      if (c >= 2 && c <= n - 3) {
        Real wm[6], w[6], wp[6], dw[6];
        lds_get(sA, ld, c - 1, wm); lds_get(sA, ld, c, w); lds_get(sA, ld, c + 1, wp);
        limited_slopes<0>(wm, w, wp, Gamma, dw);
        lds_put(sB, ld, c, dw);
      }
    }
    __syncthreads();
  }
  // CTU Steps 1b-d / VL Steps 7b, 10b: the faces is .. ie+1
  Real fl[K][5];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int f = tid + k*NT;
#pragma unroll
    for (int v = 0; v < 5; v++) fl[k][v] = 0.0;
    if (f >= AA_NGHOST_ && f <= n - AA_NGHOST_) {
      Real wl[6], wr[6], dump[6], ul[6], ur[6], fx[6];
      recon_1d<ORD, !VL>(sA, sB, ld, f - 1, dtodx, Gamma, wl, dump);
      recon_1d<ORD, !VL>(sA, sB, ld, f, dtodx, Gamma, dump, wr);
      prim_to_cons<0>(wl, ul, Gamma_1, rGamma_1);
      prim_to_cons<0>(wr, ur, Gamma_1, rGamma_1);
      flux_roe<0>(ul, ur, wl, wr, 0.0, Gamma, Gamma_1, fx);
#pragma unroll
      for (int v = 0; v < 5; v++) fl[k][v] = fx[v];
    }
  }
  __syncthreads();                       // every reconstruction has read W (and the slopes): the fluxes take W's rows
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int f = tid + k*NT;
    if (f >= AA_NGHOST_ && f <= n - AA_NGHOST_) {
#pragma unroll
      for (int v = 0; v < 5; v++) sA[v*ld + f] = fl[k][v];
    }
  }
  __syncthreads();
  // Step 12a / 13a
  Real mx = 0.0;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int c = tid + k*NT;
    if (c >= AA_NGHOST_ && c <= n - AA_NGHOST_ - 1) {
      Real u[6], fm[6], fp[6];
      lds_get(sU, ld, c, u); lds_get(sA, ld, c, fm); lds_get(sA, ld, c + 1, fp);
#pragma unroll
      for (int v = 0; v < 5; v++) u[v] -= dtodx*(fp[v] - fm[v]);
      lds_put(sU, ld, c, u);
      mx = cfl_zone1(u[0], u[1], u[2], u[3], u[4], Gamma, Gamma_1, mx);
    }
  }
  return mx;
}

// the maximum over a wavefront (a NaN loses every comparison and is dropped, as in the CFL kernel of the 3-D path)
AA_DEV Real wave_max(Real x)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = rmax(x, __shfl_xor(x, o));
  return x;
}

template <bool VL, int ORD>
__global__ void __launch_bounds__(S1_NT)
k1d_step(DevGrid g, Real dt, Real *Unew, DevScalars *sc)
{
  __shared__ Real sU[5*S1_LD], sA[5*S1_LD], sB[5*S1_LD];
  __shared__ Real red[S1_NT/64];
  const int tid = threadIdx.x;
  const int a0 = g.is + S1_B*(int)blockIdx.x;                       // first active zone of the block
  const int left = g.ie + 1 - a0;
  const int nact = left < S1_B ? left : S1_B;                       // (the launch has no block with nact < 1)
  const int n = nact + 2*AA_NGHOST_, g0 = a0 - AA_NGHOST_;          // g0 >= 0, g0 + n <= N1
  if (tid < n) {
#pragma unroll
    for (int v = 0; v < 5; v++) sU[v*S1_LD + tid] = g.U[(long)v*g.nc + g0 + tid];
  }
  __syncthreads();
  Real mx = step_core<VL, ORD, S1_NT, 1>(sU, sA, sB, S1_LD, n, dt, g.dx[0], g.Gamma, g.Gamma_1, g.rGamma_1);
  // (a zone is written to LDS and read back here by the same thread)
  const bool first = blockIdx.x == 0, last = blockIdx.x == gridDim.x - 1;
  if (tid < n) {
    const bool act = tid >= AA_NGHOST_ && tid < n - AA_NGHOST_;
    if (act || (first && tid < AA_NGHOST_) || (last && tid >= n - AA_NGHOST_)) {
#pragma unroll
      for (int v = 0; v < 5; v++) Unew[(long)v*g.nc + g0 + tid] = sU[v*S1_LD + tid];
    }
  }
  if (sc) {
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
      Real r = red[0];
      for (int q = 1; q < S1_NT/64; q++) r = rmax(r, red[q]);
      if (r == r) atomicMax(&sc->max_v[0], (unsigned long long)__double_as_longlong(r));
    }
  }
}

// bvals_mhd.c x1 pass on the LDS rows: reflect :959 (flag 1, M1 negated), outflow :1319 (2), periodic :1637 (4); 0 leaves the side alone.
// Eight threads fill the eight ghost zones at once: with Nx1 >= 4 (aa_create refuses a 1-D Grid of fewer) every source is an active zone, so
// no thread reads what another writes.  (With fewer zones the reference's side-after-side order would matter.)
AA_DEV void bc_x1_lds(Real *sU, int ld, int is, int ie, int bc_in, int bc_out)
{
  const int tid = threadIdx.x;
  if (tid >= 2*AA_NGHOST_) return;
  const int side = tid / AA_NGHOST_, gl = 1 + tid % AA_NGHOST_;
  const int flag = side ? bc_out : bc_in;
  if (!flag) return;
  int dst, src;
  if (side == 0) { dst = is - gl; src = (flag == 1) ? is + (gl - 1) : (flag == 2) ? is : ie - (gl - 1); }
  else           { dst = ie + gl; src = (flag == 1) ? ie - (gl - 1) : (flag == 2) ? ie : is + (gl - 1); }
#pragma unroll
  for (int v = 0; v < 5; v++) {
    Real x = sU[v*ld + src];
    if (flag == 1 && v == 1) x = -x;
    sU[v*ld + dst] = x;
  }
}

template <bool VL, int ORD>
__global__ void __launch_bounds__(R1_NT)
k1d_run(DevGrid g, int bc_in, int bc_out, Real cour_no, Real t_stop, Real tlim, int nstep_stop, RunClock *rs)
{
  __shared__ Real sU[5*R1_LD], sA[5*R1_LD], sB[5*R1_LD];
  __shared__ Real red[R1_NT/64];
  const int tid = threadIdx.x;
  const int n = g.N1;                                               // <= R1_LD (api1d.hip)
  for (int c = tid; c < n; c += R1_NT) {
#pragma unroll
    for (int v = 0; v < 5; v++) sU[v*R1_LD + c] = g.U[(long)v*g.nc + c];
  }
  // (every thread carries the same time, dt and nstep: the loop condition is uniform)
  Real time = rs->time, dt = rs->dt;
  int nstep = rs->nstep;
  __syncthreads();
  while (run_live(time, t_stop, nstep, nstep_stop, dt)) {
    Real mx = step_core<VL, ORD, R1_NT, R1_K>(sU, sA, sB, R1_LD, n, dt, g.dx[0], g.Gamma, g.Gamma_1, g.rGamma_1);   // main.c:572-585
    nstep++; time += dt;                                            // :618-626
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();                                                // (the updated zones are in LDS, the waves' maxima in red)
    bc_x1_lds(sU, R1_LD, g.is, g.ie, bc_in, bc_out);                // :635-644 (ghost zones only: new_dt reads none)
    Real vmax = red[0];
#pragma unroll
    for (int q = 1; q < R1_NT/64; q++) vmax = rmax(vmax, red[q]);
    dt = dt_pick(nstep, dt, dt_courant(cour_no, dt_fold(0.0, &vmax, g.dx, 1)), time, tlim);   // new_dt.c:156-185 (time_step.h)
    __syncthreads();                                                // (the ghost zones are written; red is free again)
  }
  for (int c = tid; c < n; c += R1_NT) {
#pragma unroll
    for (int v = 0; v < 5; v++) g.U[(long)v*g.nc + c] = sU[v*R1_LD + c];
  }
  if (tid == 0) { rs->time = time; rs->dt = dt; rs->nstep = nstep; rs->live = 0; }   // (live: not read here; the loop has ended)
}

// ---- launch wrappers -----------------------------------------------------------------------------------------------------
int run1d_cap() { return R1_CAP; }
int step1d_block() { return S1_B; }

void launch_1d_step(const DevGrid &g, bool vl, bool third, Real dt, Real *Unew, DevScalars *sc, hipStream_t st)
{
  const unsigned nb = (unsigned)((g.Nx1 + S1_B - 1)/S1_B);
  with_flag(vl, [&](auto VL) { with_ord(third, [&](auto ORD) {
    hipLaunchKernelGGL((k1d_step<VL, ORD>), dim3(nb), dim3(S1_NT), 0, st, g, dt, Unew, sc); }); });
}
void launch_1d_run(const DevGrid &g, bool vl, bool third, int bc_in, int bc_out, Real cour_no, Real t_stop, Real tlim, int nstep_stop, RunClock *rs, hipStream_t st)
{
  with_flag(vl, [&](auto VL) { with_ord(third, [&](auto ORD) {
    hipLaunchKernelGGL((k1d_run<VL, ORD>), dim3(1), dim3(R1_NT), 0, st, g, bc_in, bc_out, cour_no, t_stop, tlim, nstep_stop, rs); }); });
}

}  // namespace aa
