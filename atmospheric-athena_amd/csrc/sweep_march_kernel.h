// sweep_march_kernel.h -- k_sweep_march of hydro_kernels.hip (which says in front of its #include lines why the kernel lives here).
// No include guard: compiled twice --
//   as it stands          k_sweep_march(g, src, dt, chunk, toff, tcnt): dt is a kernel argument
//   AA_CLOCK_ENTRY        k_sweep_march_dc(g, src, rc, chunk, toff, tcnt): one uniform load of `live` and dt from the device clock
//                         (hydro3d_launch.h Run3D; written by k3d_seed / k3d_advance, kernels in front of this one on the same
//                         stream, and by nobody while this one runs); a step queued behind the stop returns there, before any
//                         store (the whole grid takes the same branch).  Instantiated for the x2 first pass only.
// Below the opening brace the two are one text.
template <int NS, int D, bool GRAV, int MODE, int ORD>
__global__ void __launch_bounds__(256, SW_OCC)      // 3 waves per SIMD (168 VGPRs): the kernel is VALU-bound and sits right at that edge
#ifdef AA_CLOCK_ENTRY
k_sweep_march_dc(DevGrid g, const Real *src, const Run3D *rc, int chunk, int toff, int tcnt)
{
  if (!rc->c.live) return;
  const Real dt = rc->c.dt;
#else
k_sweep_march(DevGrid g, const Real *src, Real dt, int chunk, int toff, int tcnt)
{
#endif
  static_assert(D == 1 || D == 2, "march kernel is for the strided directions");
  // transverse lines toff .. toff+tcnt-1 of the (D == 1 ? ke - ks : je - js) + 5 (the launcher passes all of them, or
  // for x2 a range of k-planes: see launch_sweep)
  const int tlo = (D == 1 ? g.ks : g.js) - 2 + toff;
  const int nt  = tcnt;
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  // lanes on whole 128-byte lines: a row of slots starts on the line that holds is-2 and is a whole number of lines long (a
  // wavefront's 64 lanes are four whole lines of one or two rows; the lanes off the ends of [is-2, ie+2] leave)
  const int nq = march_slots(g);
  if (lin >= (long)nq*nt) return;
  const int q = (int)(lin % nq);
  int i;
  const int t = tlo + (int)(lin / nq);
  if (!march_cell(g, q, i)) return;
  const int lo = (D == 1 ? g.js : g.ks), hi = (D == 1 ? g.je : g.ke);
  const int f0 = lo - 1 + blockIdx.y*chunk;                    // first interface of this chunk
  int f1 = f0 + chunk - 1; if (f1 > hi + 2) f1 = hi + 2;
  if (f0 > f1) return;
  const long s = stride<D>(g);
  const long base = (D == 1) ? ((long)t*g.sK + i) : ((long)t*g.sJ + i);
  const Real dtodx = dt/g.dx[D];

  // ONE inlined instance of the reconstruction serves every cell, also the cell below the chunk's
  // first interface (iteration f0-1, whose face work is skipped): with fused multiply-adds allowed, two
  // instances may round differently, and the result must not depend on where the chunks start (the
  // chunk size follows the Grid size, hence the decomposition).
  Real wm[6], w[6], wp[6], wl_cur[6], wl_next[6], wr[6], u[6];
  load_sweep<D, NS>(src, g.nc, base + (long)(f0 - 2)*s, u); cons_to_prim<NS>(u, w,  g.Gamma_1);
  load_sweep<D, NS>(src, g.nc, base + (long)(f0 - 1)*s, u); cons_to_prim<NS>(u, wp, g.Gamma_1);
#pragma unroll
  for (int n = 0; n < 6; n++) wl_cur[n] = 0.0;
#pragma nounroll
  for (int f = f0 - 1; f <= f1; f++) {
    // one index for all fields instead of a strength-reduced pointer per field: a 32-bit byte offset on the fields' scalar bases
    // (hydro_kernels.hip, field accessors); the 64-bit zone index serves the correct pass of the unfused chain alone
    const ZStr z = zone_strides(g);
    const unsigned mb = zone_off(base + (long)f*s);
    long mf = 0;
    if (MODE == MODE_CORR || MODE == MODE_BOTH) { mf = base + (long)f*s; asm volatile("" : "+v"(mf)); }
#pragma unroll
    for (int n = 0; n < 6; n++) { wm[n] = w[n]; w[n] = wp[n]; }
    load_sweep<D, NS>(fup((FBase)src, zstride<D>(z)), z, mb, 0, u); cons_to_prim<NS>(u, wp, g.Gamma_1);
    recon_cell<NS, MODE != MODE_VL, ORD, D>(g, z, 0L, mb, wm, w, wp, dtodx, wl_next, wr);  // cell f -> Wl[f+1], Wr[f]
    if (f >= f0) face_work<NS, D, GRAV, MODE>(g, z, mb, mf, i, D == 1 ? f : t, D == 1 ? t : f, dt, wl_cur, wr);
#pragma unroll
    for (int n = 0; n < 6; n++) wl_cur[n] = wl_next[n];
  }
}
