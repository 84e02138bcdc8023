// history_dc.hip -- the history sums of hydro_kernels.hip k_history behind a queued step of a run call that has a history schedule
// armed (run.hip aa_run_hst_arm; time_step.h HstSched / hst_row_due), for 2-D and 3-D Grids alike.
//
// hydro_kernels.hip is one of the sources whose fingerprint the committed traffic profiles carry (bench.py KERNEL_SOURCES), so it
// stays as it is, byte for byte, and k_history keeps its code.  history_body below is k_history's body, the same text between the
// two marked lines (tests/test_hst_run_host.py compares the two texts), compiled with the same flags and launched with the same
// geometry: the partial rows are the same bits in the same order (tests/test_gpu_hst_run.py, both builds).
#include "hydro3d_launch.h"

namespace aa {

static __device__ __forceinline__ Real *Uf(const DevGrid &g, int v) { return g.U + (long)v*g.nc; }
static inline unsigned nblk(long n, int b) { return (unsigned)((n + b - 1)/b); }

// ---- history sums (dump_history.c:157-200): mass, E, momenta, kinetic energies, scalar; one
// partial row per block, added up in block order (deterministic) -------------------------------
static __device__ __forceinline__ void history_body(const DevGrid &g, int nscal, Real *partial)
{
  // >>> k_history
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
  // <<< k_history
}

// The clock as the step's advance kernel left it and the schedule as k_hst_row left it, both in uniform loads, and a return before
// any store and before any barrier -- the whole grid takes the same branch -- unless the step in front was taken (the clock's nstep
// has moved on since the schedule looked) and data_output's rule says a row is due behind it (hst_row_due; the schedule itself is
// written by k_hst_row alone, one launch behind this one).  Launch rule as k2d_advance / k3d_advance state it: a plain launch in
// stream order; nothing waits on memory or on another workgroup.
__global__ void __launch_bounds__(256)
k_history_dc(DevGrid g, int nscal, Real *partial, const RunClock *clock, Real tlim, const HstSched *sched)
{
  const RunClock c = *clock; const HstSched s = *sched;
  if (c.nstep == s.nstep_seen) return;
  double t_next = s.t_next;
  if (!hst_row_due(c.time, c.nstep, tlim, s.nlim, s.dt_out, &t_next)) return;
  history_body(g, nscal, partial);
}

int launch_history_dc(const DevGrid &g, int nscal, Real *partial, const RunClock *clock, Real tlim, const HstSched *sched, hipStream_t st)
{
  const long n = (long)(g.ie - g.is + 1)*(g.je - g.js + 1)*(g.ke - g.ks + 1);
  unsigned nb = nblk(n, 256); if (nb > 1024) nb = 1024;      // (launch_history's geometry: the rows and their order are the same)
  hipLaunchKernelGGL(k_history_dc, dim3(nb), dim3(256), 0, st, g, nscal, partial, clock, tlim, sched);
  return (int)nb;
}

}  // namespace aa
