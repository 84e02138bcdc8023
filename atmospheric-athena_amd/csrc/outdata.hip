// outdata.hip -- the payload of the reference's single-variable outputs (out = d, M1 .. cs2, flux with x1 / x2 / x3 slices) from the
// resident state: OutData3, OutData2, OutData1 (output.c:629-1107) and the expr_* functions (:1109-1233), the minimum and maximum
// minmax1/2/3 (utils.c:142-197) find, and the gray bytes of output_pgm.c:86-122.
//
// An element of the payload is the expression of one zone (nothing reduced), or the sum of the expression over the zones of the
// reduced directions in the reference's order -- k, then j, then i ascending, started at 0.0 -- times factor = 1.0/count[/count].
// ONE thread walks the whole sum of an element, so the order of the additions is the reference's whatever the launch; the lanes run
// along the fastest KEPT direction.  Where x1 is kept a wave's loads are 512 contiguous bytes per field; where x1 is reduced
// neighbouring lanes are a row (sJ doubles) apart and every lane walks its own row (see DESIGN.md section 3 for what that costs).
//
// The payload travels like a section of a data dump (dump.hip): pieces made into the idle face-state area, copied through the two
// halves of the page-locked bounce buffer while the next piece is made.  Nothing of the payload's size is allocated.
//
// The arithmetic is the reference's, operation by operation, in BOTH libraries: no contraction, IEEE quotients, multiplication by
// `factor` instead of a division.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <string.h>
#include "api_internal.h"
#include "outdata_launch.h"

#pragma clang fp contract(off)

using namespace aa;

namespace aa {

// expr_* of output.c for the ACTIVE zone (i, j, k) counted from 0; flux: print_flux of prob/ioniz_sphere.c:356-359
__device__ __forceinline__ Real out_value(const DevGrid &g, int ex, int i, int j, int k)
{
  if (ex == AA_OUT_FLUX) return g.edgeflux[((long)k*(g.Nx2 + 1) + j)*(long)(g.Nx1 + 1) + i];
  const long m = (long)(k + g.ks)*g.sK + (long)(j + g.js)*g.sJ + (long)(i + AA_NGHOST_);
  const Real d = g.U[m];
  if (ex == AA_OUT_D) return d;
  if (ex <= AA_OUT_E) return g.U[(long)ex*g.nc + m];
  if (ex <= AA_OUT_V3) return g.U[(long)(ex - AA_OUT_V1 + 1)*g.nc + m]/d;
  const Real M1 = g.U[g.nc + m], M2 = g.U[2*g.nc + m], M3 = g.U[3*g.nc + m], E = g.U[4*g.nc + m];
  const Real e = E - 0.5*(M1*M1 + M2*M2 + M3*M3)/d;
  if (ex == AA_OUT_P) return g.Gamma_1*e;
  return g.Gamma*g.Gamma_1*e/d;              // cs2, output.c:1210-1214: ((Gamma*Gamma_1)*e)/d
}

__device__ __forceinline__ Real out_element(const DevGrid &g, const OutDesc &q, unsigned long long o)
{
  const unsigned a = (unsigned)(o % q.n[0]); const unsigned long long r = o/q.n[0];
  const unsigned b = (unsigned)(r % q.n[1]), c = (unsigned)(r/q.n[1]);
  if (!q.sum) return out_value(g, q.ex, (int)a, (int)b, (int)c);
  const int i0 = q.red[0] ? q.lo[0] : (int)a, i1 = q.red[0] ? q.hi[0] : (int)a;
  const int j0 = q.red[1] ? q.lo[1] : (int)b, j1 = q.red[1] ? q.hi[1] : (int)b;
  const int k0 = q.red[2] ? q.lo[2] : (int)c, k1 = q.red[2] ? q.hi[2] : (int)c;
  Real s = 0.0;
  for (int k = k0; k <= k1; k++)
    for (int j = j0; j <= j1; j++)
      for (int i = i0; i <= i1; i++) s += out_value(g, q.ex, i, j, k);
  s *= q.factor;
  return s;
}

// ---- minimum and maximum as minmax1/2/3 leave them: dmin = MIN(dmin, data) = (dmin < data) ? dmin : data over the elements in
// payload order, so that of two elements that compare equal (the zeros of either sign) the LATER one stays.  A record carries the
// payload index beside each value; joining two records keeps, for the minimum, the earlier one where it is smaller and the later one
// otherwise -- for numbers the fold of the reference whatever the order of the joins.  (A NaN makes the reference's own result
// depend on where it stands; it is not reproduced.)
#define OUT_NONE 0xffffffffu
struct OutMM { Real mn, mx; unsigned mni, mxi; };

__device__ __forceinline__ void mm_take(OutMM &r, Real v, unsigned idx)       // idx behind everything r has seen
{
  if (r.mni == OUT_NONE) { r.mn = r.mx = v; r.mni = r.mxi = idx; return; }
  if (!(r.mn < v)) { r.mn = v; r.mni = idx; }
  if (!(r.mx > v)) { r.mx = v; r.mxi = idx; }
}
__device__ __forceinline__ OutMM mm_join(const OutMM &x, const OutMM &y)
{
  if (x.mni == OUT_NONE) return y;
  if (y.mni == OUT_NONE) return x;
  OutMM r;
  { const bool xe = x.mni < y.mni;
    const Real ev = xe ? x.mn : y.mn, lv = xe ? y.mn : x.mn; const unsigned ei = xe ? x.mni : y.mni, li = xe ? y.mni : x.mni;
    if (ev < lv) { r.mn = ev; r.mni = ei; } else { r.mn = lv; r.mni = li; } }
  { const bool xe = x.mxi < y.mxi;
    const Real ev = xe ? x.mx : y.mx, lv = xe ? y.mx : x.mx; const unsigned ei = xe ? x.mxi : y.mxi, li = xe ? y.mxi : x.mxi;
    if (ev > lv) { r.mx = ev; r.mxi = ei; } else { r.mx = lv; r.mxi = li; } }
  return r;
}
// the record of a block of 256 threads, in thread 0 (lds: 4 records)
__device__ __forceinline__ OutMM mm_block(OutMM v, OutMM *lds)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    OutMM o;
    o.mn = __shfl_down(v.mn, off, 64); o.mx = __shfl_down(v.mx, off, 64);
    o.mni = __shfl_down(v.mni, off, 64); o.mxi = __shfl_down(v.mxi, off, 64);
    v = mm_join(v, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) { v = lds[0]; for (int w = 1; w < 4; w++) v = mm_join(v, lds[w]); }
  return v;
}
__device__ __forceinline__ void mm_store(Real *p, const OutMM &v)
{ p[0] = v.mn; p[1] = (Real)v.mni; p[2] = v.mx; p[3] = (Real)v.mxi; }
__device__ __forceinline__ OutMM mm_load(const Real *p)
{ OutMM v; v.mn = p[0]; v.mni = (unsigned)p[1]; v.mx = p[2]; v.mxi = (unsigned)p[3]; return v; }

// elements p0 .. p0 + cnt of the payload to dst[0 .. cnt); a thread takes the elements t, t + T, t + 2T .. of the piece (T = all
// threads of the launch), so that a wave's elements are neighbours and a thread's own come in ascending order
__global__ void __launch_bounds__(256) k_out_payload(DevGrid g, OutDesc q, unsigned long long p0, unsigned cnt, Real *dst, Real *part)
{
  __shared__ OutMM lds[4];
  OutMM r; r.mn = r.mx = 0.0; r.mni = r.mxi = OUT_NONE;
  const unsigned T = gridDim.x*256u;
  for (unsigned long long t = (unsigned long long)blockIdx.x*256ull + threadIdx.x; t < (unsigned long long)cnt; t += T) {
    const Real v = out_element(g, q, p0 + t);
    dst[t] = v;
    mm_take(r, v, (unsigned)(p0 + t));
  }
  r = mm_block(r, lds);
  if (threadIdx.x == 0) mm_store(part + 4*blockIdx.x, r);
}

__global__ void __launch_bounds__(256) k_out_fold(const Real *part, int nblocks, Real *mm, int first)
{
  __shared__ OutMM lds[4];
  OutMM r; r.mn = r.mx = 0.0; r.mni = r.mxi = OUT_NONE;
  for (int b = threadIdx.x; b < nblocks; b += 256) r = mm_join(r, mm_load(part + 4*b));
  r = mm_block(r, lds);
  if (threadIdx.x == 0) {
    if (!first) r = mm_join(mm_load(mm), r);
    mm_store(mm, r);
  }
}

// byte p of the image: row nx2 - 1 - p/nx1 of the payload where the image is scaled (output_pgm.c:101), all 0 otherwise (:116-121)
__global__ void __launch_bounds__(256) k_out_gray(DevGrid g, OutDesc q, unsigned nx1, unsigned nx2, Real dmin, Real sfact, int scaled,
                                                  unsigned long long p0, unsigned cnt, unsigned char *dst)
{
  const unsigned t = blockIdx.x*256u + threadIdx.x;
  if (t >= cnt) return;
  int gray = 0;
  if (scaled) {
    const unsigned long long p = p0 + t;
    const unsigned long long row = p/nx1; const unsigned col = (unsigned)(p - row*nx1);
    const Real data = out_element(g, q, ((unsigned long long)nx2 - 1ull - row)*nx1 + col);
    const Real x = sfact*(data - dmin);
    // (int) of the host: a double outside the range of int, and a NaN, give INT_MIN there
    gray = (x > -2147483649.0 && x < 2147483648.0) ? (int)x : INT_MIN;
    gray = gray > 0 ? gray : 0;
    gray = gray < 255 ? gray : 255;
  }
  dst[t] = (unsigned char)gray;
}

int launch_out_payload(const DevGrid &g, const OutDesc &q, unsigned long long p0, unsigned cnt, Real *dst, Real *part, hipStream_t st)
{
  unsigned blocks = (cnt + 255u)/256u;
  if (blocks > AA_OUT_PART_BLOCKS) blocks = AA_OUT_PART_BLOCKS;
  hipLaunchKernelGGL(k_out_payload, dim3(blocks), dim3(256), 0, st, g, q, p0, cnt, dst, part);
  return (int)blocks;
}
void launch_out_fold(const Real *part, int nblocks, Real *mm, bool first, hipStream_t st)
{
  hipLaunchKernelGGL(k_out_fold, dim3(1), dim3(256), 0, st, part, nblocks, mm, first ? 1 : 0);
}
void launch_out_gray(const DevGrid &g, const OutDesc &q, Real dmin, Real sfact, bool scaled, unsigned long long p0, unsigned cnt,
                     unsigned char *dst, hipStream_t st)
{
  unsigned d[2]; int nd = 0;                 // the image's two directions: the kept ones of more than one element come first
  for (int a = 0; a < 3; a++) if (q.n[a] > 1 && nd < 2) d[nd++] = q.n[a];
  while (nd < 2) d[nd++] = 1;
  hipLaunchKernelGGL(k_out_gray, dim3((cnt + 255u)/256u), dim3(256), 0, st, g, q, d[0], d[1], dmin, sfact, scaled ? 1 : 0, p0, cnt, dst);
}

}  // namespace aa

void outdata_release(aa_grid *g)
{
  if (g->out_part) { (void)hipFree(g->out_part); g->out_part = nullptr; }
  if (g->out_mm_host) { (void)hipHostFree(g->out_mm_host); g->out_mm_host = nullptr; }
}

// the refusals and the description of an output; who: the entry's name
static int out_describe(aa_grid *g, const char *who, int expr, const int reduce[3], const int lo[3], const int hi[3], OutDesc *q,
                        unsigned long long *nout)
{
  if (!g || !reduce || !lo || !hi) return aa_fail(-1, "[%s]: null argument", who);
  if (g->link || !g->slab.empty())
    return aa_fail(-1, "[%s]: a Grid cut into slabs makes no single-variable output (one Grid on one device does)", who);
  if (g->keep_flux || g->level > 0)
    return aa_fail(-1, "[%s]: this Grid is a level of a Mesh (level %d): single-variable outputs are built for a single-level run", who, g->level);
  if (g->one_d) return aa_fail(-1, "[%s]: a 1-D Grid makes no single-variable output", who);
  if (expr < AA_OUT_D || expr > AA_OUT_FLUX) return aa_fail(-1, "[%s]: expression code %d (AA_OUT_D .. AA_OUT_FLUX)", who, expr);
  if (expr == AA_OUT_FLUX && !(g->p.ion && g->nradplane > 0))
    return aa_fail(-1, "[%s]: out = flux needs a Grid with a radiation plane (its EdgeFlux)", who);
  q->ex = expr; q->sum = 0; q->factor = 1.0;
  *nout = 1;
  for (int a = 2; a >= 0; a--) {             // factor: 1.0/count of x3, then x2, then x1 (output.c:987, :1042, :1093)
    const int N = g->p.Nx[a];
    q->red[a] = reduce[a] ? 1 : 0; q->lo[a] = q->hi[a] = 0;
    if (q->red[a]) {
      // The reference adds the Grid's first active index to a range that already counts from it (output.c:789-790: k = kstart ..
      // kend, then k+kl), so the zones it sums lie nghost further up than the slice and may be ghost zones: a range may reach into
      // them, never past the arrays (EdgeFlux has no ghost zones: its one extra plane is the limit).
      const int gh = (N > 1 && expr != AA_OUT_FLUX) ? AA_NGHOST_ : 0;
      const int first = -gh, last = (expr == AA_OUT_FLUX) ? N : N - 1 + gh;
      if (lo[a] < first || hi[a] < lo[a] || hi[a] > last)
        return aa_fail(-1, "[%s]: zones %d .. %d along x%d of a Grid whose arrays hold %d .. %d", who, lo[a], hi[a], a + 1, first, last);
      q->lo[a] = lo[a]; q->hi[a] = hi[a]; q->n[a] = 1; q->sum = 1;
      q->factor = q->factor/(Real)(hi[a] - lo[a] + 1);
    } else q->n[a] = (unsigned)N;
    *nout *= q->n[a];
  }
  if (*nout > 0xfffffffbull) return aa_fail(-1, "[%s]: %llu elements (the kernel indexes the payload with 32 bits)", who, *nout);
  return 0;
}

// `n` elements of `es` bytes (8: the payload, mm gets its minimum / maximum; 1: the gray bytes), piece by piece through the face-state
// area and the bounce buffer, as dump.hip does it
static int out_run(aa_grid *g, const OutDesc &q, unsigned long long n, size_t es, Real dmin, Real sfact, bool scaled, void *host_dst)
{
  { int rc = dump_prepare(g); if (rc) return rc; }
  if (!g->out_part) {
    HIPCHK(hipMalloc((void**)&g->out_part, (size_t)(4*AA_OUT_PART_BLOCKS + 4)*sizeof(Real)));
    HIPCHK(hipHostMalloc((void**)&g->out_mm_host, 4*sizeof(double)));
  }
  if (q.ex == AA_OUT_FLUX) { int rc = aa_edgeflux_ready(g); if (rc) return rc; }
  g->inner_swept = false;          // the face-state area is the staging buffer (see aa_integrate_begin in athena_amd.h)
  const size_t half = g->dump_cap*sizeof(float);          // bytes per half of the bounce buffer = per staging slot
  const unsigned long long per = half/es;
  char *stage = (char*)g->d.LR, *pin = (char*)g->dump_host, *out = (char*)host_dst;
  Real *mm = g->out_part + 4*AA_OUT_PART_BLOCKS;
  long long prev0 = -1; size_t prevn = 0; int c = 0;
  for (unsigned long long p0 = 0; p0 < n; p0 += per, c++) {
    const unsigned cnt = (unsigned)((p0 + per <= n) ? per : n - p0);
    const int slot = c & 1;
    char *dev = stage + (size_t)slot*half;
    {
      Scope sc(g, es == 8 ? "outdata" : "outdata_gray");
      if (es == 8) {
        const int nb = launch_out_payload(g->d, q, p0, cnt, (Real*)dev, g->out_part, g->st);
        launch_out_fold(g->out_part, nb, mm, p0 == 0, g->st);
      } else launch_out_gray(g->d, q, dmin, sfact, scaled, p0, cnt, (unsigned char*)dev, g->st);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(g->dump_ev[slot], g->st));
    HIPCHK(hipStreamWaitEvent(g->dump_st, g->dump_ev[slot], 0));
    HIPCHK(hipMemcpyAsync(pin + (size_t)slot*half, dev, (size_t)cnt*es, hipMemcpyDeviceToHost, g->dump_st));
    HIPCHK(hipEventRecord(g->dump_ev[2 + slot], g->dump_st));
    if (prev0 >= 0) {
      HIPCHK(hipEventSynchronize(g->dump_ev[2 + (slot ^ 1)]));
      memcpy(out + (size_t)prev0*es, pin + (size_t)(slot ^ 1)*half, prevn);
    }
    prev0 = (long long)p0; prevn = (size_t)cnt*es;
  }
  if (prev0 >= 0) {
    const int slot = (c - 1) & 1;
    HIPCHK(hipEventSynchronize(g->dump_ev[2 + slot]));
    memcpy(out + (size_t)prev0*es, pin + (size_t)slot*half, prevn);
  }
  if (es == 8) {
    HIPCHK(hipMemcpyAsync(g->out_mm_host, mm, 4*sizeof(double), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
  }
  return 0;
}

extern "C" {

int aa_outdata_dims(aa_grid *g, int expr, const int reduce[3], const int lo[3], const int hi[3], int dims[3])
{
  OutDesc q; unsigned long long n;
  if (!dims) return aa_fail(-1, "[aa_outdata_dims]: null argument");
  { int rc = out_describe(g, "aa_outdata_dims", expr, reduce, lo, hi, &q, &n); if (rc) return rc; }
  for (int a = 0; a < 3; a++) dims[a] = (int)q.n[a];
  return 0;
}

int aa_outdata(aa_grid *g, int expr, const int reduce[3], const int lo[3], const int hi[3], double *host_dst, int dims[3],
               double *dmin, double *dmax)
{
  OutDesc q; unsigned long long n;
  if (!host_dst || !dims || !dmin || !dmax) return aa_fail(-1, "[aa_outdata]: null argument");
  { int rc = out_describe(g, "aa_outdata", expr, reduce, lo, hi, &q, &n); if (rc) return rc; }
  { int rc = out_run(g, q, n, 8, 0.0, 0.0, false, host_dst); if (rc) return rc; }
  for (int a = 0; a < 3; a++) dims[a] = (int)q.n[a];
  *dmin = g->out_mm_host[0]; *dmax = g->out_mm_host[2];
  return 0;
}

int aa_outdata_gray(aa_grid *g, int expr, const int reduce[3], const int lo[3], const int hi[3], double dmin, double dmax,
                    unsigned char *host_dst, int dims[3])
{
  OutDesc q; unsigned long long n;
  if (!host_dst || !dims) return aa_fail(-1, "[aa_outdata_gray]: null argument");
  { int rc = out_describe(g, "aa_outdata_gray", expr, reduce, lo, hi, &q, &n); if (rc) return rc; }
  int kept = 0;
  for (int a = 0; a < 3; a++) if (q.n[a] > 1) kept++;
  if (kept > 2) return aa_fail(-1, "[aa_outdata_gray]: the payload is %u x %u x %u: an image is a 2-D slice (output_pgm.c:37)", q.n[0], q.n[1], q.n[2]);
  const double max_min = (dmax - dmin)*(1.0 + FLT_EPSILON);      // output_pgm.c:94
  const bool scaled = max_min > 0.0;
  const double sfact = scaled ? 256.0/max_min : 0.0;
  { int rc = out_run(g, q, n, 1, dmin, sfact, scaled, host_dst); if (rc) return rc; }
  for (int a = 0; a < 3; a++) dims[a] = (int)q.n[a];
  return 0;
}

}  // extern "C"
