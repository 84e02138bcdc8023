// restart.hip -- the payload of the reference's restart dumps (restart.c:463-983, read back by restart_grids :52-456) to and
// from the resident state.
//
// A restart file holds, per Grid and per variable, exactly the ACTIVE zones [k][j][i] in double precision -- the SoA arrays
// of DevGrid with the ghost shell stripped -- one labelled "section" after the other:
//   DENSITY | 1-MOMENTUM | 2-MOMENTUM | 3-MOMENTUM | ENERGY | EDGEFLUX (ion radiation: (Nx1+1)(Nx2+1)(Nx3+1), dense) | SCALAR n
// A section travels in pieces through the machinery of the data dumps (dump.hip): the idle face-state area as staging buffer,
// the page-locked bounce buffer of two halves, the second stream and its events, the threaded host copy.
//   get: a streaming kernel gathers a piece in file order into a staging slot, the copy of one piece overlaps the kernel and
//        the host copy of its neighbours (as aa_dump_section);
//   put: the inverse -- host -> bounce half -> staging slot -> a scatter kernel that writes ACTIVE zones only.
// EDGEFLUX is dense on the device: the same pipeline without kernels and without the staging slots.
// A piece is a range of the section's doubles, not a number of rows: with an odd Nx1 the two doubles of a thread may lie
// in two rows, and a piece may begin and end inside one.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include "api_internal.h"

using namespace aa;

// doubles [first, first + n) of a section of variable array `src` (one field of DevGrid.U), first = row0*Nx1 + i0 with
// row = k*Nx2 + j over the active zones; dst is 16-byte aligned.  Two consecutive doubles per thread, stored at once; every
// load is unconditional (past the end of the piece: the last double again).
__global__ void __launch_bounds__(256) k_rst_gather(DevGrid g, const Real *__restrict__ src, unsigned row0, unsigned i0, unsigned n,
                                                    Real *__restrict__ dst)
{
  const unsigned o0 = 2u*(blockIdx.x*256u + threadIdx.x);
  if (o0 >= n) return;
  const unsigned nx1 = (unsigned)g.Nx1, nx2 = (unsigned)g.Nx2;
  Real v[2];
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const unsigned o = (o0 + q < n) ? o0 + q : n - 1u;
    const unsigned t = i0 + o, r = t/nx1, i = t - r*nx1, row = row0 + r;
    const unsigned k = row/nx2, j = row - k*nx2;
    v[q] = src[(long)(k + (unsigned)g.ks)*g.sK + (long)(j + (unsigned)g.js)*g.sJ + (long)(i + AA_NGHOST_)];
  }
  if (o0 + 1u < n) *(double2*)(dst + o0) = make_double2(v[0], v[1]);
  else dst[o0] = v[0];
}

// the inverse: doubles [first, first + n) of a section from `src` (16-byte aligned) into the active zones of `dst`
__global__ void __launch_bounds__(256) k_rst_scatter(DevGrid g, Real *__restrict__ dst, unsigned row0, unsigned i0, unsigned n,
                                                     const Real *__restrict__ src)
{
  const unsigned o0 = 2u*(blockIdx.x*256u + threadIdx.x);
  if (o0 >= n) return;
  const unsigned nx1 = (unsigned)g.Nx1, nx2 = (unsigned)g.Nx2;
  Real v[2];
  const bool pair = o0 + 1u < n;
  if (pair) { const double2 w = *(const double2*)(src + o0); v[0] = w.x; v[1] = w.y; }
  else v[0] = v[1] = src[o0];
#pragma unroll
  for (int q = 0; q < 2; q++) {
    if (q && !pair) break;
    const unsigned t = i0 + o0 + q, r = t/nx1, i = t - r*nx1, row = row0 + r;
    const unsigned k = row/nx2, j = row - k*nx2;
    dst[(long)(k + (unsigned)g.ks)*g.sK + (long)(j + (unsigned)g.js)*g.sJ + (long)(i + AA_NGHOST_)] = v[q];
  }
}

// ---- the whole payload in one pass (aa_rst_snapshot_begin) ------------------------------------------------------------------
// where the sections of a Grid begin in a snapshot buffer, in doubles: file order, every section 16-byte aligned
__host__ __device__ static inline unsigned long long rst_pad2(unsigned long long x) { return (x + 1ull) & ~1ull; }

// two consecutive doubles of a section at once (p 16-byte aligned).  Non-temporal: nothing on the device reads the snapshot back
// but the copy engine; measured against plain stores in DESIGN.md section 8
__device__ __forceinline__ void rst_store2(Real *p, Real a, Real b)
{
  typedef double rst_v2d __attribute__((ext_vector_type(2)));
  rst_v2d v = {a, b};
  __builtin_nontemporal_store(v, (rst_v2d*)p);
}

// Every section of the n active zones that is not EDGEFLUX -- d, M1, M2, M3, E at f*S, scalar s at scal0 + s*S doubles -- to the
// snapshot buffer dst.  Thread t owns the doubles o = 2t, 2t + 1 of the flat index o = (k*Nx2 + j)*Nx1 + i (a row may end between
// them: odd Nx1): it computes either zone's address once, loads every field of both (unconditionally: past the end the last zone
// again) and stores one 16-byte pair per section; only the thread that holds the end of a Grid with odd n stores one word.
// Zone indices fit 32 bits (the caller refuses the rest), section offsets are 64 bits.  No LDS, no scratch.
template <int NS>
__global__ void __launch_bounds__(256) k_rst_payload(DevGrid g, unsigned n, unsigned long long S, unsigned long long scal0,
                                                     Real *__restrict__ dst)
{
  const unsigned long long t = (unsigned long long)blockIdx.x*256ull + threadIdx.x;
  if (2ull*t >= (unsigned long long)n) return;
  const unsigned o0 = 2u*(unsigned)t;
  const unsigned nx1 = (unsigned)g.Nx1, nx2 = (unsigned)g.Nx2;
  Real v[2][5 + NS];
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const unsigned o = (o0 + q < n) ? o0 + q : n - 1u;      // (n <= 2^32 - 2: no wrap)
    const unsigned r = o/nx1, i = o - r*nx1;
    const unsigned k = r/nx2, j = r - k*nx2;
    const long m = (long)(k + (unsigned)g.ks)*g.sK + (long)(j + (unsigned)g.js)*g.sJ + (long)(i + AA_NGHOST_);
#pragma unroll
    for (int f = 0; f < 5 + NS; f++) v[q][f] = g.U[(long)f*g.nc + m];
  }
  const bool pair = o0 + 1u < n;
#pragma unroll
  for (int f = 0; f < 5 + NS; f++) {
    Real *s = dst + (f < 5 ? (unsigned long long)f*S : scal0 + (unsigned long long)(f - 5)*S) + o0;
    if (pair) rst_store2(s, v[0][f], v[1][f]);
    else s[0] = v[0][f];
  }
}

static int rst_nsections(const aa_grid *g) { return 5 + (g->p.ion ? 1 : 0) + g->p.nscal; }
static bool rst_is_edgeflux(const aa_grid *g, int s) { return g->p.ion && s == 5; }
// the field of DevGrid.U behind a section that is not EDGEFLUX
static int rst_section_var(const aa_grid *g, int s) { return s < 5 ? s : s - (g->p.ion ? 1 : 0); }

static long long rst_doubles(const aa_grid *g, int s)
{
  const int *nx = g->p.Nx;
  if (rst_is_edgeflux(g, s)) return (long long)(nx[0] + 1)*(nx[1] + 1)*(nx[2] + 1);
  return (long long)nx[0]*nx[1]*nx[2];
}

// where section s begins in a snapshot buffer, in doubles (s = rst_nsections: where the payload ends): the sections one after the
// other in file order, each start rounded up to 2 doubles
static unsigned long long rst_snapshot_offset(const aa_grid *g, int s)
{
  unsigned long long off = 0;
  for (int q = 0; q < s; q++) off += rst_pad2((unsigned long long)rst_doubles(g, q));
  return off;
}

void rst_snapshot_free(aa_grid *g)
{
  for (aa_grid::RstSlot &s : g->rst_snap) {
    if (s.dev) hipFree(s.dev);
    if (s.host) hipHostFree(s.host);
    if (s.staged) hipEventDestroy(s.staged);
    if (s.done) hipEventDestroy(s.done);
    s = aa_grid::RstSlot();
  }
}

// one Grid on one device (the current one); `n` doubles of the section from its start (a slab's share of EDGEFLUX may leave
// out the plane its upper neighbour owns)
int rst_section_grid(aa_grid *g, int section, double *host, long long n, int put)
{
  { int rc = dump_prepare(g); if (rc) return rc; }
  g->inner_swept = false;          // the face-state area is the staging buffer (see aa_integrate_begin in athena_amd.h)
  const bool ef = rst_is_edgeflux(g, section);
  if (ef && !put) { int rc = aa_edgeflux_ready(g); if (rc) return rc; }
  const size_t per = g->dump_cap/2;                       // doubles per half: even, so that every piece starts 16-byte aligned
  Real *field = ef ? g->d.edgeflux : g->d.U + (size_t)rst_section_var(g, section)*(size_t)g->d.nc;
  Real *stage = g->d.LR, *pinned = (Real*)g->dump_host;
  const unsigned nx1 = (unsigned)g->d.Nx1;
  if (put) {
    // whatever is queued on the Grid's stream may still read the state and the staging area
    HIPCHK(hipEventRecord(g->dump_ev[0], g->st));
    HIPCHK(hipStreamWaitEvent(g->dump_st, g->dump_ev[0], 0));
  }
  long long prev_first = -1; size_t prev_n = 0; int c = 0;
  for (long long first = 0; first < n; first += (long long)per, c++) {
    const size_t np = (first + (long long)per <= n) ? per : (size_t)(n - first);
    const int slot = c & 1;
    Real *dev = ef ? field + first : stage + (size_t)slot*per, *pin = pinned + (size_t)slot*per;
    const unsigned row0 = (unsigned)(first/nx1), i0 = (unsigned)(first - (long long)row0*nx1);
    const unsigned blocks = (unsigned)((np + 511)/512);
    if (!put) {
      if (!ef) {
        { Scope sc(g, "rst_gather");
          hipLaunchKernelGGL(k_rst_gather, dim3(blocks), dim3(256), 0, g->st, (DevGrid)g->d, (const Real*)field, row0, i0, (unsigned)np, dev); }
        HIPCHK(hipGetLastError());
      }
      HIPCHK(hipEventRecord(g->dump_ev[slot], g->st));
      HIPCHK(hipStreamWaitEvent(g->dump_st, g->dump_ev[slot], 0));
      HIPCHK(hipMemcpyAsync(pin, dev, np*sizeof(Real), hipMemcpyDeviceToHost, g->dump_st));
      HIPCHK(hipEventRecord(g->dump_ev[2 + slot], g->dump_st));
      if (prev_first >= 0) {       // the piece before this one: hand it out while this one travels
        HIPCHK(hipEventSynchronize(g->dump_ev[2 + (slot ^ 1)]));
        dump_copy_out((float*)(host + prev_first), (const float*)(pinned + (size_t)(slot ^ 1)*per), 2*prev_n);
      }
    } else {
      if (c >= 2) {                // this half's last piece has left the host, and its staging slot has been scattered
        HIPCHK(hipEventSynchronize(g->dump_ev[2 + slot]));
        if (!ef) HIPCHK(hipStreamWaitEvent(g->dump_st, g->dump_ev[slot], 0));
      }
      dump_copy_out((float*)pin, (const float*)(host + first), 2*np);
      HIPCHK(hipMemcpyAsync(dev, pin, np*sizeof(Real), hipMemcpyHostToDevice, g->dump_st));
      HIPCHK(hipEventRecord(g->dump_ev[2 + slot], g->dump_st));
      if (!ef) {
        HIPCHK(hipStreamWaitEvent(g->st, g->dump_ev[2 + slot], 0));
        { Scope sc(g, "rst_scatter");
          hipLaunchKernelGGL(k_rst_scatter, dim3(blocks), dim3(256), 0, g->st, (DevGrid)g->d, field, row0, i0, (unsigned)np, (const Real*)dev); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(g->dump_ev[slot], g->st));
      }
    }
    prev_first = first; prev_n = np;
  }
  if (!put) {
    if (prev_first >= 0) {
      const int slot = (c - 1) & 1;
      HIPCHK(hipEventSynchronize(g->dump_ev[2 + slot]));
      dump_copy_out((float*)(host + prev_first), (const float*)(pinned + (size_t)slot*per), 2*prev_n);
    }
    return 0;
  }
  // every piece has landed before the call returns: the next user of the state or of the staging area finds them complete
  HIPCHK(hipStreamSynchronize(g->dump_st));
  HIPCHK(hipStreamSynchronize(g->st));
  g->cfl_ready = false; g->inner_swept = false; g->active_dirty = true;      // the device holds what no host block does
  if (ef) g->ef_stale = false;
  return 0;
}

// ---- boxes: a part [lo, lo + n) of a section, in the section's own index space (active zones; the (Nx+1)^3 face indices
// for EDGEFLUX), to and from a contiguous host block [k][j][i] -- what a run resumed on other cuts reads from every source file
// that meets its Grid, and what a dump written for other cuts takes out of the resident state.
//
// `base` is the field at the box's first element, sK / sJ the field's strides; doubles [row0*n1, row0*n1 + n) of the box with
// row = k*n2 + j over the box's rows.  One thread per double, lanes along i: a box narrower than a wavefront (an x1 cut) packs
// several rows into one wave, a wide one keeps 512-byte requests per row.  No arithmetic, addresses only.
__global__ void __launch_bounds__(256) k_rst_box_gather(const Real *__restrict__ base, long sK, long sJ, unsigned n1, unsigned n2,
                                                        unsigned row0, unsigned n, Real *__restrict__ dst)
{
  const unsigned o = blockIdx.x*256u + threadIdx.x;
  if (o >= n) return;
  const unsigned r = o/n1, i = o - r*n1, row = row0 + r;
  const unsigned k = row/n2, j = row - k*n2;
  dst[o] = base[(long)k*sK + (long)j*sJ + (long)i];
}

__global__ void __launch_bounds__(256) k_rst_box_scatter(Real *__restrict__ base, long sK, long sJ, unsigned n1, unsigned n2,
                                                         unsigned row0, unsigned n, const Real *__restrict__ src)
{
  const unsigned o = blockIdx.x*256u + threadIdx.x;
  if (o >= n) return;
  const unsigned r = o/n1, i = o - r*n1, row = row0 + r;
  const unsigned k = row/n2, j = row - k*n2;
  base[(long)k*sK + (long)j*sJ + (long)i] = src[o];
}

// one Grid on one device (the current one).  Pieces of whole box rows through the two halves of the bounce buffer, as
// rst_section_grid; EDGEFLUX too goes through the staging slots here (a box of it is not contiguous on the device).
static int rst_box_grid(aa_grid *g, int section, const int lo[3], const int nb[3], double *host, int put)
{
  { int rc = dump_prepare(g); if (rc) return rc; }
  g->inner_swept = false;          // the face-state area is the staging buffer (see aa_integrate_begin in athena_amd.h)
  const bool ef = rst_is_edgeflux(g, section);
  // (put as well: the entries outside the box stay what a reader would have found)
  if (ef) { int rc = aa_edgeflux_ready(g); if (rc) return rc; }
  Real *base; long sK, sJ;
  if (ef) {
    sJ = (long)g->d.Nx1 + 1; sK = sJ*((long)g->d.Nx2 + 1);
    base = g->d.edgeflux + (long)lo[2]*sK + (long)lo[1]*sJ + (long)lo[0];
  } else {
    sJ = g->d.sJ; sK = g->d.sK;
    base = g->d.U + (size_t)rst_section_var(g, section)*(size_t)g->d.nc
         + (long)(lo[2] + g->d.ks)*sK + (long)(lo[1] + g->d.js)*sJ + (long)(lo[0] + AA_NGHOST_);
  }
  const unsigned n1 = (unsigned)nb[0], n2 = (unsigned)nb[1];
  const long long nrows = (long long)nb[1]*nb[2];
  const size_t per = g->dump_cap/2;                       // doubles per half
  const long long rows_per = (long long)(per/n1);
  if (rows_per < 1) return aa_fail(-1, "[aa_rst_section_box]: a row of %u doubles does not fit the bounce buffer (%zu)", n1, per);
  Real *stage = g->d.LR, *pinned = (Real*)g->dump_host;
  if (put) {
    // whatever is queued on the Grid's stream may still read the state and the staging area
    HIPCHK(hipEventRecord(g->dump_ev[0], g->st));
    HIPCHK(hipStreamWaitEvent(g->dump_st, g->dump_ev[0], 0));
  }
  long long prev_first = -1; size_t prev_n = 0; int c = 0;
  for (long long row0 = 0; row0 < nrows; row0 += rows_per, c++) {
    const long long nr = (row0 + rows_per <= nrows) ? rows_per : nrows - row0;
    const size_t np = (size_t)nr*n1;
    const long long first = row0*(long long)n1;
    const int slot = c & 1;
    Real *dev = stage + (size_t)slot*per, *pin = pinned + (size_t)slot*per;
    const unsigned blocks = (unsigned)((np + 255)/256);
    if (!put) {
      { Scope sc(g, "rst_box_gather");
        hipLaunchKernelGGL(k_rst_box_gather, dim3(blocks), dim3(256), 0, g->st, (const Real*)base, sK, sJ, n1, n2, (unsigned)row0, (unsigned)np, dev); }
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(g->dump_ev[slot], g->st));
      HIPCHK(hipStreamWaitEvent(g->dump_st, g->dump_ev[slot], 0));
      HIPCHK(hipMemcpyAsync(pin, dev, np*sizeof(Real), hipMemcpyDeviceToHost, g->dump_st));
      HIPCHK(hipEventRecord(g->dump_ev[2 + slot], g->dump_st));
      if (prev_first >= 0) {       // the piece before this one: hand it out while this one travels
        HIPCHK(hipEventSynchronize(g->dump_ev[2 + (slot ^ 1)]));
        dump_copy_out((float*)(host + prev_first), (const float*)(pinned + (size_t)(slot ^ 1)*per), 2*prev_n);
      }
    } else {
      if (c >= 2) {                // this half's last piece has left the host, and its staging slot has been scattered
        HIPCHK(hipEventSynchronize(g->dump_ev[2 + slot]));
        HIPCHK(hipStreamWaitEvent(g->dump_st, g->dump_ev[slot], 0));
      }
      dump_copy_out((float*)pin, (const float*)(host + first), 2*np);
      HIPCHK(hipMemcpyAsync(dev, pin, np*sizeof(Real), hipMemcpyHostToDevice, g->dump_st));
      HIPCHK(hipEventRecord(g->dump_ev[2 + slot], g->dump_st));
      HIPCHK(hipStreamWaitEvent(g->st, g->dump_ev[2 + slot], 0));
      { Scope sc(g, "rst_box_scatter");
        hipLaunchKernelGGL(k_rst_box_scatter, dim3(blocks), dim3(256), 0, g->st, base, sK, sJ, n1, n2, (unsigned)row0, (unsigned)np, (const Real*)dev); }
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(g->dump_ev[slot], g->st));
    }
    prev_first = first; prev_n = np;
  }
  if (!put) {
    if (prev_first >= 0) {
      const int slot = (c - 1) & 1;
      HIPCHK(hipEventSynchronize(g->dump_ev[2 + slot]));
      dump_copy_out((float*)(host + prev_first), (const float*)(pinned + (size_t)slot*per), 2*prev_n);
    }
    return 0;
  }
  // every piece has landed before the call returns: the next user of the state or of the staging area finds them complete
  HIPCHK(hipStreamSynchronize(g->dump_st));
  HIPCHK(hipStreamSynchronize(g->st));
  g->cfl_ready = false; g->inner_swept = false; g->active_dirty = true;      // the device holds what no host block does
  if (ef) g->ef_stale = false;
  return 0;
}

static int rst_box_call(const char *who, aa_grid *g, int section, const int lo[3], const int n[3], double *host, int put)
{
  if (!g || !lo || !n || !host) return aa_fail(-1, "[%s]: null argument", who);
  if (section < 0 || section >= rst_nsections(g)) return aa_fail(-1, "[%s]: section %d of %d", who, section, rst_nsections(g));
  if (!g->slab.empty())
    return aa_fail(-1, "[%s]: a Grid cut into slabs inside the library (aa_params.nslab > 1) takes whole sections only", who);
  const int e = rst_is_edgeflux(g, section) ? 1 : 0;
  for (int d = 0; d < 3; d++) {
    const int dim = g->p.Nx[d] + e;
    if (lo[d] < 0 || n[d] < 1 || lo[d] > dim - n[d])
      return aa_fail(-1, "[%s]: box [%d, %d) along x%d is not inside the section's [0, %d)", who, lo[d], lo[d] + n[d], d + 1, dim);
  }
  return rst_box_grid(g, section, lo, n, host, put);
}

extern "C" {

int aa_rst_sections(const aa_grid *g) { return g ? rst_nsections(g) : 0; }

int aa_rst_section_label(const aa_grid *g, int section, char *buf, int n)
{
  if (!g || !buf || n <= 0) return aa_fail(-1, "[aa_rst_section_label]: null argument");
  if (section < 0 || section >= rst_nsections(g)) return aa_fail(-1, "[aa_rst_section_label]: section %d of %d", section, rst_nsections(g));
  static const char *const lab[5] = {"DENSITY", "1-MOMENTUM", "2-MOMENTUM", "3-MOMENTUM", "ENERGY"};
  if (section < 5) snprintf(buf, (size_t)n, "%s", lab[section]);
  else if (rst_is_edgeflux(g, section)) snprintf(buf, (size_t)n, "EDGEFLUX");
  else snprintf(buf, (size_t)n, "SCALAR %d", rst_section_var(g, section) - 5);
  return 0;
}

long long aa_rst_section_doubles(const aa_grid *g, int section)
{
  if (!g || section < 0 || section >= rst_nsections(g)) return 0;
  return rst_doubles(g, section);
}

int aa_rst_section_get(aa_grid *g, int section, double *host)
{
  if (!g || !host) return aa_fail(-1, "[aa_rst_section_get]: null argument");
  if (section < 0 || section >= rst_nsections(g)) return aa_fail(-1, "[aa_rst_section_get]: section %d of %d", section, rst_nsections(g));
  if (!g->slab.empty()) return slabs_rst_section(g, section, host, 0);
  return rst_section_grid(g, section, host, rst_doubles(g, section), 0);
}

int aa_rst_section_put(aa_grid *g, int section, const double *host)
{
  if (!g || !host) return aa_fail(-1, "[aa_rst_section_put]: null argument");
  if (section < 0 || section >= rst_nsections(g)) return aa_fail(-1, "[aa_rst_section_put]: section %d of %d", section, rst_nsections(g));
  ion_lean_forget(g);
  if (!g->slab.empty()) return slabs_rst_section(g, section, const_cast<double*>(host), 1);
  return rst_section_grid(g, section, const_cast<double*>(host), rst_doubles(g, section), 1);
}

int aa_rst_section_get_box(aa_grid *g, int section, const int lo[3], const int n[3], double *host)
{ return rst_box_call("aa_rst_section_get_box", g, section, lo, n, host, 0); }

int aa_rst_section_put_box(aa_grid *g, int section, const int lo[3], const int n[3], const double *host)
{ if (g) ion_lean_forget(g); return rst_box_call("aa_rst_section_put_box", g, section, lo, n, const_cast<double*>(host), 1); }

// ---- snapshots: the whole payload made by one kernel and one device copy, brought to the host beside the run (see athena_amd.h).
// The route of aa_dump_snapshot_* (dump.hip) on the same stream of copies; one slot, in doubles.
long long aa_rst_snapshot_bytes(const aa_grid *g)
{
  if (!g) return 0;
  return (long long)(rst_snapshot_offset(g, rst_nsections(g))*sizeof(Real));      // (where a section past the last would begin)
}

#define RST_SLOT(fn) \
  if (!g) return aa_fail(-1, "[" fn "]: null argument"); \
  if (slot < 0 || slot >= AA_RST_SLOTS) return aa_fail(-1, "[" fn "]: slot %d of %d", slot, AA_RST_SLOTS); \
  aa_grid::RstSlot &s = g->rst_snap[slot]

int aa_rst_snapshot_begin(aa_grid *g, int slot, long long max_bytes)
{
  RST_SLOT("aa_rst_snapshot_begin");
  if (g->link || !g->slab.empty())
    return aa_fail(-1, "[aa_rst_snapshot_begin]: a Grid cut into slabs takes no snapshot: the synchronous aa_rst_section_get is the path there");
  if (g->one_d) return aa_fail(-1, "[aa_rst_snapshot_begin]: a 1-D Grid takes no snapshot: the synchronous aa_rst_section_get is the path there");
  if (s.held) return aa_fail(-1, "[aa_rst_snapshot_begin]: slot %d is still held (aa_rst_snapshot_release frees it)", slot);
  const unsigned long long n = (unsigned long long)rst_doubles(g, 0);
  if (n > 0xfffffffdull) return aa_fail(-1, "[aa_rst_snapshot_begin]: %llu zones (the kernel indexes zones with 32 bits)", n);
  const long long bytes = aa_rst_snapshot_bytes(g);
  if (bytes > max_bytes)
    return aa_fail(-1, "[aa_rst_snapshot_begin]: a payload of %lld bytes, max_bytes = %lld", bytes, max_bytes);
  { int rc = dump_stream(g); if (rc) return rc; }
  if (!s.dev) {                    // first use; kept until aa_destroy
    const size_t cap = (size_t)bytes/sizeof(Real);
    Real *dev = nullptr, *host = nullptr;
    HIPCHK(hipMalloc((void**)&dev, cap*sizeof(Real)));
    if (hipHostMalloc((void**)&host, cap*sizeof(Real)) != hipSuccess) {
      (void)hipGetLastError(); hipFree(dev);
      return aa_fail(-2, "[aa_rst_snapshot_begin]: %zu bytes of page-locked memory", cap*sizeof(Real));
    }
    // (the padding words between sections are never written by the kernel: defined once, so that the copy moves no stale memory)
    if (hipMemset(dev, 0, cap*sizeof(Real)) != hipSuccess) { (void)hipGetLastError(); hipFree(dev); hipHostFree(host); return aa_fail(-2, "[aa_rst_snapshot_begin]: hipMemset"); }
    s.dev = dev; s.host = host; s.cap = cap;
    g->bytes += (long long)(cap*sizeof(Real));
    HIPCHK(hipEventCreateWithFlags(&s.staged, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  }
  // EdgeFlux first: the one-kernel sub-cycle fills it on demand (exactly as aa_rst_section_get asks for it)
  if (g->p.ion) { int rc = aa_edgeflux_ready(g); if (rc) return rc; }
  {
    Scope sc(g, "rst_snapshot");
    const unsigned blocks = (unsigned)((n + 511ull)/512ull);
    const unsigned long long S = rst_pad2(n), scal0 = rst_snapshot_offset(g, 5 + (g->p.ion ? 1 : 0));
    with_ns(g->p.nscal, [&](auto NS) {
      hipLaunchKernelGGL((k_rst_payload<NS>), dim3(blocks), dim3(256), 0, g->st, (DevGrid)g->d, (unsigned)n, S, scal0, s.dev);
    });
  }
  HIPCHK(hipGetLastError());
  if (g->p.ion) {                  // dense on the device: one copy into its place in file order
    Scope sc(g, "rst_snapshot_ef");
    HIPCHK(hipMemcpyAsync(s.dev + rst_snapshot_offset(g, 5), g->d.edgeflux, (size_t)rst_doubles(g, 5)*sizeof(Real),
                          hipMemcpyDeviceToDevice, g->st));
  }
  HIPCHK(hipEventRecord(s.staged, g->st));
  HIPCHK(hipStreamWaitEvent(g->dump_st, s.staged, 0));
  HIPCHK(hipMemcpyAsync(s.host, s.dev, (size_t)bytes, hipMemcpyDeviceToHost, g->dump_st));
  HIPCHK(hipEventRecord(s.done, g->dump_st));
  s.held = true;
  return 0;
}

int aa_rst_snapshot_ready(aa_grid *g, int slot)
{
  RST_SLOT("aa_rst_snapshot_ready");
  if (!s.held) return aa_fail(-1, "[aa_rst_snapshot_ready]: slot %d holds no snapshot", slot);
  const hipError_t e = hipEventQuery(s.done);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
  return aa_fail(-2, "[aa_rst_snapshot_ready]: HIP error %s", hipGetErrorString(e));
}

int aa_rst_snapshot_wait(aa_grid *g, int slot)
{
  RST_SLOT("aa_rst_snapshot_wait");
  if (!s.held) return aa_fail(-1, "[aa_rst_snapshot_wait]: slot %d holds no snapshot", slot);
  HIPCHK(hipEventSynchronize(s.done));
  return 0;
}

const double *aa_rst_snapshot_section(aa_grid *g, int slot, int section, long long *ndoubles)
{
  if (!g || !ndoubles) { aa_fail(-1, "[aa_rst_snapshot_section]: null argument"); return nullptr; }
  if (slot < 0 || slot >= AA_RST_SLOTS) { aa_fail(-1, "[aa_rst_snapshot_section]: slot %d of %d", slot, AA_RST_SLOTS); return nullptr; }
  const aa_grid::RstSlot &s = g->rst_snap[slot];
  if (!s.held) { aa_fail(-1, "[aa_rst_snapshot_section]: slot %d holds no snapshot", slot); return nullptr; }
  if (section < 0 || section >= rst_nsections(g)) {
    aa_fail(-1, "[aa_rst_snapshot_section]: section %d of %d", section, rst_nsections(g)); return nullptr;
  }
  if (hipEventQuery(s.done) != hipSuccess) {
    (void)hipGetLastError();
    aa_fail(-1, "[aa_rst_snapshot_section]: the payload of slot %d is not on the host yet (aa_rst_snapshot_ready / _wait)", slot);
    return nullptr;
  }
  *ndoubles = rst_doubles(g, section);
  return s.host + rst_snapshot_offset(g, section);
}

int aa_rst_snapshot_release(aa_grid *g, int slot)
{
  RST_SLOT("aa_rst_snapshot_release");
  if (!s.held) return 0;
  HIPCHK(hipEventSynchronize(s.done));
  s.held = false;
  return 0;
}

// main.c:398-451 of a restarted run: the ghost zones and the radiation boundary, and NOT new_dt -- the file's dt is the next step's
int aa_resume(aa_grid *g)
{
  int rc;
  if (!g) return aa_fail(-1, "[aa_resume]: null argument");
  if ((rc = aa_bvals_mhd(g))) return rc;
  return aa_bvals_ionrad(g);
}

}  // extern "C"
