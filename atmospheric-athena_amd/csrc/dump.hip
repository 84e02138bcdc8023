// dump.hip -- the payload of the reference's data dumps (dump_vtk.c:28-327, dump_binary.c:30-266) from the resident state.
//
// Both formats are single precision over the ACTIVE zones, [k][j][i] with i fastest, one "section" after the other:
//   vtk: density (n floats) | momentum or velocity (3n, the components of a zone next to each other) | total energy or
//        pressure (n) | one section per passive scalar (n); every word big-endian (ath_bswap, dump_vtk.c:175)
//   bin: NVAR = 5 + NSCALARS sections of n floats in ConsS / PrimS order, native byte order
// with n = Nx1*Nx2*Nx3.  A section is produced in file order by one streaming kernel per piece (whole rows, as many as the
// bounce buffer holds) into the idle face-state area -- the staging buffer of aa_download_cons -- and travels from there
// through a page-locked bounce buffer of two halves, so that the copy of one piece overlaps the kernel and the host copy of
// its neighbours.  The host never touches a payload word: conversion to primitive variables (Cons1D_to_Prim1D,
// convert_var.c:389-421), the cast, the byte swap, the stripping of the ghost zones and the interleave happen here.
//
// A snapshot (aa_dump_snapshot_begin) is the same payload made whole by ONE kernel, k_dump_payload, into a device buffer of its
// own and copied to page-locked memory beside the run: two slots per Grid, nothing staged through the face-state area, no wait.
// Only the thread that drives the run calls these functions; a writer thread reads the page-locked memory and nothing else.
//
// The arithmetic is the reference's, operation by operation, in BOTH libraries: no contraction, the IEEE quotient for
// 1.0/d (the kernel is bound by bytes), so that a state gives the same file whichever library wrote it.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>
#include "api_internal.h"

#pragma clang fp contract(off)

using namespace aa;

#define DUMP_TINY_NUMBER 1.0e-20   /* defs.h.in:160 */

// variable `var` (0 d, 1..3 M or V, 4 E or P, 5 s or r) of the zone at offset m of the SoA arrays
__device__ __forceinline__ float dump_value(const DevGrid &g, int var, int prim, long m)
{
  const Real d = g.U[m];
  if (var == 0) return (float)d;
  if (!prim) return (float)g.U[(long)var*g.nc + m];
  const Real di = 1.0/d;
  if (var != 4) return (float)(g.U[(long)var*g.nc + m]*di);
  const Real M1 = g.U[g.nc + m], M2 = g.U[2*g.nc + m], M3 = g.U[3*g.nc + m], E = g.U[4*g.nc + m];
  Real P = E - 0.5*(M1*M1 + M2*M2 + M3*M3)*di;
  P *= g.Gamma_1;
  P = (P > DUMP_TINY_NUMBER) ? P : DUMP_TINY_NUMBER;      // the reference's MAX(): a NaN pressure becomes TINY_NUMBER
  return (float)P;
}

// `nwords` floats of one section, starting at the first zone of row `row0` (row = k*Nx2 + j over the active zones), to dst
// (16-byte aligned).  VEC: the 3-vector section, word o = component o % 3 of zone o / 3; else variable `var`.  Every thread
// makes four consecutive words of the payload and stores them at once; only the last thread of a piece can hold fewer.
template <bool VEC>
__global__ void __launch_bounds__(256) k_dump_section(DevGrid g, int var, int prim, int swap, int row0, unsigned nwords, float *dst)
{
  const unsigned o0 = 4u*(blockIdx.x*256u + threadIdx.x);
  if (o0 >= nwords) return;
  const unsigned nx1 = (unsigned)g.Nx1, nx2 = (unsigned)g.Nx2;
  unsigned w[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    // (past the end of the piece: the last word again -- every load is unconditional, so the four of them go out together)
    const unsigned o = (o0 + q < nwords) ? o0 + q : nwords - 1u;
    const unsigned z = VEC ? o/3u : o, c = VEC ? o - 3u*z : 0u;
    const unsigned r = z/nx1, i = z - r*nx1, row = (unsigned)row0 + r;
    const unsigned k = row/nx2, j = row - k*nx2;
    const long m = (long)(k + (unsigned)g.ks)*g.sK + (long)(j + (unsigned)g.js)*g.sJ + (long)(i + AA_NGHOST_);
    const unsigned b = __float_as_uint(dump_value(g, VEC ? 1 + (int)c : var, prim, m));
    w[q] = swap ? __builtin_bswap32(b) : b;
  }
  if (o0 + 3u < nwords) *(uint4*)(dst + o0) = make_uint4(w[0], w[1], w[2], w[3]);
  else for (unsigned q = 0; o0 + q < nwords; q++) ((unsigned*)dst)[o0 + q] = w[q];
}

// ---- the whole payload in one pass (aa_dump_snapshot_begin) ---------------------------------------------------------------
// the words of zone m in ConsS / PrimS order: dump_value's operations, every field of the zone loaded once
template <int NS>
__device__ __forceinline__ void dump_zone(const DevGrid &g, int prim, long m, unsigned swap, unsigned w[5 + NS])
{
  Real u[5 + NS];
#pragma unroll
  for (int v = 0; v < 5 + NS; v++) u[v] = g.U[(long)v*g.nc + m];
  float f[5 + NS];
  f[0] = (float)u[0];
  if (!prim) {
#pragma unroll
    for (int v = 1; v < 5 + NS; v++) f[v] = (float)u[v];
  } else {
    const Real di = 1.0/u[0];
#pragma unroll
    for (int v = 1; v < 5 + NS; v++) if (v != 4) f[v] = (float)(u[v]*di);
    Real P = u[4] - 0.5*(u[1]*u[1] + u[2]*u[2] + u[3]*u[3])*di;
    P *= g.Gamma_1;
    P = (P > DUMP_TINY_NUMBER) ? P : DUMP_TINY_NUMBER;      // the reference's MAX(): a NaN pressure becomes TINY_NUMBER
    f[4] = (float)P;
  }
#pragma unroll
  for (int v = 0; v < 5 + NS; v++) { const unsigned b = __float_as_uint(f[v]); w[v] = swap ? __builtin_bswap32(b) : b; }
}

// where the sections of a payload of n zones begin in a snapshot buffer, in floats: every section 16-byte aligned
__host__ __device__ static inline unsigned long long dump_pad4(unsigned long long x) { return (x + 3ull) & ~3ull; }
__host__ __device__ static inline unsigned long long dump_snapshot_offset(bool vtk, unsigned long long n, int section)
{
  if (!vtk || section < 2) return (unsigned long long)section*dump_pad4(n);      // bin: n floats each; vtk: n | 3n | n | n ...
  return dump_pad4(3ull*n) + (unsigned long long)(section - 1)*dump_pad4(n);
}

// four consecutive words of a section at once (p 16-byte aligned).  Non-temporal: nothing on the device reads the snapshot back;
// measured against plain stores at 512^3 with the scalar: vtk 2.16 against 2.27 ms, bin 2.30 against 2.61
__device__ __forceinline__ void dump_store4(unsigned *p, unsigned a, unsigned b, unsigned c, unsigned d)
{
  typedef unsigned dump_v4u __attribute__((ext_vector_type(4)));
  dump_v4u v = {a, b, c, d};
  __builtin_nontemporal_store(v, (dump_v4u*)p);
}

// Every section of a vtk (VTK) or bin payload of the n active zones, in file order and byte order, to the snapshot buffer dst.
// Thread t owns the zones z = 4t .. 4t+3 of the flat index z = (k*Nx2 + j)*Nx1 + i (rows may end inside them): it loads their
// d, M1, M2, M3, E[, s] once and stores one uint4 per scalar section, three for the 12 words of the vtk vector section; only the
// thread that holds the end of a Grid with n % 4 != 0 stores word by word.  Zone indices fit 32 bits (the caller refuses the
// rest), word offsets do not: 3n passes 2^31 from 895^3 on.  No LDS, no scratch.
template <int NS, bool VTK>
__global__ void __launch_bounds__(256) k_dump_payload(DevGrid g, int prim, unsigned n, float *dst)
{
  const unsigned long long t = (unsigned long long)blockIdx.x*256ull + threadIdx.x;
  if (4ull*t >= (unsigned long long)n) return;
  const unsigned z0 = 4u*(unsigned)t;
  const unsigned nx1 = (unsigned)g.Nx1, nx2 = (unsigned)g.Nx2;
  unsigned w[4][5 + NS];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    // (past the end of the Grid: the last zone again -- every load is unconditional)
    const unsigned z = (z0 + q < n) ? z0 + q : n - 1u;      // (n <= 2^32 - 4: no wrap)
    const unsigned r = z/nx1, i = z - r*nx1;
    const unsigned k = r/nx2, j = r - k*nx2;
    const long m = (long)(k + (unsigned)g.ks)*g.sK + (long)(j + (unsigned)g.js)*g.sJ + (long)(i + AA_NGHOST_);
    dump_zone<NS>(g, prim, m, VTK ? 1u : 0u, w[q]);
  }
  unsigned *out = (unsigned*)dst;
  const unsigned long long S = dump_pad4(n);
  const bool whole = (unsigned long long)z0 + 3ull < (unsigned long long)n;
  if (VTK) {
    unsigned *s0 = out + z0, *s1 = out + S + 3ull*z0, *s2 = out + S + dump_pad4(3ull*n) + z0;
    if (whole) {
      dump_store4(s0, w[0][0], w[1][0], w[2][0], w[3][0]);
      dump_store4(s1, w[0][1], w[0][2], w[0][3], w[1][1]);
      dump_store4(s1 + 4, w[1][2], w[1][3], w[2][1], w[2][2]);
      dump_store4(s1 + 8, w[2][3], w[3][1], w[3][2], w[3][3]);
      dump_store4(s2, w[0][4], w[1][4], w[2][4], w[3][4]);
      if (NS) dump_store4(s2 + S, w[0][4 + NS], w[1][4 + NS], w[2][4 + NS], w[3][4 + NS]);
    } else {
#pragma unroll
      for (int q = 0; q < 3; q++) if (z0 + q < n) {
        s0[q] = w[q][0]; s1[3*q] = w[q][1]; s1[3*q + 1] = w[q][2]; s1[3*q + 2] = w[q][3]; s2[q] = w[q][4];
        if (NS) s2[S + q] = w[q][4 + NS];
      }
    }
  } else {
#pragma unroll
    for (int v = 0; v < 5 + NS; v++) {
      unsigned *s = out + (unsigned long long)v*S + z0;
      if (whole) dump_store4(s, w[0][v], w[1][v], w[2][v], w[3][v]);
      else {
#pragma unroll
        for (int q = 0; q < 3; q++) if (z0 + q < n) s[q] = w[q][v];
      }
    }
  }
}

static int dump_nsections(const aa_grid *g, int fmt)
{
  if (fmt == AA_DUMP_VTK) return 3 + g->p.nscal;
  if (fmt == AA_DUMP_BIN) return 5 + g->p.nscal;
  return 0;
}
// (variable, words per zone) of a section
static void dump_section_shape(int fmt, int section, int *var, int *ncomp)
{
  *ncomp = 1; *var = section;
  if (fmt == AA_DUMP_VTK) {
    if (section == 1) { *ncomp = 3; *var = 1; }
    else if (section == 2) *var = 4;
    else if (section >= 3) *var = 5 + (section - 3);
  }
}

void dump_release(aa_grid *g)
{
  if (g->dump_st) hipStreamSynchronize(g->dump_st);        // a snapshot in flight: its copy lands before its buffers go
  rst_snapshot_free(g);
  for (aa_grid::DumpSlot &s : g->snap) {
    if (s.dev) hipFree(s.dev);
    if (s.host) hipHostFree(s.host);
    if (s.staged) hipEventDestroy(s.staged);
    if (s.done) hipEventDestroy(s.done);
    s = aa_grid::DumpSlot();
  }
  if (g->dump_host) { hipHostFree(g->dump_host); g->dump_host = nullptr; }
  for (hipEvent_t &e : g->dump_ev) if (e) { hipEventDestroy(e); e = nullptr; }
  if (g->dump_st) { hipStreamDestroy(g->dump_st); g->dump_st = nullptr; }
  g->dump_cap = 0;
}

// floats per half of the bounce buffer (= per staging slot): what AA_DUMP_CHUNK_FLOATS asks for, at most what half the
// face-state area holds, at least one row of the vector section; a multiple of 4, so that both slots are 16-byte aligned
static size_t dump_capacity(const aa_grid *g)
{
  size_t cap = (size_t)g->d.cfg.dump_chunk;
  const size_t room = (size_t)(g->one_d ? 5 : g->two_d ? 20 : 36)*(size_t)g->d.nc;   // LR is 36*nc doubles = 72*nc floats: two slots of 36*nc (a 2-D Grid: 20*nc, a 1-D Grid: 5*nc)
  const size_t row = (size_t)3*(size_t)g->d.Nx1;
  if (cap > room) cap = room;
  if (cap < row) cap = row;
  return (cap + 3) & ~(size_t)3;
}

// the stream of the dumps' copies (the snapshots need it without the bounce buffer)
int dump_stream(aa_grid *g)
{
  if (!g->dump_st) HIPCHK(hipStreamCreateWithFlags(&g->dump_st, hipStreamNonBlocking));
  return 0;
}

int dump_prepare(aa_grid *g)
{
  if (g->dump_host) return 0;
  const size_t cap = dump_capacity(g);
  HIPCHK(hipHostMalloc((void**)&g->dump_host, 2*cap*sizeof(float)));
  g->dump_cap = cap;
  { int rc = dump_stream(g); if (rc) return rc; }
  for (hipEvent_t &e : g->dump_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return 0;
}

// bounce buffer -> the caller's memory (pageable as a rule): large pieces on a few threads, a single one does not reach the
// rate of the link (restart.hip uses it in both directions)
void dump_copy_out(float *dst, const float *src, size_t n)
{
  const size_t bytes = n*sizeof(float);
  if (bytes < ((size_t)4 << 20)) { memcpy(dst, src, bytes); return; }
  const int nth = 4;
  std::vector<std::thread> pool;
  const size_t per = ((n + nth - 1)/nth + 1023) & ~(size_t)1023;
  for (int t = 1; t < nth; t++) {
    const size_t a = (size_t)t*per; if (a >= n) break;
    const size_t len = (a + per <= n) ? per : n - a;
    pool.emplace_back([=]() { memcpy(dst + a, src + a, len*sizeof(float)); });
  }
  memcpy(dst, src, (per < n ? per : n)*sizeof(float));
  for (auto &th : pool) th.join();
}

// one Grid on one device (the current one)
static int dump_section_grid(aa_grid *g, int fmt, int prim, int section, float *host_dst)
{
  { int rc = dump_prepare(g); if (rc) return rc; }
  g->inner_swept = false;          // the face-state area is the staging buffer (see aa_integrate_begin in athena_amd.h)
  int var, ncomp; dump_section_shape(fmt, section, &var, &ncomp);
  const size_t cap = g->dump_cap, roww = (size_t)g->d.Nx1*ncomp;
  const long nrows = (long)g->d.Nx2*g->d.Nx3;
  const long rows_per = (long)(cap/roww);                 // >= 1: dump_capacity
  float *stage = (float*)g->d.LR;
  const int swap = (fmt == AA_DUMP_VTK) ? 1 : 0;          // little-endian host (ath_big_endian() == 0)
  long prev_row = -1, prev_n = 0; int c = 0;
  for (long row0 = 0; row0 < nrows; row0 += rows_per, c++) {
    const long nr = (row0 + rows_per <= nrows) ? rows_per : nrows - row0;
    const size_t nwords = (size_t)nr*roww;
    const int slot = c & 1;
    float *dev = stage + (size_t)slot*cap, *pin = g->dump_host + (size_t)slot*cap;
    {
      Scope sc(g, "dump_section");
      const unsigned blocks = (unsigned)((nwords + 1023)/1024);
      if (ncomp == 3) hipLaunchKernelGGL(k_dump_section<true>, dim3(blocks), dim3(256), 0, g->st, (DevGrid)g->d, var, prim, swap, (int)row0, (unsigned)nwords, dev);
      else            hipLaunchKernelGGL(k_dump_section<false>, dim3(blocks), dim3(256), 0, g->st, (DevGrid)g->d, var, prim, swap, (int)row0, (unsigned)nwords, dev);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(g->dump_ev[slot], g->st));
    HIPCHK(hipStreamWaitEvent(g->dump_st, g->dump_ev[slot], 0));
    HIPCHK(hipMemcpyAsync(pin, dev, nwords*sizeof(float), hipMemcpyDeviceToHost, g->dump_st));
    HIPCHK(hipEventRecord(g->dump_ev[2 + slot], g->dump_st));
    if (prev_row >= 0) {           // the piece before this one: its copy has had this kernel's time; hand it out while this one travels
      HIPCHK(hipEventSynchronize(g->dump_ev[2 + (slot ^ 1)]));
      dump_copy_out(host_dst + (size_t)prev_row*roww, g->dump_host + (size_t)(slot ^ 1)*cap, (size_t)prev_n);
    }
    prev_row = row0; prev_n = (long)nwords;
  }
  if (prev_row >= 0) {
    const int slot = (c - 1) & 1;
    HIPCHK(hipEventSynchronize(g->dump_ev[2 + slot]));
    dump_copy_out(host_dst + (size_t)prev_row*roww, g->dump_host + (size_t)slot*cap, (size_t)prev_n);
  }
  // (every slot's copy has been waited for: the next user of the face-state area on g->st finds it free)
  return 0;
}

extern "C" {

int aa_dump_sections(const aa_grid *g, int fmt) { return g ? dump_nsections(g, fmt) : 0; }

long long aa_dump_section_floats(const aa_grid *g, int fmt, int section)
{
  if (!g || section < 0 || section >= dump_nsections(g, fmt)) return 0;
  int var, ncomp; dump_section_shape(fmt, section, &var, &ncomp);
  return (long long)g->p.Nx[0]*g->p.Nx[1]*g->p.Nx[2]*ncomp;
}

int aa_dump_section(aa_grid *g, int fmt, int prim, int section, float *host_dst)
{
  if (!g || !host_dst) return aa_fail(-1, "[aa_dump_section]: null argument");
  if (fmt != AA_DUMP_VTK && fmt != AA_DUMP_BIN) return aa_fail(-1, "[aa_dump_section]: format %d (AA_DUMP_VTK or AA_DUMP_BIN)", fmt);
  if (section < 0 || section >= dump_nsections(g, fmt))
    return aa_fail(-1, "[aa_dump_section]: section %d of %d", section, dump_nsections(g, fmt));
  if (!g->slab.empty()) return slabs_dump_section(g, fmt, prim != 0, section, host_dst);
  return dump_section_grid(g, fmt, prim != 0, section, host_dst);
}

// ---- snapshots: the whole payload made by one kernel, copied beside the run (see athena_amd.h) ------------------------------
static unsigned long long snapshot_floats(const aa_grid *g, int fmt)
{
  const unsigned long long n = (unsigned long long)g->p.Nx[0]*g->p.Nx[1]*g->p.Nx[2];
  return dump_snapshot_offset(fmt == AA_DUMP_VTK, n, dump_nsections(g, fmt));      // (where a section past the last would begin)
}

long long aa_dump_snapshot_bytes(const aa_grid *g, int fmt)
{
  if (!g || !dump_nsections(g, fmt)) return 0;
  return (long long)(snapshot_floats(g, fmt)*sizeof(float));
}

#define SNAP_SLOT(fn) \
  if (!g) return aa_fail(-1, "[" fn "]: null argument"); \
  if (slot < 0 || slot >= AA_DUMP_SLOTS) return aa_fail(-1, "[" fn "]: slot %d of %d", slot, AA_DUMP_SLOTS); \
  aa_grid::DumpSlot &s = g->snap[slot]

int aa_dump_snapshot_begin(aa_grid *g, int slot, int fmt, int prim, long long max_bytes)
{
  SNAP_SLOT("aa_dump_snapshot_begin");
  if (fmt != AA_DUMP_VTK && fmt != AA_DUMP_BIN) return aa_fail(-1, "[aa_dump_snapshot_begin]: format %d (AA_DUMP_VTK or AA_DUMP_BIN)", fmt);
  if (g->link || !g->slab.empty())
    return aa_fail(-1, "[aa_dump_snapshot_begin]: a Grid cut into slabs takes no snapshot: the synchronous aa_dump_section is the path there");
  if (g->one_d) return aa_fail(-1, "[aa_dump_snapshot_begin]: a 1-D Grid takes no snapshot: the synchronous aa_dump_section is the path there");
  if (s.held) return aa_fail(-1, "[aa_dump_snapshot_begin]: slot %d is still held (aa_dump_snapshot_release frees it)", slot);
  const unsigned long long n = (unsigned long long)g->p.Nx[0]*g->p.Nx[1]*g->p.Nx[2];
  if (n > 0xfffffffbull) return aa_fail(-1, "[aa_dump_snapshot_begin]: %llu zones (the kernel indexes zones with 32 bits)", n);
  const long long bytes = aa_dump_snapshot_bytes(g, fmt);
  if (bytes > max_bytes)
    return aa_fail(-1, "[aa_dump_snapshot_begin]: a payload of %lld bytes, max_bytes = %lld", bytes, max_bytes);
  { int rc = dump_stream(g); if (rc) return rc; }
  if (!s.dev) {                    // first use: room for either format, so that the slot is never made again
    const unsigned long long fv = snapshot_floats(g, AA_DUMP_VTK), fb = snapshot_floats(g, AA_DUMP_BIN);
    const size_t cap = (size_t)(fv > fb ? fv : fb);
    float *dev = nullptr, *host = nullptr;
    HIPCHK(hipMalloc((void**)&dev, cap*sizeof(float)));
    if (hipHostMalloc((void**)&host, cap*sizeof(float)) != hipSuccess) {
      (void)hipGetLastError(); hipFree(dev);
      return aa_fail(-2, "[aa_dump_snapshot_begin]: %zu bytes of page-locked memory", cap*sizeof(float));
    }
    s.dev = dev; s.host = host; s.cap = cap;
    g->bytes += (long long)(cap*sizeof(float));
    HIPCHK(hipEventCreateWithFlags(&s.staged, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  }
  {
    Scope sc(g, "dump_snapshot");
    const unsigned blocks = (unsigned)((n + 1023ull)/1024ull);
    const bool vtk = fmt == AA_DUMP_VTK;
    with_ns(g->p.nscal, [&](auto NS) { with_flag(vtk, [&](auto VTK) {
      hipLaunchKernelGGL((k_dump_payload<NS, VTK>), dim3(blocks), dim3(256), 0, g->st, (DevGrid)g->d, prim != 0, (unsigned)n, s.dev);
    }); });
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(s.staged, g->st));
  HIPCHK(hipStreamWaitEvent(g->dump_st, s.staged, 0));
  HIPCHK(hipMemcpyAsync(s.host, s.dev, (size_t)bytes, hipMemcpyDeviceToHost, g->dump_st));
  HIPCHK(hipEventRecord(s.done, g->dump_st));
  s.held = true; s.fmt = fmt;
  return 0;
}

int aa_dump_snapshot_ready(aa_grid *g, int slot)
{
  SNAP_SLOT("aa_dump_snapshot_ready");
  if (!s.held) return aa_fail(-1, "[aa_dump_snapshot_ready]: slot %d holds no snapshot", slot);
  const hipError_t e = hipEventQuery(s.done);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
  return aa_fail(-2, "[aa_dump_snapshot_ready]: HIP error %s", hipGetErrorString(e));
}

int aa_dump_snapshot_wait(aa_grid *g, int slot)
{
  SNAP_SLOT("aa_dump_snapshot_wait");
  if (!s.held) return aa_fail(-1, "[aa_dump_snapshot_wait]: slot %d holds no snapshot", slot);
  HIPCHK(hipEventSynchronize(s.done));
  return 0;
}

const float *aa_dump_snapshot_section(aa_grid *g, int slot, int section, long long *nfloats)
{
  if (!g || !nfloats) { aa_fail(-1, "[aa_dump_snapshot_section]: null argument"); return nullptr; }
  if (slot < 0 || slot >= AA_DUMP_SLOTS) { aa_fail(-1, "[aa_dump_snapshot_section]: slot %d of %d", slot, AA_DUMP_SLOTS); return nullptr; }
  const aa_grid::DumpSlot &s = g->snap[slot];
  if (!s.held) { aa_fail(-1, "[aa_dump_snapshot_section]: slot %d holds no snapshot", slot); return nullptr; }
  if (section < 0 || section >= dump_nsections(g, s.fmt)) {
    aa_fail(-1, "[aa_dump_snapshot_section]: section %d of %d", section, dump_nsections(g, s.fmt)); return nullptr;
  }
  if (hipEventQuery(s.done) != hipSuccess) {
    (void)hipGetLastError();
    aa_fail(-1, "[aa_dump_snapshot_section]: the payload of slot %d is not on the host yet (aa_dump_snapshot_ready / _wait)", slot);
    return nullptr;
  }
  const unsigned long long n = (unsigned long long)g->p.Nx[0]*g->p.Nx[1]*g->p.Nx[2];
  *nfloats = aa_dump_section_floats(g, s.fmt, section);
  return s.host + dump_snapshot_offset(s.fmt == AA_DUMP_VTK, n, section);
}

int aa_dump_snapshot_release(aa_grid *g, int slot)
{
  SNAP_SLOT("aa_dump_snapshot_release");
  if (!s.held) return 0;
  HIPCHK(hipEventSynchronize(s.done));
  s.held = false;
  return 0;
}

}  // extern "C"
