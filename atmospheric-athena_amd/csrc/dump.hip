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
    const long m = (long)(k + (unsigned)g.ks)*g.sK + (long)(j + AA_NGHOST_)*g.sJ + (long)(i + AA_NGHOST_);
    const unsigned b = __float_as_uint(dump_value(g, VEC ? 1 + (int)c : var, prim, m));
    w[q] = swap ? __builtin_bswap32(b) : b;
  }
  if (o0 + 3u < nwords) *(uint4*)(dst + o0) = make_uint4(w[0], w[1], w[2], w[3]);
  else for (unsigned q = 0; o0 + q < nwords; q++) ((unsigned*)dst)[o0 + q] = w[q];
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
  const size_t room = (size_t)(g->two_d ? 20 : 36)*(size_t)g->d.nc;   // LR is 36*nc doubles = 72*nc floats: two slots of 36*nc (a 2-D Grid: 20*nc)
  const size_t row = (size_t)3*(size_t)g->d.Nx1;
  if (cap > room) cap = room;
  if (cap < row) cap = row;
  return (cap + 3) & ~(size_t)3;
}

int dump_prepare(aa_grid *g)
{
  if (g->dump_host) return 0;
  const size_t cap = dump_capacity(g);
  HIPCHK(hipHostMalloc((void**)&g->dump_host, 2*cap*sizeof(float)));
  g->dump_cap = cap;
  HIPCHK(hipStreamCreateWithFlags(&g->dump_st, hipStreamNonBlocking));
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

}  // extern "C"
