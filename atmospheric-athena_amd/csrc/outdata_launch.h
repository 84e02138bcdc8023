// outdata_launch.h -- launch interface of outdata.hip: the payload of a single-variable output (OutData1 / OutData2 / OutData3 of
// output.c:629-1107 with the expr_* functions of :1109-1233) from a resident Grid.  Kept apart from grid.h like the other kernel
// files' launch headers.
#pragma once
#include "grid.h"

struct aa_grid;

namespace aa {

// One output.  Element o = (c*n[1] + b)*n[0] + a of the payload belongs to the zones (i, j, k) with i = a where x1 is kept
// (n[0] = Nx1) and i = lo[0] .. hi[0] where it is reduced (n[0] = 1), likewise j / b and k / c; all indices count ACTIVE zones from 0.
// sum: some direction is reduced -- the element starts at 0.0, takes its zones in ascending k, then j, then i, and is multiplied by
// `factor`; else it IS the expression of its one zone (no 0.0 + x: the sign of a zero stays).
struct OutDesc {
  int ex;                           // AA_OUT_* of include/athena_amd.h
  int red[3], lo[3], hi[3];
  unsigned n[3];
  int sum;
  Real factor;                      // 1.0/count/count, the reference's quotients in its order (k, j, i over the reduced directions)
};

#define AA_OUT_PART_BLOCKS 1024     /* most blocks of a k_out_payload launch = partial records of its minimum / maximum */

// `cnt` elements of the payload from element p0 on, as doubles to dst; the piece's minimum and maximum with the payload index of
// each go to part[0 .. blocks) as 4 doubles {min, index, max, index}.  -> blocks
int  launch_out_payload(const DevGrid &g, const OutDesc &q, unsigned long long p0, unsigned cnt, Real *dst, Real *part, hipStream_t st);
// part[0 .. nblocks) and, unless `first`, the running record mm -> mm (4 doubles as above): minmax1/2/3 of utils.c
void launch_out_fold(const Real *part, int nblocks, Real *mm, bool first, hipStream_t st);
// `cnt` bytes of the pgm image (output_pgm.c:94-122) from byte p0 on: scaled (rows from the last to the first, gray = (int)(sfact*
// (data - dmin)) clamped to 0 .. 255), or all 0 where max_min is not positive (`scaled` false)
void launch_out_gray(const DevGrid &g, const OutDesc &q, Real dmin, Real sfact, bool scaled, unsigned long long p0, unsigned cnt,
                     unsigned char *dst, hipStream_t st);

}  // namespace aa

void outdata_release(aa_grid *g);   // the partial records and the page-locked minimum / maximum of a Grid that is going away
