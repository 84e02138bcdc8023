// field_offsets.h -- whether the marching 3-D kernels can address a Grid.  They reach a zone of a field as scalar base + ONE 32-bit
// unsigned byte offset + immediate (hydro_kernels.hip, field accessors): the offset is the zone's place inside a field, at most
// nc*8 bytes, the +-1 zone neighbours are in the immediate, and the row / plane neighbours (sJ, sK, 2 sK) are added to the base.
// A Grid fits if the farthest byte such an access can mean, counted from the field's first, is below 2^32:
//   nc*8 + max(2 sK, sJ)*8 + 8 < 2^32
// (672 B/zone: a Grid that does not fit is a Grid of 360 GB).  aa_create refuses the others; there is one code path.
// Plain C++, no HIP: tests/fixtures/field_offsets_probe.cpp compiles it with the host compiler.
#pragma once

static inline bool field_offsets_fit(long long nc, long long sJ, long long sK)
{
  const long long big = 1LL << 40;                                // (far beyond the limit, far below where the products overflow)
  if (nc < 0 || sJ < 0 || sK < 0 || nc >= big || sJ >= big || sK >= big) return false;
  const long long far = (2*sK > sJ) ? 2*sK : sJ;
  return nc*8 + far*8 + 8 < (1LL << 32);
}
