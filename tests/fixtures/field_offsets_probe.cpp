/* field_offsets_fit of csrc/field_offsets.h -- the guard aa_create puts in front of the marching kernels' 32-bit zone offsets --
 * compiled with the host compiler (tests/test_field_offsets_host.py). */
#include "field_offsets.h"

extern "C" int probe_field_offsets_fit(long long nc, long long sJ, long long sK) { return field_offsets_fit(nc, sJ, sK) ? 1 : 0; }
