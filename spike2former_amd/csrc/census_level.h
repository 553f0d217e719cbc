// The integer spike level of one element (include/s2f.h "operand census"), shared by the kernels that count levels: the operand
// census (opcensus.hip) and the firing maps (firingmap.hip).  ONE definition, so that a map and a census of the same tensor agree.
#pragma once
#include "s2f_common.h"

struct S2fLevel {
  unsigned level;          // x * D where that is an integer in [0, 65535], else 0
  bool nonzero;            // x != 0 (-0.0 counts as zero)
  bool on;                 // on the level grid
  bool finite;
};

// One element, given as the bits of its fp32 value (a bf16 element: its 16 bits in the high half, which IS its fp32 value).
// The product x * D is ONE fp32 multiply, rounded to nearest (exact for the powers of two every shipped config uses).  A subnormal x
// is off the grid by its bits: x * D lies strictly between 0 and 1 there, and the verdict must not hang on the denormal mode.
__device__ __forceinline__ S2fLevel s2f_census_level(unsigned bits, float Df) {
  const unsigned mag = bits & 0x7fffffffu;
  const float p = __uint_as_float(bits) * Df;
  const bool finite = mag < 0x7f800000u;
  const bool subnormal = mag != 0u && mag < 0x00800000u;
  const bool on = finite && !subnormal && p >= 0.0f && p <= 65535.0f && p == truncf(p);
  return S2fLevel{on ? (unsigned)p : 0u, mag != 0u, on, finite};
}
