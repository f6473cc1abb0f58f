// p7x_oaguard.hpp -- device helpers of the optimal-accuracy step of the envelope / alignment kernel (p7x_envkernel.hpp):
// gates of the OA recursion, the posterior digit of the alignment display and the
// near-tie guards that tell the host which choices its own summation order has to decide.
#pragma once
#include "p7x_wave.hpp"

namespace p7x {

namespace {

constexpr float kNegInf = -__builtin_inff();

// p7T_* state codes (p7_trace.pxd), as the host uses them
enum { tM = 1, tD = 2, tI = 3, tS = 4, tN = 5, tB = 6, tE = 7, tC = 8, tT = 9, tJ = 10 };

__device__ __forceinline__ float gate(float t, float v) { return t > 0.0f ? v : 0.0f; }          // and(cmpgt(t, 0), v)
__device__ __forceinline__ float block(float t, float v) { return t > 0.0f ? v : kNegInf; }      // traceback: t == 0 ? -inf : v
__device__ __forceinline__ float vmax(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float rflf(float v) { return __builtin_bit_cast(float, rfl(__builtin_bit_cast(int, v))); }

__device__ __forceinline__ void phase_fence()
{ // Rows written by this wavefront are read back by it (possibly by other lanes, and the workspace is re-used for the
  // next envelope).  Producer and consumer are the same wavefront, so work-group scope is all that is needed: the
  // stores have left the wavefront (vmcnt(0)) and the CU's vector cache is coherent for its own stores.  Agent scope
  // would write back and invalidate the XCD's whole L2 (buffer_wbl2 / buffer_inv sc1) four times per envelope and
  // wavefront -- taking the lines of every other wavefront and of the filter kernels running beside this one with it.
  // (This relies on the wavefront's producer and consumer lanes sharing one CU's vector cache: the kernels that use it must
  // not be built for tgsplit mode, where a work-group may straddle CUs.)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

} // namespace

// posterior probability -> the digit of the alignment's posterior line, exactly as the host prints it
// (p7_alidisplay: (p + 0.05 >= 1.0) ? '*' : '0' + (int) ((p + 0.05) * 10.0), in double): 0..9, 10 = '*'
__device__ __forceinline__ unsigned pp_code(float p)
{
  const double v = (double) p + 0.05;
  return v >= 1.0 ? 10u : (unsigned) (int) (v * 10.0);
}
// Near-tie guard (status bit 6).  The optimal-accuracy recursion sums posteriors that differ from the host twin's by a
// few units in the last place (another summation order in Forward / Backward), so a traceback choice between two
// candidates that lie within a few ulps of each other -- or a posterior within that distance of the next printed digit
// -- can fall the other way than in the reference's order of operations.  Every such choice ON THE TRACE flags the
// envelope, and the host stage repeats flagged envelopes with the host twin (domaindef_finish_deferred), which performs
// the reference's operations in the reference's order.  guard: relative half-width (cfg.oa_guard); 0 switches it off.
__device__ __forceinline__ float guard_band(float v, float guard) { return __builtin_fabsf(v) * guard + guard; }
__device__ __forceinline__ int near_tie(float x, float y, float guard)
{ // the band is the winner's: one candidate at -inf (a closed transition, the first row) is an infinite distance away;
  // both at -inf: the difference is NaN and the test is false (such a cell is unreachable anyway)
  return (__builtin_fabsf(x - y) <= guard_band(vmax(x, y), guard)) ? 1 : 0;
}
__device__ __forceinline__ int pp_near(float p, float guard)
{
  // float is enough here: the band is an order of magnitude wider than the rounding of this expression
  const float v = (p + 0.05f) * 10.0f;
  return (__builtin_fabsf(v - __builtin_rintf(v)) < 4.0f * guard && v > 0.75f) ? 1 : 0;
}
// The same two tests as they run inside the decoding row (every cell of every row): the winner <hi> is known there and
// optimal-accuracy values are sums of probabilities (>= 0, or -inf where nothing leads), so  hi - lo <= hi g + g  is
// lo >= fma(hi, 1 - g, -g): one fused multiply-add and one comparison.  (An unreachable cell, hi = -inf, tests true; no
// trace passes through one.)
__device__ __forceinline__ int near_below(float hi, float lo, float g1, float g) { return lo >= __builtin_fmaf(hi, g1, -g) ? 1 : 0; }
// ... and the printed digit with its distance from the next one, in float under the guard: v = 10 p + 0.5 is off by an ulp
// or two of what the host computes in double, the band of 4 guards on either side of a digit boundary is ten times wider
__device__ __forceinline__ unsigned pp_code_guarded(float p, float band, int &near)
{
  const float v = __builtin_fmaf(p, 10.0f, 0.5f);
  const float f = v - __builtin_floorf(v);
  near |= (__builtin_fabsf(f - 0.5f) > band) ? 1 : 0;             // band = 0.5 - 4 guard
  const int d = (int) v;
  return (unsigned) (d > 10 ? 10 : d);
}
// and back to a float that prints as that digit (the host stage formats the line from floats)
__device__ __forceinline__ float pp_from_code(unsigned code) { return code >= 10u ? 1.0f : (float) (((double) code + 0.5) / 10.0 - 0.05); }

} // namespace p7x
