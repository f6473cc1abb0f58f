// p7x_emitwalk.hpp -- one sampled path through the core model (upstream p7_CoreEmit), written once for the device kernel
// (p7x_emit.hip) and for its host twin (p7x_emit.cpp: p7x_emit_block_host).
//
// The random numbers are counter based (Philox-4x32-10, Salmon et al., SC'11): the key is the caller's seed, the counter
// is (sequence index, attempt, step), so sequence i is the same whatever the number of sequences, the grid or the
// processor.  Step s of a path takes ONE block of four words: words 0-1 make the deviate of the transition out of the
// state the path is in, words 2-3 the deviate of the residue the next state emits (unused when it is a delete state).
// A deviate is a 53-bit integer scaled to [0, 1) in double -- exact -- and every choice is "the first entry of a cumulative
// table (double, built on the host: p7x_emit.cpp) that the deviate is below": conversions and comparisons only, no
// arithmetic whose rounding could differ between the two processors.  Same function, same tables: the same path.
#pragma once
#include "p7x_choice.hpp"        // P7X_HD
#include <cstdint>

namespace p7x {

// ---- the tables: kEmitTrans + 2 K doubles per node k = 0 .. M
//   [0] MM  [1] MM + MI   (M_k, or B for k = 0: to M_k+1 below [0], to I_k below [1], else to D_k+1)
//   [2] IM                (I_k: to M_k+1 below it, else stays)
//   [3] DM                (D_k: to M_k+1 below it, else to D_k+1)
//   [4 .. 4 + K)          cumulative match emissions of node k
//   [4 + K .. 4 + 2 K)    cumulative insert emissions of node k
// every row over its own sum; the last entry of a row (for the transition rows the one that is not stored) is exactly 1.0
constexpr int kEmitTrans = 4;
P7X_HD int emit_stride(int K) { return kEmitTrans + 2 * K; }

constexpr int kEmitMaxLen = 100000;        // the pipeline's target length limit: a longer emission is an error, not cut
constexpr int kEmitMaxAttempts = 4096;     // attempts that emitted nothing before the model counts as one that cannot emit
enum { EMIT_OK = 0, EMIT_TOO_LONG = 1, EMIT_NEVER = 2 };
enum { EMIT_ST_M = 1, EMIT_ST_D = 2, EMIT_ST_I = 3 };       // p7T_M, p7T_D, p7T_I

struct Philox4 { uint32_t v[4]; };
P7X_HD Philox4 philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3)
{
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t) 0xD2511F53u * c0, p1 = (uint64_t) 0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t) (p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t) (p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t) p1; c3 = (uint32_t) p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  Philox4 o; o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}
// 53 bits of two words over 2^53
P7X_HD double emit_uniform(uint32_t hi, uint32_t lo)
{
  const uint64_t b = ((uint64_t) (hi >> 5) << 26) | (uint64_t) (lo >> 6);
  return (double) b * (1.0 / 9007199254740992.0);
}
// the first of n entries that u is below; the last one is 1.0, u is not
P7X_HD int emit_pick(const double *c, int n, double u)
{
  int x = 0;
  while (x < n - 1 && !(u < c[x])) ++x;
  return x;
}

// One sequence: attempts a0, a0 + 1, ... until one emits a residue.  sink.put(pos, residue, state, node) receives residue
// number pos (from 0) of the attempt that counts; an attempt that emits nothing has called it never.  Returns the status;
// *len = residues emitted (all of them, also those a sink with a bounded slot had to drop), *attempt = the attempt used.
template <class Sink>
P7X_HD int emit_walk(const double *tab, int M, int K, uint32_t key0, uint32_t key1, uint64_t seq, uint32_t a0, Sink &sink,
                     int32_t *len, uint32_t *attempt)
{
  const int S = emit_stride(K);
  const uint32_t s0 = (uint32_t) seq, s1 = (uint32_t) (seq >> 32);
  for (uint32_t a = a0; a - a0 < (uint32_t) kEmitMaxAttempts; ++a) {
    int k = 0, st = EMIT_ST_M, n = 0;      // B is M_0
    uint32_t step = 0;
    for (;;) {
      const Philox4 r = philox4x32_10(key0, key1, s0, s1, a, step++);
      const double u = emit_uniform(r.v[0], r.v[1]);
      const double *t = tab + (size_t) k * S;
      if (st == EMIT_ST_M)      { if (u < t[0]) { st = EMIT_ST_M; ++k; } else if (u < t[1]) st = EMIT_ST_I; else { st = EMIT_ST_D; ++k; } }
      else if (st == EMIT_ST_I) { if (u < t[2]) { st = EMIT_ST_M; ++k; } }
      else                      { ++k; if (u < t[3]) st = EMIT_ST_M; }
      if (k > M) break;                    // E
      if (st != EMIT_ST_D) {
        if (n >= kEmitMaxLen) { *len = n; *attempt = a; return EMIT_TOO_LONG; }
        const double *e = tab + (size_t) k * S + kEmitTrans + (st == EMIT_ST_I ? K : 0);
        const int x = emit_pick(e, K, emit_uniform(r.v[2], r.v[3]));
        sink.put(n, x, st, k);
        ++n;
      }
    }
    if (n > 0) { *len = n; *attempt = a; return EMIT_OK; }
  }
  *len = 0; *attempt = a0;
  return EMIT_NEVER;
}

} // namespace p7x
