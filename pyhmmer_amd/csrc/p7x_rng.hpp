// p7x_rng.hpp -- Easel's two generators (esl_random.c), stated once: the calibration stream (p7x_builder.cpp), easel.Randomness
// (p7x_rng_seed / p7x_rng_draw) and the host emitters (p7x_emit.cpp) all draw from this one unit.
//   * the default one (esl_randomness_Create): MT19937 seeded by mt[z] = 69069 mt[z-1];
//   * the fast one (esl_randomness_CreateFast): the LCG the pipeline already draws with (fast_rng_state, lcg_next).
// A deviate is x / 2^32 either way.  Host only.
#pragma once
#include "p7x_host.hpp"
#include "p7x_choice.hpp"
#include <cstring>

namespace p7x {

struct EaselRng {
  int kind = P7X_RNG_FAST;
  uint32_t mt[624] = {}; int mti = 0;
  uint32_t x = 0;
  void fill()
  {
    static const uint32_t mag01[2] = { 0x0u, 0x9908b0dfu };
    uint32_t y; int z;
    for (z = 0; z < 227; ++z) { y = (mt[z] & 0x80000000u) | (mt[z + 1] & 0x7fffffffu); mt[z] = mt[z + 397] ^ (y >> 1) ^ mag01[y & 1u]; }
    for (; z < 623; ++z)      { y = (mt[z] & 0x80000000u) | (mt[z + 1] & 0x7fffffffu); mt[z] = mt[z - 227] ^ (y >> 1) ^ mag01[y & 1u]; }
    y = (mt[623] & 0x80000000u) | (mt[0] & 0x7fffffffu);
    mt[623] = mt[396] ^ (y >> 1) ^ mag01[y & 1u];
    mti = 0;
  }
  void init(int kind_, uint32_t seed)
  {
    kind = kind_;
    if (kind == P7X_RNG_MERSENNE) {
      mt[0] = seed;
      for (int z = 1; z < 624; ++z) mt[z] = 69069u * mt[z - 1];
      fill();
    } else {
      x = fast_rng_state(seed);               // the pipeline's generator: p7x_domaindef.cpp
    }
  }
  double next()
  {
    if (kind != P7X_RNG_MERSENNE) { x = lcg_next(x); return (double) x / 4294967296.0; }
    if (mti >= 624) fill();
    uint32_t y = mt[mti++];
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return (double) y / 4294967296.0;
  }
  // the generator's state as easel.Randomness keeps it between calls (P7X_RNG_STATE_WORDS words): mt[624], mti, x
  void load(int kind_, const uint32_t *s) { kind = kind_; std::memcpy(mt, s, sizeof(mt)); mti = (int) s[624]; x = s[625]; if (mti < 0 || mti > 624) mti = 624; }
  void save(uint32_t *s) const { std::memcpy(s, mt, sizeof(mt)); s[624] = (uint32_t) mti; s[625] = x; }
};

} // namespace p7x
