// p7x_shufflewalk.hpp -- one sequence shuffled in place, every mode, written once for the device kernels (p7x_shuffle.hip)
// and for their host twin (p7x_shuffle.cpp).  Definitions: DESIGN.md 3.19.
//
// Everything is integer arithmetic.  The random numbers are the counter-based stream of p7x_emitwalk.hpp (Philox-4x32-10;
// the generator is shared with the emitters, not copied): the key is (seed, 0), the counter is (sequence index low, high,
// attempt, step).  One block of four words v[0..3] gives two 64-bit draws, v[0] | v[1] << 32 and then v[2] | v[3] << 32;
// the draws of one (sequence, attempt) are taken in order, step 0, 1, ...  A number below n is the high half of the 128-bit
// product draw x n (Lemire's multiply-shift without the rejection step): its bias is below n / 2^64 per draw, below
// L / 2^64 for every draw of a sequence of L residues, and is documented, not corrected.
// Same function, same draws: the same bytes on either processor, whatever the other sequences, the grid or the slab.
#pragma once
#include "p7x_emitwalk.hpp"
#include <cstdint>

namespace p7x {

enum { SHUF_MONO = 0, SHUF_DI = 1, SHUF_WINDOW = 2, SHUF_REVERSE = 3, SHUF_NMODES = 4 };       // P7X_SHUFFLE_*
constexpr int kShufSyms = 32;                     // digital codes are below MAXKP = 29: the di counters are sized for 32 symbols
constexpr uint32_t kShufMaxAttempts = 1u << 16;   // di: rejected choices of last edges before the source's own are taken

// the high 64 bits of the 128-bit product draw x n, n below 2^32: the two partial products cannot overflow 64 bits
P7X_HD uint32_t shuf_mulhi(uint64_t draw, uint32_t n)
{
  const uint64_t lo = (draw & 0xffffffffu) * (uint64_t) n, hi = (draw >> 32) * (uint64_t) n;
  return (uint32_t) ((hi + (lo >> 32)) >> 32);
}

struct ShufRng {
  uint32_t key, s0, s1, attempt, step;
  uint64_t spare;
  bool has_spare;
  P7X_HD ShufRng(uint32_t seed, uint64_t seq) : key(seed), s0((uint32_t) seq), s1((uint32_t) (seq >> 32)), attempt(0), step(0), spare(0), has_spare(false) {}
  P7X_HD void restart(uint32_t a) { attempt = a; step = 0; has_spare = false; }
  P7X_HD uint64_t next()
  {
    if (has_spare) { has_spare = false; return spare; }
    const Philox4 r = philox4x32_10(key, 0u, s0, s1, attempt, step++);
    spare = (uint64_t) r.v[2] | ((uint64_t) r.v[3] << 32);
    has_spare = true;
    return (uint64_t) r.v[0] | ((uint64_t) r.v[1] << 32);
  }
  P7X_HD uint32_t below(uint32_t n) { return shuf_mulhi(next(), n); }
};

P7X_HD void shuf_swap(uint8_t *s, uint32_t i, uint32_t j) { const uint8_t a = s[i], b = s[j]; s[i] = b; s[j] = a; }

// Fisher-Yates from the last position down: position i takes the element at below(i + 1); n - 1 draws
P7X_HD void shuf_fisher_yates(uint8_t *s, uint32_t n, ShufRng &rng)
{
  for (uint32_t i = n; i-- > 1; ) shuf_swap(s, i, rng.below(i + 1));
}

// following the chosen last edges leads from every symbol of <need> to <f>
P7X_HD bool shuf_di_tree(const uint8_t *E, const uint32_t *pick, uint32_t need, int f)
{
  uint32_t good = 1u << f;
  for (int a = 0; a < kShufSyms; ++a) {
    if (!(need >> a & 1u) || (good >> a & 1u)) continue;
    uint32_t path = 0;
    int y = a;
    while (!(good >> y & 1u)) {
      if (path >> y & 1u) return false;        // a cycle that does not pass the last residue
      path |= 1u << y;
      y = E[pick[y]];
    }
    good |= path;
  }
  return true;
}

// Altschul & Erickson (1985): a uniform draw among the sequences with the first residue, the last residue and the count of
// every adjacent pair of s[0..L).  E[0..L-1): workspace, the successor lists.  Every code of s is below kShufSyms.
P7X_HD void shuf_di(uint8_t *s, int32_t L, uint8_t *E, ShufRng &rng)
{
  if (L < 3) return;
  uint32_t start[kShufSyms + 1], pick[kShufSyms];
  for (int a = 0; a <= kShufSyms; ++a) start[a] = 0;
  for (int32_t t = 0; t + 1 < L; ++t) ++start[s[t] + 1];
  for (int a = 0; a < kShufSyms; ++a) start[a + 1] += start[a];
  // the successor list of symbol a is E[start[a] .. start[a + 1]), in the order of the source (a counting sort of the edges)
  for (int a = 0; a < kShufSyms; ++a) pick[a] = start[a];
  for (int32_t t = 0; t + 1 < L; ++t) E[pick[s[t]]++] = s[t + 1];
  const int f = s[L - 1];
  uint32_t has = 0;
  for (int a = 0; a < kShufSyms; ++a) if (start[a + 1] > start[a]) has |= 1u << a;
  const uint32_t need = has & ~(1u << f);      // every one of them has a last edge to choose
  bool ok = false;
  for (uint32_t att = 0; att < kShufMaxAttempts && !ok; ++att) {
    rng.restart(att);
    for (int a = 0; a < kShufSyms; ++a) if (need >> a & 1u) pick[a] = start[a] + rng.below(start[a + 1] - start[a]);
    ok = shuf_di_tree(E, pick, need, f);
  }
  if (!ok) {      // never seen: the last edges of the source itself always lead to f
    rng.restart(kShufMaxAttempts);
    for (int a = 0; a < kShufSyms; ++a) if (need >> a & 1u) pick[a] = start[a + 1] - 1;
  }
  // the last edge goes to the end of its list, the rest is permuted (the draws go on in the stream of the accepted attempt)
  for (int a = 0; a < kShufSyms; ++a) {
    if (!(has >> a & 1u)) continue;
    uint32_t n = start[a + 1] - start[a];
    if (need >> a & 1u) { --n; shuf_swap(E, pick[a], start[a] + n); }
    shuf_fisher_yates(E + start[a], n, rng);
  }
  // the walk from the first residue takes the edges of every list in order; start[] is the cursor
  int cur = s[0];
  for (int32_t t = 1; t < L; ++t) { cur = E[start[cur]++]; s[t] = (uint8_t) cur; }
}

// sequence <seq> of a block, s[0..L), in place.  E: L bytes of workspace for SHUF_DI, unused otherwise.
P7X_HD void shuffle_sequence(int mode, uint8_t *s, int32_t L, uint8_t *E, int32_t window, uint32_t seed, uint64_t seq)
{
  if (L < 2) return;
  ShufRng rng(seed, seq);
  if (mode == SHUF_REVERSE) {
    for (int32_t i = 0; i < L / 2; ++i) shuf_swap(s, (uint32_t) i, (uint32_t) (L - 1 - i));
  } else if (mode == SHUF_MONO) {
    shuf_fisher_yates(s, (uint32_t) L, rng);
  } else if (mode == SHUF_WINDOW) {
    for (int64_t b = 0; b < L; b += window) shuf_fisher_yates(s + b, (uint32_t) (L - b < window ? L - b : window), rng);
  } else {
    shuf_di(s, L, E, rng);
  }
}

} // namespace p7x
