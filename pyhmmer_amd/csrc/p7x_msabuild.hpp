// p7x_msabuild.hpp -- Builder.build_msa: what the host code (p7x_msabuild.cpp) and the kernels (p7x_msabuild.hip) share.
//
// The alignment is an N x Lp byte matrix of digital codes (Lp = L rounded up to four, the pad cells hold kMsaPad; the
// cells outside a fragment's span hold the missing-data code).  Everything that is summed over the rows is an integer:
// plain counts, or row weights in fixed point (unit 2^-40).  Integer sums do not depend on the order of the terms, so
// the kernels, whatever their grid, and the host twin give the same bits; the one conversion to double is host code that
// both share (p7x_msabuild.cpp).
#pragma once
#include "p7x_internal.hpp"
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define P7X_MSA_HD __host__ __device__ inline
#else
#define P7X_MSA_HD inline
#endif

namespace p7x {

constexpr int      kMsaSlots   = 32;            // counters per column: one per code (Kp <= 29)
constexpr int      kMsaCodes   = 29;            // codes that are counted: everything below the pad code
constexpr uint8_t  kMsaPad     = 31;
constexpr int      kMsaK       = 20;            // amino: residues 0..19, gap 20, degenerate 21..26, '*' 27, missing 28
constexpr uint8_t  kMsaMissing = 28;
constexpr int      kMsaShift   = 40;            // fixed point: a weight of 1 is 2^40
constexpr int      kMsaSplit   = 20;            // the I->I count of a step, (inserted residues - 1) x weight, in two sums (below)
constexpr int64_t  kMsaMaxRows = (int64_t) 1 << 20;
constexpr int      kMsaMaxCols = 65535;

P7X_MSA_HD bool msa_is_canonical(unsigned a) { return a < (unsigned) kMsaK; }
P7X_MSA_HD bool msa_is_residue(unsigned a) { return a < (unsigned) kMsaK || (a > (unsigned) kMsaK && a <= 26u); }
P7X_MSA_HD bool msa_is_gap(unsigned a) { return a == (unsigned) kMsaK; }

// ---- one row as a path through the consensus columns.  map[0] = -1, map[1..M] = the column of node k, map[M+1] = L.
// The raw state of node k: 0 a residue (match), 1 a gap (delete), 2 missing; nodes 0 and M + 1 stand for B and E, which a
// fragment does not pass through.
P7X_MSA_HD int msa_raw(const uint8_t *row, const int32_t *map, int M, int k, bool frag)
{
  if (k == 0 || k == M + 1) return frag ? 2 : 0;
  const unsigned a = row[map[k]];
  return msa_is_residue(a) ? 0 : (msa_is_gap(a) ? 1 : 2);
}
// the residues in the columns between nodes k and k + 1 (run k): how many, the first and the last
P7X_MSA_HD int msa_run(const uint8_t *row, const int32_t *map, int k, int *first, int *last)
{
  int n = 0;
  for (int c = map[k] + 1; c < map[k + 1]; ++c) {
    const unsigned a = row[c];
    if (msa_is_residue(a)) { if (n == 0 && first) *first = (int) a; if (last) *last = (int) a; ++n; }
  }
  return n;
}
// Plan 7 has neither D->I nor I->D.  A delete next to inserted residues takes one of them and becomes a match: the last
// one before it if there is one left, else the first one after it (left to right, so a delete further left chooses
// first).  Node j is a gap: does it take the last residue of run j - 1?  Only a run of exactly one residue behind another
// gap leaves that open, and then the answer is the left neighbour's own answer (it takes the residue after it exactly when
// it takes none before it).
P7X_MSA_HD bool msa_takes_before(const uint8_t *row, const int32_t *map, int M, int j, bool frag)
{
  for (;;) {
    const int n = msa_run(row, map, j - 1, nullptr, nullptr);
    if (n == 0) return false;
    if (n >= 2) return true;
    if (j - 1 < 1 || msa_raw(row, map, M, j - 1, frag) != 1) return true;
    --j;
  }
}

// What a row adds to node k (0..M): the step to node k + 1, and the residue node k takes from a neighbouring run.
// slot: the transition (0 MM, 2 MD, 5 DM, 6 DD) of a step without inserted residues, -1 otherwise; nins > 0: M->I, nins - 1
// times I->I, I->M.  Nothing (slot -1, nins 0) when either end is missing.  taken: the code node k takes, or -1.
struct MsaStep { int slot, nins, taken; };
// The weights sum to N 2^40 <= 2^60 and a run holds up to 65,533 residues, so the sum over the rows of (nins - 1) x weight
// does not fit 64 bits.  It is kept as two sums that do: the weight's bits above 2^20 times (nins - 1), in units of 2^-20
// (at most 2^40 x 2^16), and its low 20 bits times (nins - 1), in units of 2^-40 (at most 2^20 x 2^16 per row, 2^20 rows).
P7X_MSA_HD unsigned long long msa_ii_high(unsigned long long w, int nins) { return (w >> kMsaSplit) * (unsigned long long) (nins - 1); }
P7X_MSA_HD unsigned long long msa_ii_low(unsigned long long w, int nins) { return (w & ((1ull << kMsaSplit) - 1)) * (unsigned long long) (nins - 1); }
P7X_MSA_HD MsaStep msa_step(const uint8_t *row, const int32_t *map, int M, int k, bool frag)
{
  MsaStep s; s.slot = -1; s.nins = 0; s.taken = -1;
  const int rk = msa_raw(row, map, M, k, frag), rn = msa_raw(row, map, M, k + 1, frag);
  int first = -1, last = -1;
  const int n = msa_run(row, map, k, &first, &last);
  bool before_k = false, after_k = false, before_n = false, after_n = false;
  if (rk == 1) {
    before_k = msa_takes_before(row, map, M, k, frag);
    after_k = !before_k && n > 0;
    if (before_k) { int f2 = -1, l2 = -1; (void) msa_run(row, map, k - 1, &f2, &l2); s.taken = l2; }
    else if (after_k) s.taken = first;
  }
  if (rn == 1) {
    before_n = n - (after_k ? 1 : 0) > 0;
    if (!before_n) after_n = msa_run(row, map, k + 1, nullptr, nullptr) > 0;
  }
  if (rk == 2 || rn == 2) return s;
  const bool mk = rk == 0 || before_k || after_k, mn = rn == 0 || before_n || after_n;
  const int nins = n - (after_k ? 1 : 0) - (before_n ? 1 : 0);
  if (nins > 0) s.nins = nins;                 // both ends are matches then (see above)
  else s.slot = mk ? (mn ? 0 : 2) : (mn ? 5 : 6);
  return s;
}

} // namespace p7x

// Steps 3-5 of the build for one alignment, on the device or by the host twin.
struct p7x_msacounts {
  int64_t N = 0; int L = 0, Lp = 0, M = 0, on_device = 0, nwcols = 0, rows_per_block = 0;
  int64_t nfrag = 0;
  std::vector<uint8_t> ax;            // [N][Lp]
  std::vector<uint8_t> frag;          // [N]
  std::vector<uint32_t> colcnt;       // [Lp][32] rows holding each code
  std::vector<uint8_t> wmask;         // [Lp] weighting columns
  std::vector<uint64_t> termq;        // [Lp][20] 2^40 / (r_c n_c(a)) in the weighting columns
  std::vector<uint64_t> rowsum;       // [N] sum of the terms of a row's residues
  std::vector<int32_t> rowlen;        // [N] its residues in the weighting columns
  std::vector<uint64_t> wq;           // [N] weights, sum N 2^40
  std::vector<uint64_t> wcnt;         // [Lp][32] weighted counts of each code
  std::vector<int32_t> map;           // [M + 2]
  std::vector<uint64_t> taken;        // [M + 1][32] residues the nodes took from neighbouring runs
  std::vector<uint64_t> trq;          // [M + 1][8] transitions MM MI MD IM II DM DD; II holds msa_ii_low, slot 7 msa_ii_high
  std::vector<uint64_t> emq;          // [M + 1][32] weighted counts of each code at every node
  double kernel_us[4] = { 0, 0, 0, 0 };   // column counts, weights, weighted counts, transitions (device events; the twin: wall clock)
  double upload_us = 0;
};

namespace p7x {
// the passes over the alignment, on the device (p7x_msabuild.hip); their host twins are in p7x_msabuild.cpp
struct MsaDevice;
int  msa_device_open(int device, p7x_msacounts &c, MsaDevice **out);       // uploads c.ax and c.frag
int  msa_device_colcount(MsaDevice *d, p7x_msacounts &c);
int  msa_device_pbweight(MsaDevice *d, p7x_msacounts &c);                  // needs wmask, termq
int  msa_device_wcount(MsaDevice *d, p7x_msacounts &c);                    // needs wq
int  msa_device_transitions(MsaDevice *d, p7x_msacounts &c);               // needs map
void msa_device_close(MsaDevice *d);
}
