// p7x_ens_plan.hpp -- where ens_walk_kernel (p7x_ensemble.hip) keeps each piece of a region's working set, written once
// for the kernel, for the host that sizes the launch's LDS and for the test seam p7x_debug_ens_walk_plan.
//
// Every placement selects another code path of the walk, so the tests run one region under every placement the arithmetic
// below can produce (tests/test_host_ens_walk_plan.py holds the arithmetic, tests/test_gpu_ens_walk_placement.py the kernel).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "p7x_choice.hpp"

namespace p7x {

enum { ENS_N2_REGS = 0, ENS_N2_LDS = 1, ENS_N2_GLOBAL = 2 };      // home of the per-residue null2 accumulators
constexpr int ENS_N2_PER_LANE = 8;                                // lane l keeps residues l + 1 + 64 j, j < 8, in registers
constexpr int ENS_CACHE_MIN_BYTES = 4096;                         // the record caches' minimum stays free of everything else

// Sections in the order they lie in LDS; a section that stays in memory has no offset (-1) and no bytes.
enum { ENS_SEC_CNT, ENS_SEC_N2V, ENS_SEC_ACCZ, ENS_SEC_MDTAG, ENS_SEC_ROWS, ENS_SEC_NORM, ENS_SEC_SQ, ENS_SEC_N2, ENS_SEC_RFT,
       ENS_SEC_MD, ENS_SEC_MCACHE, ENS_SEC_IDCACHE, ENS_NSEC };

struct EnsWalkPlan {
  bool rows_in_lds;        // the rows' records C / J / B (16 bytes each) and select_e's factor 1 / xE(i)
  bool sq_in_lds;          // the region's residues
  int n2_home;             // ENS_N2_*
  bool rft_in_lds;         // the profile's residue-minor match odds
  bool md_in_lds;          // eight Forward rows (M and D cells) for select_e
  int mbits, idbits;       // index bits of the match-cell cache and of the insert / delete cache (16-byte entries)
  bool by_row;             // every row has its own four match entries (else: hashed by cell number)
  bool cache_ok;           // cell numbers fit the caches' 27-bit tags
  int32_t off[ENS_NSEC];   // byte offset of each section, -1: not in LDS
  uint32_t bytes[ENS_NSEC];
  uint32_t used_before_caches, used_after_caches;
};

// A region of Lr residues of a model of M nodes in a launch of lds_bytes: each piece takes what fits below
// lds_bytes - ENS_CACHE_MIN_BYTES, in the order of the sections; the caches take powers of two of what is left, the match
// cells' about three quarters of it (at most 4096 entries), the insert / delete cells' the rest (at most 1024).
P7X_HD EnsWalkPlan ens_walk_plan(int M, int Lr, int lds_bytes)
{
  EnsWalkPlan p;
  for (int s = 0; s < ENS_NSEC; ++s) { p.off[s] = -1; p.bytes[s] = 0u; }
  const int Mrow = M + 1;
  const size_t ncnt = (size_t) ((M + 2 + 31) & ~31);
  p.off[ENS_SEC_CNT] = 0;                               p.bytes[ENS_SEC_CNT] = (uint32_t) (ncnt * 4);        // [M + 2]
  p.off[ENS_SEC_N2V] = (int32_t) (ncnt * 4);            p.bytes[ENS_SEC_N2V] = 32u * 4u;                     // [32]
  p.off[ENS_SEC_ACCZ] = (int32_t) ((ncnt + 32) * 4);    p.bytes[ENS_SEC_ACCZ] = 128u * 4u;                   // [4][32]
  p.off[ENS_SEC_MDTAG] = (int32_t) ((ncnt + 160) * 4);  p.bytes[ENS_SEC_MDTAG] = 8u * 4u;                    // [8]
  size_t used = (ncnt + 32 + 128 + 8) * 4;
  const size_t cap = (size_t) lds_bytes - ENS_CACHE_MIN_BYTES;
  p.rows_in_lds = used + (size_t) (Lr + 1) * 20 + 16 <= cap;
  if (p.rows_in_lds) {
    p.off[ENS_SEC_ROWS] = (int32_t) used;                             p.bytes[ENS_SEC_ROWS] = (uint32_t) (Lr + 1) * 16u;
    p.off[ENS_SEC_NORM] = (int32_t) (used + (size_t) (Lr + 1) * 16);  p.bytes[ENS_SEC_NORM] = (uint32_t) (Lr + 1) * 4u;
    used += ((size_t) (Lr + 1) * 20 + 15) & ~(size_t) 15;
  }
  p.sq_in_lds = used + (size_t) Lr + 16 <= cap;
  if (p.sq_in_lds) { p.off[ENS_SEC_SQ] = (int32_t) used; p.bytes[ENS_SEC_SQ] = (uint32_t) Lr; used += ((size_t) Lr + 15) & ~(size_t) 15; }
  const bool n2_in_regs = Lr <= 64 * ENS_N2_PER_LANE && p.sq_in_lds;
  const bool n2_in_lds = !n2_in_regs && used + (size_t) (Lr + 1) * 4 + 16 <= cap;
  p.n2_home = n2_in_regs ? ENS_N2_REGS : (n2_in_lds ? ENS_N2_LDS : ENS_N2_GLOBAL);
  if (n2_in_lds) { p.off[ENS_SEC_N2] = (int32_t) used; p.bytes[ENS_SEC_N2] = (uint32_t) (Lr + 1) * 4u; used += (size_t) (((Lr + 1) + 3) & ~3) * 4; }
  p.rft_in_lds = used + (size_t) (M + 1) * 128 <= cap;
  if (p.rft_in_lds) { p.off[ENS_SEC_RFT] = (int32_t) used; p.bytes[ENS_SEC_RFT] = (uint32_t) (M + 1) * 128u; used += (size_t) (M + 1) * 128; }
  p.md_in_lds = used + (size_t) 8 * Mrow * 8 + 16 <= cap;
  if (p.md_in_lds) { p.off[ENS_SEC_MD] = (int32_t) used; p.bytes[ENS_SEC_MD] = (uint32_t) Mrow * 64u; used += ((size_t) 8 * Mrow * 8 + 15) & ~(size_t) 15; }
  used = (used + 15) & ~(size_t) 15;
  p.used_before_caches = (uint32_t) used;
  const size_t left = (size_t) lds_bytes - used;
  int mbits = 7, idbits = 6;
  while (mbits < 12 && ((size_t) 32 << mbits) <= left - left / 4) ++mbits;
  while (idbits < 10 && ((size_t) 16 << mbits) + ((size_t) 32 << idbits) <= left) ++idbits;
  p.mbits = mbits; p.idbits = idbits;
  p.off[ENS_SEC_MCACHE] = (int32_t) used;                                p.bytes[ENS_SEC_MCACHE] = 16u << mbits;
  p.off[ENS_SEC_IDCACHE] = (int32_t) (used + ((size_t) 16 << mbits));    p.bytes[ENS_SEC_IDCACHE] = 16u << idbits;    // follows the match cache
  p.used_after_caches = (uint32_t) (used + ((size_t) 16 << mbits) + ((size_t) 16 << idbits));
  p.cache_ok = (size_t) (Lr + 1) * (size_t) Mrow < ((size_t) 1 << 27) - 2;
  p.by_row = Lr < (1 << (mbits - 2));
  return p;
}

// LDS of one walk launch: node counts and the null2 scratch always; then, as far as <most_bytes> go, the largest region's row
// records, residues and accumulators, the longest model's odds table and eight of its Forward rows (each region takes what
// fits, in that order), and the record caches of the core walk in the rest (48 KiB when there is room, never less than 4 KiB).
struct EnsLdsBudget { size_t least, want, lds_bytes; };
constexpr size_t ENS_LDS_DEFAULT_MOST = (size_t) 32 * 1024;
inline EnsLdsBudget ens_walk_lds_budget(int maxM, int maxLr, size_t most_bytes)
{
  EnsLdsBudget b;
  b.least = (size_t) (((maxM + 2 + 31) & ~31) + 32 + 128 + 8) * 4 + 64 + ENS_CACHE_MIN_BYTES;
  b.want = b.least + (size_t) (maxLr + 1) * 25 + 128 + (size_t) (maxM + 1) * (128 + 64) + 44 * 1024;
  b.lds_bytes = std::max(b.least, std::min(b.want, most_bytes));
  return b;
}

} // namespace p7x
