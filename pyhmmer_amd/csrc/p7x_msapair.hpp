// p7x_msapair.hpp -- pairwise identity of the rows of an alignment: what the host code (p7x_msapair.cpp) and the kernels
// (p7x_msapair.hip) share.
//
// The alignment is kept as two byte images of N x Lp (Lp = L rounded up to four, as in p7x_msabuild.hpp).  A canonical
// residue keeps its code in both; every other cell (gap, degenerate, '*', '~', pad) is kPairOtherA in image A and
// kPairOtherB in image B.  A byte of row i in A then equals the byte of row j in B exactly when both rows hold the same
// canonical residue there, so idents_ij = Lp - (bytes that differ): no mask in the inner loop.  Every byte of either
// image is below 0x80 (codes are below 32), which is what makes the carry-free count of pair_dword_diff exact.
// Everything is an integer: the decision "linked" is idents >= need[min(len_i, len_j)], with the table built once on the
// host, so the kernels, whatever their tile and grid, and the host twin give the same bits.
#pragma once
#include "p7x_internal.hpp"
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define P7X_PAIR_HD __host__ __device__ inline
#else
#define P7X_PAIR_HD inline
#endif

namespace p7x {

constexpr uint8_t  kPairOtherA   = 0x40;          // a cell that is no canonical residue, in image A ...
constexpr uint8_t  kPairOtherB   = 0x20;          // ... and in image B: they differ from each other and from every code
constexpr uint32_t kPairFillA    = 0x40404040u;   // what the kernel stages beyond the last dword or row
constexpr uint32_t kPairFillB    = 0x20202020u;
constexpr uint32_t kPairNever    = 0xffffffffu;   // need[l] when no count of identities reaches the threshold
constexpr int      kPairTileMax  = 64;            // rows per tile side (debug option "pairid_tile" lowers it)
constexpr int      kPairChunk    = 32;            // dwords (128 columns) of every row that a block stages at a time
constexpr int      kPairStride   = kPairChunk + 4;   // LDS row stride in dwords (see p7x_msapair.hip)
constexpr int      kPairBlockTiles = 16;          // the filter's candidate block, in tiles
constexpr int64_t  kPairMaxRows  = (int64_t) 1 << 20;   // the filter: build_msa's limits
constexpr int      kPairMaxCols  = 65535;
constexpr int64_t  kPairMaxIdentRows = 4096;      // the raw counts: an N x N matrix comes back
constexpr int64_t  kPairMaxLinkRows  = (int64_t) 1 << 18;   // clusters: N^2 / 16 bytes of link bits come back (4 GiB here)

P7X_PAIR_HD bool pair_is_canonical(unsigned a, unsigned K) { return a < K; }
P7X_PAIR_HD uint8_t pair_code_a(unsigned a, unsigned K) { return pair_is_canonical(a, K) ? (uint8_t) a : kPairOtherA; }
P7X_PAIR_HD uint8_t pair_code_b(unsigned a, unsigned K) { return pair_is_canonical(a, K) ? (uint8_t) a : kPairOtherB; }

// bytes of two dwords that differ, both with every byte below 0x80: a byte of the xor is 1..0x7f where they differ, and
// 0x7f more sets its top bit without a carry into the next byte
// (returned added to <acc>).  On the device three instructions a dword: xor-and-add in one, and, a population count that
// adds; the compiler picks neither fused form by itself (it sums the counts in a tree of three-operand adds), so the two
// are written out -- plain register-to-register vector instructions.
P7X_PAIR_HD uint32_t pair_dword_diff(uint32_t acc, uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t t, r;
  asm("v_xad_u32 %0, %1, %2, %3" : "=v"(t) : "v"(a), "v"(b), "s"(0x7f7f7f7fu));
  t &= 0x80808080u;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(t), "v"(acc));
  return r;
#else
  const uint32_t m = ((a ^ b) + 0x7f7f7f7fu) & 0x80808080u;
  return acc + (uint32_t) __builtin_popcount(m);
#endif
}
P7X_PAIR_HD bool pair_linked(uint32_t idents, uint32_t len_i, uint32_t len_j, const uint32_t *need)
{
  return idents >= need[len_i < len_j ? len_i : len_j];
}

// need[l], l = 0..L: the smallest k with (double) k / l >= t; need[0] = 0 if 0.0 >= t.  kPairNever where there is none.
inline void pair_need_table(double t, int L, std::vector<uint32_t> &need)
{
  need.assign((size_t) L + 1, kPairNever);
  need[0] = 0.0 >= t ? 0u : kPairNever;
  for (int l = 1; l <= L; ++l) {
    if (!(t <= 1.0)) continue;                       // k / l <= 1 (a NaN links nothing)
    int64_t k = t <= 0.0 ? 0 : (int64_t) (t * (double) l);
    while (k > 0 && (double) (k - 1) / (double) l >= t) --k;
    while (k <= l && !((double) k / (double) l >= t)) ++k;
    if (k <= l) need[l] = (uint32_t) k;
  }
}

// The alignment as the drivers hold it.
struct PairImages {
  int64_t N = 0; int L = 0, Lp = 0;
  std::vector<uint8_t> a, b;          // [N][Lp]
  std::vector<uint32_t> len;          // [N] canonical residues of every row
};

// What one call computes over row sets of the images, on the device or by the twin: rows_a[na] against rows_b[nb] (row
// indices; nullptr: the rows base_a .. base_a + na - 1).  lower: only pairs of tiles that hold a pair with
// (index in b) <= (index in a) are looked at -- the tile grid starts at row 0 of either set, so what a tile is depends on
// <tile> and what is written above the diagonal does too: callers read j <= i only.
struct PairJob {
  const int32_t *rows_a = nullptr, *rows_b = nullptr;
  int64_t base_a = 0, base_b = 0, na = 0, nb = 0;
  bool lower = false;
  uint32_t *idents = nullptr;         // [na][nb] or nullptr
  uint64_t *bits = nullptr;           // [na][(nb + 63) / 64] link bits, bit j & 63 of word j / 64, or nullptr; zeroed by the callee
  uint8_t *any = nullptr;             // [na] linked to at least one row of b, or nullptr
};

struct PairStats { int64_t pairs = 0; double kernel_ns = 0, upload_ns = 0; int on_device = 0; };

struct PairDevice;
int  pair_device_open(int device, const PairImages &img, const std::vector<uint32_t> &need, int tile, PairStats &st, PairDevice **out);
int  pair_device_run(PairDevice *d, const PairJob &job, PairStats &st);
// the clusters' link bits, band after band of rows against all the rows before them, through two pinned buffers:
// visit(i0, i1, words_per_row, bits) sees bits[(i - i0) * words_per_row + j / 64] for i0 <= i < i1, j <= i
typedef void (*PairBandVisitor)(void *user, int64_t i0, int64_t i1, int64_t words_per_row, const uint64_t *bits);
int  pair_device_bands(PairDevice *d, int64_t N, PairBandVisitor visit, void *user, PairStats &st);
void pair_device_close(PairDevice *d);

} // namespace p7x
