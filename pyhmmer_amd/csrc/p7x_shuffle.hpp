// p7x_shuffle.hpp -- decoy sequences: a packed block shuffled sequence by sequence (p7x_shuffle.cpp: entry points, plan and
// host twin; p7x_shuffle.hip: the kernels; p7x_shufflewalk.hpp: the procedure both run).  Definitions: DESIGN.md 3.19.
#pragma once
#include "p7x_internal.hpp"
#include <cstdint>
#include <vector>

namespace p7x {

constexpr int kShufThreads = 256;                 // lanes of a workgroup: the sequences a run holds at most
constexpr int kShufSlabDefault = 64 * 1024;       // LDS bytes of a run's span (two resident workgroups per CU); option "shuffle_slab"
constexpr int kShufSlabMin = 64, kShufSlabMax = 160 * 1024 - 64;
constexpr int kShufLdsPad = 16;                   // beyond a region: the span is staged from the aligned dword at or before its first byte

struct ShuffleView { const uint8_t *dsq; const int64_t *offsets; const int32_t *lengths; int64_t n; int64_t nbytes; };

// The work of one call.  A run is a range of consecutive sequences, at most kShufThreads of them, whose span of the packed
// array -- the sentinel before the first one to the sentinel after the last one -- is at most <region> bytes; a sequence
// whose own span is longer is in no run and takes the long path.  region = slab, or slab / 2 in mode "di", whose
// successor lists take the other half.
struct ShufflePlan {
  int32_t slab = 0, region = 0;
  std::vector<int64_t> run_first;
  std::vector<int32_t> run_count;
  std::vector<int64_t> long_idx;
};
void shuffle_plan(const int64_t *offsets, const int32_t *lengths, int64_t n, int mode, ShufflePlan &plan);

// stats[5]: nanoseconds of the kernels, of the upload, runs, long sequences, 1 when shuffled on the device
enum { SHUF_STAT_KERNEL_NS = 0, SHUF_STAT_UPLOAD_NS, SHUF_STAT_RUNS, SHUF_STAT_LONG, SHUF_STAT_ON_DEVICE, SHUF_NSTATS };

int shuffle_block_device(int device, const ShuffleView &in, const ShufflePlan &plan, int mode, int32_t window, uint32_t seed, uint8_t *out_dsq,
                         int64_t *stats);

} // namespace p7x
