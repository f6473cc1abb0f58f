// p7x_emit.hpp -- what the emitters share: the cumulative tables of a core model (built by p7x_emit.cpp), the block of
// sequences that HMM.emit_block returns, and the sizes of the device emitter's workspace (p7x_emit.hip).
#pragma once
#include "p7x_internal.hpp"
#include "p7x_emitwalk.hpp"
#include <vector>

struct p7x_emit_model {
  int M = 0, K = 0, abc_type = 0;
  std::vector<double> tab;            // [(M + 1) * emit_stride(K)], see p7x_emitwalk.hpp
  std::vector<double> occ;            // [M + 1] match occupancy (the local entry distribution of Profile.emit_sequence)
  double expected_length = 0.0;       // of one pass through the core model, the empty path included
};

struct p7x_emitted {               // packed as easel.PackedBlock: 255 x1..xL 255 x1..xL 255
  int64_t n = 0, nres = 0;
  int32_t cap = 0;                    // slot capacity of the first pass
  int64_t nredrawn = 0;               // sequences longer than that: drawn again into an exact slot
  int on_device = 0;
  double kernel_us = 0.0;             // device time of the emit kernel's launches (both passes), from events
  bool traces = false;
  std::vector<uint8_t> dsq;           // [nres + n + 1]
  std::vector<int64_t> offsets;       // [n]
  std::vector<int32_t> lengths, attempts;   // [n]
  std::vector<int8_t> st;             // traces: [nres + n + 1] state of every residue (p7T_M 1, p7T_I 3), 0 at the sentinels
  std::vector<int32_t> node;          // traces: [nres + n + 1] node of every residue
};

namespace p7x {

// slot capacity of the first pass: option "emit_cap" when set, else twice the expected length, a multiple of four
int32_t emit_default_cap(const p7x_emit_model &em);
// bytes of device memory the first pass takes for n sequences; P7X_EMEM when they exceed <budget> (or do not fit 63 bits)
int emit_workspace_bytes(int64_t n, int64_t cap, bool traces, int64_t budget, int64_t *bytes);
int emit_status_error(int status, int64_t seq);
int emit_block_host(const p7x_emit_model &em, int64_t n, uint64_t seed, bool traces, int threads, p7x_emitted &out);

} // namespace p7x
