// p7x_shuffle.cpp -- decoy sequences: the entry points, the plan of the device's runs and the host twin of
// p7x_shuffle.hip.  The twin runs p7x_shufflewalk.hpp over the sequences on a few threads and gives the bytes of the
// kernels; DigitalSequence.shuffle is served from it, and option "host_shuffle" sends the block entry point here too.
#include "p7x_shuffle.hpp"
#include "p7x_shufflewalk.hpp"
#include "p7x.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>

namespace p7x {

static_assert(SHUF_MONO == P7X_SHUFFLE_MONO && SHUF_DI == P7X_SHUFFLE_DI && SHUF_WINDOW == P7X_SHUFFLE_WINDOW && SHUF_REVERSE == P7X_SHUFFLE_REVERSE,
              "the modes of p7x.h");

static int shuffle_slab()
{
  int s = debug_opt(OPT_SHUFFLE_SLAB);
  if (s <= 0) s = kShufSlabDefault;
  return std::min(std::max(s / 64 * 64, kShufSlabMin), kShufSlabMax);
}

void shuffle_plan(const int64_t *offsets, const int32_t *lengths, int64_t n, int mode, ShufflePlan &plan)
{
  plan = ShufflePlan();
  plan.slab = shuffle_slab();
  plan.region = mode == SHUF_DI ? plan.slab / 2 : plan.slab;
  int64_t first = -1, span = 0;           // the open run: its first sequence, its span
  int32_t count = 0;
  auto close = [&] { if (first >= 0) { plan.run_first.push_back(first); plan.run_count.push_back(count); } first = -1; };
  for (int64_t s = 0; s < n; ++s) {
    const int64_t L = lengths[s];
    if (L + 2 > plan.region) { close(); plan.long_idx.push_back(s); continue; }
    if (first >= 0 && (count == kShufThreads || span + L + 1 > plan.region)) close();
    if (first < 0) { first = s; count = 0; span = 1; }
    ++count; span += L + 1;
  }
  close();
  (void) offsets;                         // the packing fixes them: a span is the lengths and the sentinels
}

namespace {

int check_block(const ShuffleView &in, int abc_type, int mode)
{
  if (in.n < 0 || !in.dsq || (in.n && (!in.offsets || !in.lengths)) || in.nbytes < 1) { set_error("shuffle: bad packed block"); return P7X_EINVAL; }
  if (in.dsq[0] != 255) { set_error("shuffle: the packed block does not start with a sentinel"); return P7X_EINVAL; }
  int64_t pos = 1;
  for (int64_t s = 0; s < in.n; ++s) {
    if (in.lengths[s] < 0 || in.offsets[s] != pos || pos + in.lengths[s] >= in.nbytes || in.dsq[pos + in.lengths[s]] != 255) {
      set_error("shuffle: sequence " + std::to_string(s) + " is not packed as 255 x1..xL 255");
      return P7X_EINVAL;
    }
    pos += (int64_t) in.lengths[s] + 1;
  }
  if (pos != in.nbytes) { set_error("shuffle: the lengths of the packed block do not add up"); return P7X_EINVAL; }
  if (mode == SHUF_DI) {                  // the pair counters are indexed by the codes
    const int Kp = Alphabet::get(abc_type).Kp;
    for (int64_t s = 0; s < in.n; ++s) {
      const uint8_t *x = in.dsq + in.offsets[s];
      uint8_t top = 0;
      for (int32_t i = 0; i < in.lengths[s]; ++i) top = std::max(top, x[i]);
      if (top >= Kp) { set_error("shuffle: sequence " + std::to_string(s) + " holds a code outside the alphabet"); return P7X_EINVAL; }
    }
  }
  return P7X_OK;
}

int check_arguments(int abc_type, int mode, int32_t window, const uint8_t *out_dsq)
{
  if (abc_type != P7X_AMINO && abc_type != P7X_DNA && abc_type != P7X_RNA) { set_error("shuffle: unknown alphabet"); return P7X_EINVAL; }
  if (mode < 0 || mode >= SHUF_NMODES) { set_error("shuffle: unknown mode"); return P7X_EINVAL; }
  if (window < 0 || (mode == SHUF_WINDOW && window == 0)) { set_error("shuffle: the window must be at least one residue"); return P7X_EINVAL; }
  if (!out_dsq) { set_error("shuffle: no output"); return P7X_EINVAL; }
  return P7X_OK;
}

void shuffle_block_host(const ShuffleView &in, const ShufflePlan &plan, int mode, int32_t window, uint32_t seed, int threads, uint8_t *out_dsq,
                        int64_t *stats)
{
  const auto t0 = std::chrono::steady_clock::now();
  std::memcpy(out_dsq, in.dsq, (size_t) in.nbytes);
  if (threads <= 0) threads = (int) std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
  // sequences in turns of a few, so that a long one holds up one worker only
  const int64_t turn = std::max<int64_t>(1, std::min<int64_t>(256, in.n / (8 * (int64_t) threads)));
  std::atomic<int64_t> next{ 0 };
  auto work = [&] {
    std::vector<uint8_t> E;
    for (int64_t s0; (s0 = next.fetch_add(turn)) < in.n; )
      for (int64_t s = s0; s < std::min(in.n, s0 + turn); ++s) {
        const int32_t L = in.lengths[s];
        if (mode == SHUF_DI && (size_t) L > E.size()) E.resize((size_t) L);
        shuffle_sequence(mode, out_dsq + in.offsets[s], L, E.data(), window, seed, (uint64_t) s);
      }
  };
  const int nw = (int) std::min<int64_t>(threads, (in.n + turn - 1) / turn);
  std::vector<std::thread> pool;
  for (int w = 1; w < nw; ++w) pool.emplace_back(work);
  work();
  for (auto &t : pool) t.join();
  if (stats) {
    stats[SHUF_STAT_KERNEL_NS] = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    stats[SHUF_STAT_UPLOAD_NS] = 0;
    stats[SHUF_STAT_RUNS] = (int64_t) plan.run_first.size();
    stats[SHUF_STAT_LONG] = (int64_t) plan.long_idx.size();
    stats[SHUF_STAT_ON_DEVICE] = 0;
  }
}

int shuffle_entry(int32_t abc_type, int device, const ShuffleView &in, int mode, int32_t window, uint32_t seed, bool host, int threads,
                  uint8_t *out_dsq, int64_t *stats)
{
  int st = check_arguments(abc_type, mode, window, out_dsq);
  if (st != P7X_OK) return st;
  if ((st = check_block(in, abc_type, mode)) != P7X_OK) return st;
  ShufflePlan plan;
  shuffle_plan(in.offsets, in.lengths, in.n, mode, plan);
  if (host) { shuffle_block_host(in, plan, mode, window, seed, threads, out_dsq, stats); return P7X_OK; }
  return shuffle_block_device(device, in, plan, mode, window, seed, out_dsq, stats);
}

} // namespace
} // namespace p7x

using namespace p7x;

extern "C" {

int p7x_shuffle_block(int32_t abc_type, int device, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, size_t n, int64_t nbytes,
                      int mode, int32_t window, uint32_t seed, uint8_t *out_dsq, int64_t *stats)
{
  const ShuffleView in{ dsq, offsets, lengths, (int64_t) n, nbytes };
  return shuffle_entry(abc_type, device, in, mode, window, seed, debug_opt(OPT_HOST_SHUFFLE) > 0, 0, out_dsq, stats);
}

int p7x_shuffle_host(int32_t abc_type, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, size_t n, int64_t nbytes, int mode,
                     int32_t window, uint32_t seed, int threads, uint8_t *out_dsq, int64_t *stats)
{
  const ShuffleView in{ dsq, offsets, lengths, (int64_t) n, nbytes };
  return shuffle_entry(abc_type, -1, in, mode, window, seed, true, threads, out_dsq, stats);
}

int p7x_shuffle_plan(const int64_t *offsets, const int32_t *lengths, size_t n, int mode, int64_t *runs, int64_t *long_sequences, int32_t *slab)
{
  if (mode < 0 || mode >= SHUF_NMODES || (n && !lengths)) { set_error("p7x_shuffle_plan: bad arguments"); return P7X_EINVAL; }
  for (size_t s = 0; s < n; ++s) if (lengths[s] < 0) { set_error("p7x_shuffle_plan: a negative length"); return P7X_EINVAL; }
  ShufflePlan plan;
  shuffle_plan(offsets, lengths, (int64_t) n, mode, plan);
  if (runs) *runs = (int64_t) plan.run_first.size();
  if (long_sequences) *long_sequences = (int64_t) plan.long_idx.size();
  if (slab) *slab = plan.slab;
  return P7X_OK;
}

} // extern "C"
