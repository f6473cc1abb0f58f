// p7x_shuffle.hip -- a packed block shuffled sequence by sequence on the device (gfx950): DESIGN.md 3.19.  The host twin and
// the plan are p7x_shuffle.cpp; the procedure of every mode is p7x_shufflewalk.hpp, the same code for both.
//
// The output has the input's layout, so a workgroup takes a run of consecutive sequences (p7x_shuffle.hpp: ShufflePlan),
// stages their span of the packed array in LDS with dword reads by all its lanes, lane t shuffles sequence t of the run in
// place with byte reads and writes, and the span goes back as it came.  In mode "di" the LDS holds a second region of the
// same size: the successor list of the sequence at offset o of the span is at offset o of that region.  The pair
// counters of "di" (33 + 32 dwords) are the lane's private memory.  A sequence whose own span exceeds the region is shuffled
// by a second launch, one workgroup per sequence: all its lanes copy it to the output, lane 0 shuffles it there, in
// global memory, with its successor list in a workspace laid out as the block.  Every output byte has one writer: byte 0 is
// set by the driver, a run writes its sequences and the sentinel after each, and so does the long path.
#include "p7x_shuffle.hpp"
#include "p7x_shufflewalk.hpp"
#include "p7x_device.hpp"
#include "p7x_launch.hpp"
#include "p7x.h"
#include <algorithm>

namespace p7x {
namespace {

struct ShufArgs {
  const uint8_t *in; uint8_t *out;          // the packed block and its image: nbytes each, readable / writable up to the next multiple of four
  uint8_t *work;                            // "di", long path: successor lists, laid out as the block
  int64_t nbytes;
  const int64_t *offsets; const int32_t *lengths; int64_t n;
  const int64_t *run_first; const int32_t *run_count;
  const int64_t *long_idx;
  int32_t mode, window, region;
  uint32_t seed;
};

// out[lo, hi) = src[lo - base, hi - base): bytes up to a multiple of four, dwords, bytes.  <src> is dword aligned and <base> a
// multiple of four, so both sides of a dword copy are aligned.
__device__ inline void store_span(uint8_t *out, const uint8_t *src, int64_t base, int64_t lo, int64_t hi, int tid, int nthreads)
{
  const int64_t alo = std::min(hi, (lo + 3) & ~(int64_t) 3), ahi = std::max(alo, hi & ~(int64_t) 3);
  for (int64_t p = lo + tid; p < alo; p += nthreads) out[p] = src[p - base];
  uint32_t *o32 = reinterpret_cast<uint32_t *>(out);
  const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
  for (int64_t w = (alo >> 2) + tid; w < (ahi >> 2); w += nthreads) o32[w] = s32[w - (base >> 2)];
  for (int64_t p = ahi + tid; p < hi; p += nthreads) out[p] = src[p - base];
}

__global__ __launch_bounds__(kShufThreads) void shuffle_runs_kernel(ShufArgs a)
{
  extern __shared__ __align__(16) uint8_t lds[];
  const int tid = threadIdx.x;
  const int64_t first = a.run_first[blockIdx.x];
  const int cnt = a.run_count[blockIdx.x];
  if (first < 0 || cnt < 1 || cnt > kShufThreads || first + cnt > a.n) return;
  const int64_t last = first + cnt - 1;
  const int64_t p0 = a.offsets[first] - 1, p1 = a.offsets[last] + a.lengths[last] + 1;      // the span [p0, p1), both sentinels in it
  const int64_t base = p0 & ~(int64_t) 3, w0 = base >> 2, w1 = (p1 + 3) >> 2;
  // a span the plan did not make: nothing is read or written
  if (p0 < 0 || p1 > a.nbytes || p1 - p0 > a.region || p1 <= p0) return;
  uint32_t *l32 = reinterpret_cast<uint32_t *>(lds);
  const uint32_t *in32 = reinterpret_cast<const uint32_t *>(a.in);
  for (int64_t w = w0 + tid; w < w1; w += kShufThreads) l32[w - w0] = in32[w];
  __syncthreads();
  if (tid < cnt) {
    const int64_t sq = first + tid;
    const int64_t off = a.offsets[sq] - base;
    const int32_t L = a.lengths[sq];
    if (off >= 1 && L >= 0 && off + L < p1 - base)       // inside the staged span, the sentinel after it too
      shuffle_sequence(a.mode, lds + off, L, lds + a.region + kShufLdsPad + off, a.window, a.seed, (uint64_t) sq);
  }
  __syncthreads();
  store_span(a.out, lds, base, p0 + 1, p1, tid, kShufThreads);
}

__global__ __launch_bounds__(kShufThreads) void shuffle_long_kernel(ShufArgs a)
{
  const int tid = threadIdx.x;
  const int64_t sq = a.long_idx[blockIdx.x];
  if (sq < 0 || sq >= a.n) return;
  const int64_t o = a.offsets[sq];
  const int32_t L = a.lengths[sq];
  if (o < 1 || L < 0 || o + L + 1 > a.nbytes) return;
  // the sequence and the sentinel after it, in 16-byte pieces where both sides allow (they are aligned alike)
  const int64_t lo = o, hi = o + L + 1;
  const int64_t alo = std::min(hi, (lo + 15) & ~(int64_t) 15), ahi = std::max(alo, hi & ~(int64_t) 15);
  for (int64_t p = lo + tid; p < alo; p += kShufThreads) a.out[p] = a.in[p];
  const uint4 *i16 = reinterpret_cast<const uint4 *>(a.in);
  uint4 *o16 = reinterpret_cast<uint4 *>(a.out);
  for (int64_t w = (alo >> 4) + tid; w < (ahi >> 4); w += kShufThreads) o16[w] = i16[w];
  for (int64_t p = ahi + tid; p < hi; p += kShufThreads) a.out[p] = a.in[p];
  __syncthreads();                          // the copy of the other lanes is visible to lane 0
  if (tid == 0) shuffle_sequence(a.mode, a.out + o, L, a.work ? a.work + o : nullptr, a.window, a.seed, (uint64_t) sq);
}

struct ShuffleSet {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev[3] = { nullptr, nullptr, nullptr };
  DeviceBuf in, out, work;
  // The end of a lease: the buffers are as large as the caller's block, so they go back to the slab pool.
  void on_return()
  {
    if (stream) (void) hipStreamSynchronize(stream);
    in.reset(); out.reset(); work.reset();
  }
};

} // namespace

int shuffle_block_device(int device, const ShuffleView &in, const ShufflePlan &plan, int mode, int32_t window, uint32_t seed, uint8_t *out_dsq,
                         int64_t *stats)
{
  DeviceCtx *ctx = nullptr;
  int st = get_ctx(device, &ctx);
  if (st != P7X_OK) return st;
  P7X_HIP(hipSetDevice(ctx->device));
  const size_t T = (size_t) in.nbytes, n = (size_t) in.n, nruns = plan.run_first.size(), nlong = plan.long_idx.size();
  if (nruns > 0x7fffffffu || nlong > 0x7fffffffu) { set_error("shuffle: too many runs for one launch; shuffle fewer sequences per call"); return P7X_ERANGE; }
  const bool di = mode == SHUF_DI;
  const size_t lds = (size_t) (plan.region + kShufLdsPad) * (di ? 2 : 1);

  auto lease = LeasePool<ShuffleSet>::instance().lease(ctx->device, [](const ShuffleSet &, const ShuffleSet *b) { return !b; });
  ShuffleSet &set = *lease;
  if (!set.stream) P7X_HIP(hipStreamCreateWithFlags(&set.stream, hipStreamNonBlocking));
  for (auto &e : set.ev) if (!e) P7X_HIP(hipEventCreate(&e));
  hipStream_t q = set.stream;

  // the input buffer, cut into arrays that start on multiples of 16 bytes
  size_t in_bytes = 0;
  auto take = [&in_bytes](size_t bytes) { const size_t o = in_bytes; in_bytes += (bytes + 15) / 16 * 16; return o; };
  const size_t i_dsq = take(T + 4), i_off = take(8 * n), i_len = take(4 * n), i_rf = take(8 * nruns), i_rc = take(4 * nruns), i_long = take(8 * nlong);
  const size_t out_bytes = (T + 3) / 4 * 4 + 16, work_bytes = di && nlong ? out_bytes : 0;
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      size_t budget;
      { std::lock_guard<std::mutex> lk(ctx->slab_mu); budget = free_b / 10 * 9 + ctx->slab_free_bytes; }
      if (in_bytes + out_bytes + work_bytes > budget) {
        set_error("shuffle: " + std::to_string(in_bytes + out_bytes + work_bytes) + " bytes of device memory, " + std::to_string(budget) +
                  " available: shuffle fewer sequences per call");
        return P7X_EMEM;
      }
    }
  }
  if ((st = set.in.reserve(ctx, in_bytes)) != P7X_OK) return st;
  if ((st = set.out.reserve(ctx, out_bytes)) != P7X_OK) return st;
  if (work_bytes && (st = set.work.reserve(ctx, work_bytes)) != P7X_OK) return st;
  uint8_t *d_in = set.in.as<uint8_t>();

  P7X_HIP(hipEventRecord(set.ev[0], q));
  P7X_HIP(hipMemsetAsync(d_in + i_dsq + T, 255, 4, q));
  P7X_HIP(hipMemcpyAsync(d_in + i_dsq, in.dsq, T, hipMemcpyHostToDevice, q));
  if (n) {
    P7X_HIP(hipMemcpyAsync(d_in + i_off, in.offsets, 8 * n, hipMemcpyHostToDevice, q));
    P7X_HIP(hipMemcpyAsync(d_in + i_len, in.lengths, 4 * n, hipMemcpyHostToDevice, q));
  }
  if (nruns) {
    P7X_HIP(hipMemcpyAsync(d_in + i_rf, plan.run_first.data(), 8 * nruns, hipMemcpyHostToDevice, q));
    P7X_HIP(hipMemcpyAsync(d_in + i_rc, plan.run_count.data(), 4 * nruns, hipMemcpyHostToDevice, q));
  }
  if (nlong) P7X_HIP(hipMemcpyAsync(d_in + i_long, plan.long_idx.data(), 8 * nlong, hipMemcpyHostToDevice, q));
  P7X_HIP(hipMemsetAsync(set.out.as<uint8_t>(), 255, 1, q));
  P7X_HIP(hipEventRecord(set.ev[1], q));

  ShufArgs a{};
  a.in = d_in + i_dsq; a.out = set.out.as<uint8_t>(); a.work = work_bytes ? set.work.as<uint8_t>() : nullptr; a.nbytes = in.nbytes;
  a.offsets = reinterpret_cast<const int64_t *>(d_in + i_off); a.lengths = reinterpret_cast<const int32_t *>(d_in + i_len); a.n = in.n;
  a.run_first = reinterpret_cast<const int64_t *>(d_in + i_rf); a.run_count = reinterpret_cast<const int32_t *>(d_in + i_rc);
  a.long_idx = reinterpret_cast<const int64_t *>(d_in + i_long);
  a.mode = mode; a.window = window; a.region = plan.region; a.seed = seed;
  if (nruns) {
    if ((st = kernel_grant_lds(shuffle_runs_kernel, lds)) != P7X_OK) return st;
    hipLaunchKernelGGL(shuffle_runs_kernel, dim3((unsigned) nruns), dim3(kShufThreads), lds, q, a);
    P7X_HIP(hipGetLastError());
  }
  if (nlong) {
    hipLaunchKernelGGL(shuffle_long_kernel, dim3((unsigned) nlong), dim3(kShufThreads), 0, q, a);
    P7X_HIP(hipGetLastError());
  }
  P7X_HIP(hipEventRecord(set.ev[2], q));
  P7X_HIP(hipMemcpyAsync(out_dsq, a.out, T, hipMemcpyDeviceToHost, q));
  P7X_HIP(hipStreamSynchronize(q));
  if (stats) {
    float up = 0.0f, ker = 0.0f;
    (void) hipEventElapsedTime(&up, set.ev[0], set.ev[1]);
    (void) hipEventElapsedTime(&ker, set.ev[1], set.ev[2]);
    stats[SHUF_STAT_KERNEL_NS] = (int64_t) ((double) ker * 1e6);
    stats[SHUF_STAT_UPLOAD_NS] = (int64_t) ((double) up * 1e6);
    stats[SHUF_STAT_RUNS] = (int64_t) nruns;
    stats[SHUF_STAT_LONG] = (int64_t) nlong;
    stats[SHUF_STAT_ON_DEVICE] = 1;
  }
  return P7X_OK;
}

} // namespace p7x
