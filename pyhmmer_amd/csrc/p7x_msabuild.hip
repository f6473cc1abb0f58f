// p7x_msabuild.hip -- Builder.build_msa: the passes over the alignment on the device (gfx950).
//
// The alignment is uploaded once as an N x Lp byte matrix (p7x_msabuild.hpp).  Four passes read it; between them the
// host decides, from O(L) or O(N) numbers, which columns weigh, what the weights are and which columns are consensus.
//
//   msa_colcount_kernel<false>   rows holding each code, per column.  A block is one wavefront: it owns a tile of 256
//                                columns and a chunk of rows, each lane reads a dword (four columns) of every row and keeps
//                                its columns' 29 x 4 counters in LDS, laid out [code][column of the lane][lane]: dword
//                                index = slot * 64 + lane, so the 32 lanes of either half of the wavefront (the unit
//                                within which LDS accesses conflict) fall into 32 different banks whatever codes they
//                                hold.  No lane touches another's counters: no atomics and no barrier inside the block.
//                                The partial counts of the row chunks meet in global memory through integer atomics.
//   msa_pbweight_kernel          one wavefront per row: the sum of the fixed-point terms of its residues in the weighting
//                                columns and how many residues it has there.
//   msa_colcount_kernel<true>    the same tile walk with the row's 64-bit weight added instead of one, two columns per lane
//                                (the counters are twice as wide, the LDS per block stays 29 KiB; a 64-bit write of 32
//                                lanes spans two bank rows, which costs what it must).
//   msa_trans_kernel             a thread owns a node and walks a chunk of rows: the step from its node to the next
//                                (msa_step, shared with the host twin) into eight register accumulators, flushed with
//                                integer atomics; a residue that a delete takes from a neighbouring run (rare) goes
//                                straight to global memory.
// Every sum is an integer sum, so the results do not depend on the grid, the row chunk ("build_rows") or the schedule.
#include "p7x_msabuild.hpp"
#include "p7x_device.hpp"
#include <cstring>

namespace p7x {

template <bool W> struct MsaAcc { using type = uint32_t; using load = uint32_t; static constexpr int CPL = 4; };
template <> struct MsaAcc<true> { using type = unsigned long long; using load = uint16_t; static constexpr int CPL = 2; };

template <bool W>
__global__ __launch_bounds__(64) void msa_colcount_kernel(const uint8_t *ax, int64_t N, int Lp, int rows_per_block,
                                                          const unsigned long long *wq, typename MsaAcc<W>::type *out)
{
  using acc_t = typename MsaAcc<W>::type;
  using load_t = typename MsaAcc<W>::load;
  constexpr int CPL = MsaAcc<W>::CPL;
  __shared__ acc_t cnt[kMsaCodes * CPL * 64];
  const int lane = (int) threadIdx.x;
  const int col = ((int) blockIdx.x * 64 + lane) * CPL;
  if (col >= Lp) return;                              // Lp is a multiple of four: a lane's columns are all inside or all outside
  for (int s = 0; s < kMsaCodes * CPL; ++s) cnt[s * 64 + lane] = 0;
  const int64_t r0 = (int64_t) blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
  const uint8_t *p = ax + (size_t) r0 * (size_t) Lp + (size_t) col;
#pragma unroll 4
  for (int64_t r = r0; r < r1; ++r, p += Lp) {
    const uint32_t v = (uint32_t) *reinterpret_cast<const load_t *>(p);
    acc_t w = 1;
    if constexpr (W) w = wq[r];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const uint32_t code = (v >> (8 * j)) & 0xffu;
      if (code < (uint32_t) kMsaCodes) cnt[((int) code * CPL + j) * 64 + lane] += w;
    }
  }
  for (int code = 0; code < kMsaCodes; ++code)
    for (int j = 0; j < CPL; ++j) {
      const acc_t v = cnt[(code * CPL + j) * 64 + lane];
      if (v) atomicAdd(&out[(size_t) (col + j) * kMsaSlots + code], v);
    }
}

__global__ __launch_bounds__(256) void msa_pbweight_kernel(const uint8_t *ax, int64_t N, int Lp, const uint8_t *wmask,
                                                           const unsigned long long *termq, unsigned long long *rowsum, int32_t *rowlen)
{
  const int64_t row = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = (int) (threadIdx.x & 63);
  if (row >= N) return;
  const uint32_t *p = reinterpret_cast<const uint32_t *>(ax + (size_t) row * (size_t) Lp);
  const uint32_t *m = reinterpret_cast<const uint32_t *>(wmask);
  unsigned long long s = 0;
  int len = 0;
  for (int c4 = lane; c4 < Lp / 4; c4 += 64) {
    const uint32_t v = p[c4], use = m[c4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((use >> (8 * j)) & 0xffu)) continue;
      const uint32_t a = (v >> (8 * j)) & 0xffu;
      if (msa_is_canonical(a)) { s += termq[(size_t) (c4 * 4 + j) * 20 + a]; ++len; }
      else if (msa_is_residue(a)) ++len;
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = (uint32_t) __shfl_xor((int) (uint32_t) s, d, 64), hi = (uint32_t) __shfl_xor((int) (uint32_t) (s >> 32), d, 64);
    s += ((unsigned long long) hi << 32) | lo;
    len += __shfl_xor(len, d, 64);
  }
  if (lane == 0) { rowsum[row] = s; rowlen[row] = len; }
}

__global__ __launch_bounds__(256) void msa_trans_kernel(const uint8_t *ax, int64_t N, int Lp, int rows_per_block, const uint8_t *frag,
                                                        const unsigned long long *wq, const int32_t *map, int M,
                                                        unsigned long long *trq, unsigned long long *taken)
{
  const int k = (int) (blockIdx.x * blockDim.x + threadIdx.x);
  if (k > M) return;
  const int64_t r0 = (int64_t) blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
  unsigned long long mm = 0, mi = 0, md = 0, im = 0, ii = 0, ii_high = 0, dm = 0, dd = 0;
  for (int64_t r = r0; r < r1; ++r) {
    const MsaStep s = msa_step(ax + (size_t) r * (size_t) Lp, map, M, k, frag[r] != 0);
    const unsigned long long w = wq[r];
    if (s.slot == 0) mm += w; else if (s.slot == 2) md += w; else if (s.slot == 5) dm += w; else if (s.slot == 6) dd += w;
    if (s.nins > 0) { mi += w; ii += msa_ii_low(w, s.nins); ii_high += msa_ii_high(w, s.nins); im += w; }
    if (s.taken >= 0) atomicAdd(&taken[(size_t) k * kMsaSlots + s.taken], w);
  }
  unsigned long long *t = trq + (size_t) k * 8;
  if (mm) atomicAdd(&t[0], mm);
  if (mi) atomicAdd(&t[1], mi);
  if (md) atomicAdd(&t[2], md);
  if (im) atomicAdd(&t[3], im);
  if (ii) atomicAdd(&t[4], ii);
  if (dm) atomicAdd(&t[5], dm);
  if (dd) atomicAdd(&t[6], dd);
  if (ii_high) atomicAdd(&t[7], ii_high);
}

struct MsaSet {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = { nullptr, nullptr };
  DeviceBuf ax, frag, colcnt, wmask, termq, rowsum, rowlen, wq, wcnt, map, trq, taken;
  // the end of a lease: the alignment can be gigabytes and belongs to one call, so it goes back to the slab pool
  void on_return()
  {
    if (stream) (void) hipStreamSynchronize(stream);
    ax.reset();
  }
};

struct MsaDevice {
  DeviceCtx *ctx = nullptr;
  Lease<MsaSet> lease;
  int rows_per_block = 0;
  unsigned nchunks = 0;
};

// the event pair around a pass, read after the stream has been synchronised
static int timed(MsaSet &set, double *us)
{
  float ms = 0.0f;
  *us = hipEventElapsedTime(&ms, set.ev[0], set.ev[1]) == hipSuccess ? (double) ms * 1000.0 : 0.0;      // no time rather than a stale one
  return P7X_OK;
}

int msa_device_open(int device, p7x_msacounts &c, MsaDevice **out)
{
  DeviceCtx *ctx = nullptr;
  int st = get_ctx(device, &ctx);
  if (st != P7X_OK) return st;
  P7X_HIP(hipSetDevice(ctx->device));
  auto *d = new MsaDevice();
  d->ctx = ctx;
  d->lease = LeasePool<MsaSet>::instance().lease(ctx->device, [](const MsaSet &, const MsaSet *b) { return !b; });
  *out = d;                                  // the caller closes it, whatever happens below
  MsaSet &set = *d->lease;
  if (!set.stream) P7X_HIP(hipStreamCreateWithFlags(&set.stream, hipStreamNonBlocking));
  for (auto &e : set.ev) if (!e) P7X_HIP(hipEventCreate(&e));
  // the row chunk of a block: enough blocks to fill the device eight times over, at least 64 rows each; "build_rows" overrides
  int64_t rows = c.rows_per_block;
  if (rows <= 0) {
    const int64_t tiles = (c.Lp + 255) / 256, want = std::max<int64_t>(1, (int64_t) ctx->num_cu * 8 / tiles);
    rows = std::max<int64_t>(64, (c.N + want - 1) / want);
  }
  rows = std::min<int64_t>(rows, c.N);
  // the grid's second dimension holds 65,535 blocks
  rows = std::max<int64_t>(rows, (c.N + 65534) / 65535);
  d->rows_per_block = (int) rows;
  d->nchunks = (unsigned) ((c.N + rows - 1) / rows);
  c.rows_per_block = d->rows_per_block;
  const size_t ax_bytes = (size_t) c.N * (size_t) c.Lp;
  if ((st = set.ax.reserve(ctx, ax_bytes)) != P7X_OK) return st;
  if ((st = set.frag.reserve(ctx, (size_t) c.N)) != P7X_OK) return st;
  P7X_HIP(hipEventRecord(set.ev[0], set.stream));
  P7X_HIP(hipMemcpyAsync(set.ax.as<uint8_t>(), c.ax.data(), ax_bytes, hipMemcpyHostToDevice, set.stream));
  P7X_HIP(hipMemcpyAsync(set.frag.as<uint8_t>(), c.frag.data(), (size_t) c.N, hipMemcpyHostToDevice, set.stream));
  P7X_HIP(hipEventRecord(set.ev[1], set.stream));
  P7X_HIP(hipStreamSynchronize(set.stream));
  return timed(set, &c.upload_us);
}

void msa_device_close(MsaDevice *d) { delete d; }

template <bool W>
static int launch_colcount(MsaDevice *d, p7x_msacounts &c, DeviceBuf &dst, void *host_out, double *us)
{
  using acc_t = typename MsaAcc<W>::type;
  MsaSet &set = *d->lease;
  const size_t bytes = (size_t) c.Lp * kMsaSlots * sizeof(acc_t);
  int st = dst.reserve(d->ctx, bytes);
  if (st != P7X_OK) return st;
  if (W) {
    if ((st = set.wq.reserve(d->ctx, (size_t) c.N * sizeof(uint64_t))) != P7X_OK) return st;
    P7X_HIP(hipMemcpyAsync(set.wq.as<uint64_t>(), c.wq.data(), (size_t) c.N * sizeof(uint64_t), hipMemcpyHostToDevice, set.stream));
  }
  P7X_HIP(hipMemsetAsync(dst.as<void>(), 0, bytes, set.stream));
  constexpr int tile = 64 * MsaAcc<W>::CPL;
  const dim3 grid((unsigned) ((c.Lp + tile - 1) / tile), d->nchunks);
  P7X_HIP(hipEventRecord(set.ev[0], set.stream));
  hipLaunchKernelGGL(msa_colcount_kernel<W>, grid, dim3(64), 0, set.stream, set.ax.as<uint8_t>(), c.N, c.Lp, d->rows_per_block,
                     W ? set.wq.as<unsigned long long>() : nullptr, dst.as<acc_t>());
  P7X_HIP(hipGetLastError());
  P7X_HIP(hipEventRecord(set.ev[1], set.stream));
  P7X_HIP(hipMemcpyAsync(host_out, dst.as<void>(), bytes, hipMemcpyDeviceToHost, set.stream));
  P7X_HIP(hipStreamSynchronize(set.stream));
  return timed(set, us);
}

int msa_device_colcount(MsaDevice *d, p7x_msacounts &c)
{
  return launch_colcount<false>(d, c, d->lease->colcnt, c.colcnt.data(), &c.kernel_us[0]);
}

int msa_device_wcount(MsaDevice *d, p7x_msacounts &c)
{
  return launch_colcount<true>(d, c, d->lease->wcnt, c.wcnt.data(), &c.kernel_us[2]);
}

int msa_device_pbweight(MsaDevice *d, p7x_msacounts &c)
{
  MsaSet &set = *d->lease;
  DeviceCtx *ctx = d->ctx;
  const size_t n8 = (size_t) c.N * sizeof(uint64_t), n4 = (size_t) c.N * sizeof(int32_t), tq = (size_t) c.Lp * 20 * sizeof(uint64_t);
  int st;
  if ((st = set.wmask.reserve(ctx, (size_t) c.Lp)) != P7X_OK) return st;
  if ((st = set.termq.reserve(ctx, tq)) != P7X_OK) return st;
  if ((st = set.rowsum.reserve(ctx, n8)) != P7X_OK) return st;
  if ((st = set.rowlen.reserve(ctx, n4)) != P7X_OK) return st;
  P7X_HIP(hipMemcpyAsync(set.wmask.as<uint8_t>(), c.wmask.data(), (size_t) c.Lp, hipMemcpyHostToDevice, set.stream));
  P7X_HIP(hipMemcpyAsync(set.termq.as<uint64_t>(), c.termq.data(), tq, hipMemcpyHostToDevice, set.stream));
  P7X_HIP(hipEventRecord(set.ev[0], set.stream));
  hipLaunchKernelGGL(msa_pbweight_kernel, dim3((unsigned) ((c.N + 3) / 4)), dim3(256), 0, set.stream, set.ax.as<uint8_t>(), c.N, c.Lp,
                     set.wmask.as<uint8_t>(), set.termq.as<unsigned long long>(), set.rowsum.as<unsigned long long>(), set.rowlen.as<int32_t>());
  P7X_HIP(hipGetLastError());
  P7X_HIP(hipEventRecord(set.ev[1], set.stream));
  P7X_HIP(hipMemcpyAsync(c.rowsum.data(), set.rowsum.as<void>(), n8, hipMemcpyDeviceToHost, set.stream));
  P7X_HIP(hipMemcpyAsync(c.rowlen.data(), set.rowlen.as<void>(), n4, hipMemcpyDeviceToHost, set.stream));
  P7X_HIP(hipStreamSynchronize(set.stream));
  return timed(set, &c.kernel_us[1]);
}

int msa_device_transitions(MsaDevice *d, p7x_msacounts &c)
{
  MsaSet &set = *d->lease;
  DeviceCtx *ctx = d->ctx;
  const size_t mb = c.map.size() * sizeof(int32_t), tb = c.trq.size() * sizeof(uint64_t), kb = c.taken.size() * sizeof(uint64_t);
  int st;
  if ((st = set.map.reserve(ctx, mb)) != P7X_OK) return st;
  if ((st = set.trq.reserve(ctx, tb)) != P7X_OK) return st;
  if ((st = set.taken.reserve(ctx, kb)) != P7X_OK) return st;
  P7X_HIP(hipMemcpyAsync(set.map.as<int32_t>(), c.map.data(), mb, hipMemcpyHostToDevice, set.stream));
  P7X_HIP(hipMemsetAsync(set.trq.as<void>(), 0, tb, set.stream));
  P7X_HIP(hipMemsetAsync(set.taken.as<void>(), 0, kb, set.stream));
  const dim3 grid((unsigned) ((c.M + 1 + 255) / 256), d->nchunks);
  P7X_HIP(hipEventRecord(set.ev[0], set.stream));
  hipLaunchKernelGGL(msa_trans_kernel, grid, dim3(256), 0, set.stream, set.ax.as<uint8_t>(), c.N, c.Lp, d->rows_per_block,
                     set.frag.as<uint8_t>(), set.wq.as<unsigned long long>(), set.map.as<int32_t>(), c.M,
                     set.trq.as<unsigned long long>(), set.taken.as<unsigned long long>());
  P7X_HIP(hipGetLastError());
  P7X_HIP(hipEventRecord(set.ev[1], set.stream));
  P7X_HIP(hipMemcpyAsync(c.trq.data(), set.trq.as<void>(), tb, hipMemcpyDeviceToHost, set.stream));
  P7X_HIP(hipMemcpyAsync(c.taken.data(), set.taken.as<void>(), kb, hipMemcpyDeviceToHost, set.stream));
  P7X_HIP(hipStreamSynchronize(set.stream));
  return timed(set, &c.kernel_us[3]);
}

} // namespace p7x
