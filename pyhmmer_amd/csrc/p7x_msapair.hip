// p7x_msapair.hip -- pairwise identity of the rows of an alignment on the device (gfx950).
//
// The two byte images of the alignment (p7x_msapair.hpp) are uploaded once.  One kernel, pair_tile_kernel: a block of 256
// threads owns a tile of T x T pairs (T <= 64 rows of set a against T rows of set b; the sets are row index lists or
// ranges).  It walks the columns in chunks of 32 dwords: the chunk of the tile's rows of image A and of image B is staged in
// LDS (a thread loads dword t % 32 of rows t / 32, t / 32 + 8, ...: 128 contiguous bytes per row), then thread (tx, ty)
// = (t % 16, t / 16) counts the differing bytes of its 4 x 4 pairs, rows ty + 16 a against rows tx + 16 b, four dwords
// per ds_read_b128: xor-and-add, and, adding population count per dword pair (pair_dword_diff), 32-bit accumulators in
// registers.
// LDS layout: row r at dword r * 36.  A ds_read_b128 is served in groups of 16 lanes that hold all 16 values of tx and
// two of ty: the 16 rows tx + 16 b start at dwords 36 tx mod 64 = {0, 36, 8, 44, ...}, sixteen different slots of four banks,
// and the two rows of A differ by 36 dwords: no conflict; the staging ds_write_b32 of a half wavefront goes to 32 consecutive
// dwords.  Rows and dwords beyond the end are staged as the images' "other" bytes, which differ, so idents = (bytes
// staged) - (bytes that differ) needs no tail code.
// Outputs (any subset): the counts, the link bits (idents >= need[min len]) packed 64 to a word, and for every row of a
// whether it is linked to any row of b (integer atomicOr across the tiles of a row).  No floating point anywhere.
#include "p7x_msapair.hpp"
#include "p7x_device.hpp"
#include <cstring>

namespace p7x {

struct PairArgs {
  const uint32_t *img_a, *img_b;           // [N][lp4] dwords
  const int32_t *rows_a, *rows_b;          // row lists or nullptr
  int64_t base_a, base_b;
  int na, nb, lp4, tile, lower;
  const uint32_t *len, *need;
  uint32_t *idents;                        // [na][nb]
  unsigned long long *bits;                // [na][words]
  int words;
  uint32_t *any;                           // [na]
};

__global__ __launch_bounds__(256) void pair_tile_kernel(PairArgs p)
{
  __shared__ __attribute__((aligned(16))) uint32_t sa[kPairTileMax * kPairStride];
  __shared__ __attribute__((aligned(16))) uint32_t sb[kPairTileMax * kPairStride];
  const int T = p.tile;
  const int64_t i0 = (int64_t) blockIdx.y * T, j0 = (int64_t) blockIdx.x * T;
  // lower: the tile's smallest index in b against its largest in a (the sets are the same rows then)
  if (p.lower && p.base_b + j0 > p.base_a + i0 + (T - 1)) return;
  const int t = (int) threadIdx.x, tx = t & 15, ty = t >> 4;
  const int sk = t & 31, sr = t >> 5;       // staging: dword sk of rows sr + 8 q

  // where this thread's eight staged rows of either image begin; -1: beyond the tile or the set
  int64_t off_a[8], off_b[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int r = sr + 8 * q;
    off_a[q] = off_b[q] = -1;
    if (r < T && i0 + r < p.na) off_a[q] = (p.rows_a ? (int64_t) p.rows_a[i0 + r] : p.base_a + i0 + r) * p.lp4;
    if (r < T && j0 + r < p.nb) off_b[q] = (p.rows_b ? (int64_t) p.rows_b[j0 + r] : p.base_b + j0 + r) * p.lp4;
  }
  uint32_t diff[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) diff[a][b] = 0;

  int staged = 0;                           // dwords of every row that were compared
  for (int c0 = 0; c0 < p.lp4; c0 += kPairChunk, staged += kPairChunk) {
    const bool in = c0 + sk < p.lp4;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = sr + 8 * q;
      sa[r * kPairStride + sk] = in && off_a[q] >= 0 ? p.img_a[off_a[q] + c0 + sk] : kPairFillA;
      sb[r * kPairStride + sk] = in && off_b[q] >= 0 ? p.img_b[off_b[q] + c0 + sk] : kPairFillB;
    }
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < kPairChunk; k += 4) {
      uint4 va[4], vb[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) va[a] = *reinterpret_cast<const uint4 *>(&sa[(ty + 16 * a) * kPairStride + k]);
#pragma unroll
      for (int b = 0; b < 4; ++b) vb[b] = *reinterpret_cast<const uint4 *>(&sb[(tx + 16 * b) * kPairStride + k]);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          uint32_t d = diff[a][b];
          d = pair_dword_diff(d, va[a].x, vb[b].x);
          d = pair_dword_diff(d, va[a].y, vb[b].y);
          d = pair_dword_diff(d, va[a].z, vb[b].z);
          diff[a][b] = pair_dword_diff(d, va[a].w, vb[b].w);
        }
    }
    __syncthreads();
  }

  const uint32_t bytes = (uint32_t) staged * 4u;
  const bool want_link = p.bits != nullptr || p.any != nullptr;
  const bool fast_bits = p.bits != nullptr && T == 64;       // a tile's 64 columns are one word of the row
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int ri = ty + 16 * a;
    const int64_t i = i0 + ri;
    const bool vi = ri < T && i < p.na;
    uint32_t len_i = 0;
    if (vi && want_link) len_i = p.len[p.rows_a ? (int64_t) p.rows_a[i] : p.base_a + i];
    unsigned long long word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int rj = tx + 16 * b;
      const int64_t j = j0 + rj;
      if (!(vi && rj < T && j < p.nb)) continue;
      const uint32_t idents = bytes - diff[a][b];
      if (p.idents) p.idents[i * p.nb + j] = idents;
      if (want_link) {
        const uint32_t len_j = p.len[p.rows_b ? (int64_t) p.rows_b[j] : p.base_b + j];
        if (pair_linked(idents, len_i, len_j, p.need)) {
          word |= 1ull << rj;
          if (p.bits && !fast_bits) atomicOr(&p.bits[i * p.words + (j >> 6)], 1ull << (j & 63));
        }
      }
    }
    if (want_link) {
      // the sixteen lanes that share ty hold the row's 64 bits between them
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) {
        const uint32_t lo = (uint32_t) __shfl_xor((int) (uint32_t) word, d, 64), hi = (uint32_t) __shfl_xor((int) (uint32_t) (word >> 32), d, 64);
        word |= ((unsigned long long) hi << 32) | lo;
      }
      if (tx == 0 && vi) {
        if (fast_bits) p.bits[i * p.words + (j0 >> 6)] = word;
        if (p.any && word) atomicOr(&p.any[i], 1u);
      }
    }
  }
}

struct PairSet {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev[8] = {};      // upload / one job: 0, 1; the bands: three a buffer
  DeviceBuf img_a, img_b, len, need, rows_a, rows_b, idents, bits[2], any;
  PinnedBuf host[2];
  // the end of a lease: the images can be gigabytes and belong to one call
  void on_return()
  {
    if (stream) (void) hipStreamSynchronize(stream);
    img_a.reset(); img_b.reset(); idents.reset(); bits[0].reset(); bits[1].reset();
  }
};

struct PairDevice {
  DeviceCtx *ctx = nullptr;
  Lease<PairSet> lease;
  int64_t N = 0;
  int lp4 = 0, tile = kPairTileMax;
};

static double elapsed_ns(hipEvent_t a, hipEvent_t b)
{
  float ms = 0.0f;
  return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (double) ms * 1.0e6 : 0.0;
}

int pair_device_open(int device, const PairImages &img, const std::vector<uint32_t> &need, int tile, PairStats &st, PairDevice **out)
{
  DeviceCtx *ctx = nullptr;
  int rc = get_ctx(device, &ctx);
  if (rc != P7X_OK) return rc;
  P7X_HIP(hipSetDevice(ctx->device));
  auto *d = new PairDevice();
  d->ctx = ctx;
  d->lease = LeasePool<PairSet>::instance().lease(ctx->device, [](const PairSet &, const PairSet *b) { return !b; });
  *out = d;                                  // the caller closes it, whatever happens below
  d->N = img.N; d->lp4 = img.Lp / 4;
  d->tile = tile >= 1 && tile <= kPairTileMax ? tile : kPairTileMax;
  PairSet &set = *d->lease;
  if (!set.stream) P7X_HIP(hipStreamCreateWithFlags(&set.stream, hipStreamNonBlocking));
  for (auto &e : set.ev) if (!e) P7X_HIP(hipEventCreate(&e));
  const size_t bytes = (size_t) img.N * (size_t) img.Lp, nb = (size_t) img.N * sizeof(uint32_t), tb = need.size() * sizeof(uint32_t);
  if ((rc = set.img_a.reserve(ctx, bytes)) != P7X_OK) return rc;
  if ((rc = set.img_b.reserve(ctx, bytes)) != P7X_OK) return rc;
  if ((rc = set.len.reserve(ctx, nb)) != P7X_OK) return rc;
  if ((rc = set.need.reserve(ctx, tb)) != P7X_OK) return rc;
  P7X_HIP(hipEventRecord(set.ev[0], set.stream));
  P7X_HIP(hipMemcpyAsync(set.img_a.as<void>(), img.a.data(), bytes, hipMemcpyHostToDevice, set.stream));
  P7X_HIP(hipMemcpyAsync(set.img_b.as<void>(), img.b.data(), bytes, hipMemcpyHostToDevice, set.stream));
  P7X_HIP(hipMemcpyAsync(set.len.as<void>(), img.len.data(), nb, hipMemcpyHostToDevice, set.stream));
  P7X_HIP(hipMemcpyAsync(set.need.as<void>(), need.data(), tb, hipMemcpyHostToDevice, set.stream));
  P7X_HIP(hipEventRecord(set.ev[1], set.stream));
  P7X_HIP(hipStreamSynchronize(set.stream));
  st.upload_ns += elapsed_ns(set.ev[0], set.ev[1]);
  st.on_device = 1;
  return P7X_OK;
}

void pair_device_close(PairDevice *d) { delete d; }

// the kernel's arguments for rows [base_a, base_a + na) or a list against rows [base_b, ...) or a list; the grid
static int pair_launch(PairDevice *d, PairArgs &a, PairStats &st)
{
  PairSet &set = *d->lease;
  const int T = d->tile;
  const int64_t ga = (a.na + T - 1) / T, gb = (a.nb + T - 1) / T;
  if (ga > 65535 || gb > 0x7fffffff) { set_error("pairwise identity: too many tiles in one launch"); return P7X_ERANGE; }
  a.img_a = set.img_a.as<uint32_t>(); a.img_b = set.img_b.as<uint32_t>();
  a.len = set.len.as<uint32_t>(); a.need = set.need.as<uint32_t>();
  a.lp4 = d->lp4; a.tile = T;
  hipLaunchKernelGGL(pair_tile_kernel, dim3((unsigned) gb, (unsigned) ga), dim3(256), 0, set.stream, a);
  P7X_HIP(hipGetLastError());
  // the pairs of the tiles that are looked at (with <lower>, those not wholly above the diagonal)
  if (!a.lower) st.pairs += (int64_t) a.na * (int64_t) a.nb;
  else
    for (int64_t ti = 0; ti < ga; ++ti) {
      const int64_t top = a.base_a - a.base_b + ti * T + (T - 1);      // the largest index in b that the row of tiles reaches
      if (top < 0) continue;
      st.pairs += std::min<int64_t>(T, a.na - ti * T) * std::min<int64_t>(a.nb, (top / T + 1) * T);
    }
  return P7X_OK;
}

int pair_device_run(PairDevice *d, const PairJob &job, PairStats &st)
{
  PairSet &set = *d->lease;
  DeviceCtx *ctx = d->ctx;
  if (job.na < 1 || job.nb < 1 || job.na > 0x7fffffff || job.nb > 0x7fffffff) { set_error("pairwise identity: bad row sets"); return P7X_EINVAL; }
  PairArgs a;
  std::memset(&a, 0, sizeof(a));
  a.base_a = job.base_a; a.base_b = job.base_b; a.na = (int) job.na; a.nb = (int) job.nb; a.lower = job.lower ? 1 : 0;
  a.words = (int) ((job.nb + 63) / 64);
  int rc;
  const size_t ra = (size_t) job.na * sizeof(int32_t), rb = (size_t) job.nb * sizeof(int32_t);
  const size_t ib = (size_t) job.na * (size_t) job.nb * sizeof(uint32_t), wb = (size_t) job.na * (size_t) a.words * sizeof(uint64_t);
  const size_t ab = (size_t) job.na * sizeof(uint32_t);
  if (job.rows_a) {
    if ((rc = set.rows_a.reserve(ctx, ra)) != P7X_OK) return rc;
    P7X_HIP(hipMemcpyAsync(set.rows_a.as<void>(), job.rows_a, ra, hipMemcpyHostToDevice, set.stream));
    a.rows_a = set.rows_a.as<int32_t>();
  }
  if (job.rows_b) {
    if ((rc = set.rows_b.reserve(ctx, rb)) != P7X_OK) return rc;
    P7X_HIP(hipMemcpyAsync(set.rows_b.as<void>(), job.rows_b, rb, hipMemcpyHostToDevice, set.stream));
    a.rows_b = set.rows_b.as<int32_t>();
  }
  if (job.idents) {
    if ((rc = set.idents.reserve(ctx, ib)) != P7X_OK) return rc;
    P7X_HIP(hipMemsetAsync(set.idents.as<void>(), 0, ib, set.stream));
    a.idents = set.idents.as<uint32_t>();
  }
  if (job.bits) {
    if ((rc = set.bits[0].reserve(ctx, wb)) != P7X_OK) return rc;
    P7X_HIP(hipMemsetAsync(set.bits[0].as<void>(), 0, wb, set.stream));
    a.bits = set.bits[0].as<unsigned long long>();
  }
  if (job.any) {
    if ((rc = set.any.reserve(ctx, ab)) != P7X_OK) return rc;
    P7X_HIP(hipMemsetAsync(set.any.as<void>(), 0, ab, set.stream));
    a.any = set.any.as<uint32_t>();
  }
  P7X_HIP(hipEventRecord(set.ev[0], set.stream));
  if ((rc = pair_launch(d, a, st)) != P7X_OK) return rc;
  P7X_HIP(hipEventRecord(set.ev[1], set.stream));
  std::vector<uint32_t> any32;
  if (job.idents) P7X_HIP(hipMemcpyAsync(job.idents, set.idents.as<void>(), ib, hipMemcpyDeviceToHost, set.stream));
  if (job.bits) P7X_HIP(hipMemcpyAsync(job.bits, set.bits[0].as<void>(), wb, hipMemcpyDeviceToHost, set.stream));
  if (job.any) { any32.resize((size_t) job.na); P7X_HIP(hipMemcpyAsync(any32.data(), set.any.as<void>(), ab, hipMemcpyDeviceToHost, set.stream)); }
  P7X_HIP(hipStreamSynchronize(set.stream));
  if (job.any) for (int64_t i = 0; i < job.na; ++i) job.any[i] = any32[(size_t) i] != 0;
  st.kernel_ns += elapsed_ns(set.ev[0], set.ev[1]);
  return P7X_OK;
}

int pair_device_bands(PairDevice *d, int64_t N, PairBandVisitor visit, void *user, PairStats &st)
{
  PairSet &set = *d->lease;
  DeviceCtx *ctx = d->ctx;
  const int T = d->tile;
  // a band: whole tiles of rows, about 8 MiB of link bits (at least one tile), at most 65,535 tiles
  const int64_t words_all = (N + 63) / 64;
  int64_t band = ((int64_t) 1 << 20) / std::max<int64_t>(1, words_all) / T * T;
  band = std::min<int64_t>(std::max<int64_t>(band, T), (int64_t) 65535 * T);
  if (debug_opt(OPT_PAIRID_TILE) > 0) band = 2 * T;      // the seam: small alignments cross bands too
  int rc;
  const size_t cap = (size_t) band * (size_t) words_all * sizeof(uint64_t);
  for (int s = 0; s < 2; ++s) {
    if ((rc = set.bits[s].reserve(ctx, cap)) != P7X_OK) return rc;
    if ((rc = set.host[s].reserve(cap)) != P7X_OK) return rc;
  }
  struct Band { int64_t i0 = 0, i1 = 0, words = 0; bool busy = false; } inflight[2];
  // events of buffer s: 2 + 3 s kernel begin, + 1 kernel end, + 2 copy done
  auto finish = [&](int s) -> int {
    Band &b = inflight[s];
    if (!b.busy) return P7X_OK;
    P7X_HIP(hipEventSynchronize(set.ev[2 + 3 * s + 2]));
    st.kernel_ns += elapsed_ns(set.ev[2 + 3 * s], set.ev[2 + 3 * s + 1]);
    visit(user, b.i0, b.i1, b.words, set.host[s].as<uint64_t>());
    b.busy = false;
    return P7X_OK;
  };
  // the device runs one band ahead: the host walks band k - 2 while band k - 1 is computed, then queues band k
  int s = 0;
  for (int64_t i0 = 0; i0 < N; i0 += band, s ^= 1) {
    const int64_t i1 = std::min(N, i0 + band);
    if ((rc = finish(s)) != P7X_OK) return rc;
    PairArgs a;
    std::memset(&a, 0, sizeof(a));
    a.base_a = i0; a.base_b = 0; a.na = (int) (i1 - i0); a.nb = (int) i1; a.lower = 1;
    a.words = (int) ((i1 + 63) / 64);
    const size_t wb = (size_t) a.na * (size_t) a.words * sizeof(uint64_t);
    P7X_HIP(hipMemsetAsync(set.bits[s].as<void>(), 0, wb, set.stream));
    a.bits = set.bits[s].as<unsigned long long>();
    P7X_HIP(hipEventRecord(set.ev[2 + 3 * s], set.stream));
    if ((rc = pair_launch(d, a, st)) != P7X_OK) return rc;
    P7X_HIP(hipEventRecord(set.ev[2 + 3 * s + 1], set.stream));
    P7X_HIP(hipMemcpyAsync(set.host[s].as<void>(), set.bits[s].as<void>(), wb, hipMemcpyDeviceToHost, set.stream));
    P7X_HIP(hipEventRecord(set.ev[2 + 3 * s + 2], set.stream));
    inflight[s].i0 = i0; inflight[s].i1 = i1; inflight[s].words = a.words; inflight[s].busy = true;
  }
  if ((rc = finish(s)) != P7X_OK) return rc;          // the older band first
  return finish(s ^ 1);
}

} // namespace p7x
