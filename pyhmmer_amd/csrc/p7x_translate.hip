// p7x_translate.hip -- six-frame ORFs and in-frame translation of a packed nucleotide block on the device (gfx950);
// definitions and pass structure: DESIGN.md 3.18.  The host twin is p7x_translate.cpp.
//
// The ORF finder reads the packed array 255 x1..xL 255 ... as one stream per strand: watson is the array itself, crick the
// array read downwards through the complement map, so that both strands run the same code.  A codon that touches a
// sentinel belongs to no sequence and ends a run as a stop does.  The unit of work is a chunk of <orf_chunk> stream
// positions, one lane per chunk, cut without regard to sequences; a block stages the stream bytes of its chunks and the
// codon lookup in LDS.  Four passes over the chunks, two O(chunks + sequences) scans on the host between them:
//   summaries   per stream frame (position mod 3): codons before the first break, after the last, and whether there is one
//   (host)      the length of the run that enters every chunk, and how far the run that leaves it goes on
//   counts      qualifying ORFs whose first codon lies in the chunk and their residues; the same at every sentinel
//   (host)      prefix sums: the output slot of every chunk's first ORF, and of every sequence's first ORF of a strand
//   heads       records, residues and the closing sentinel of the ORFs that start in the chunk (as far as the chunk goes)
//   tails       the residues of the runs that entered the chunk
// Nothing depends on the order in which lanes or blocks run: every output byte has one writer.
#include "p7x_translate.hpp"
#include "p7x_device.hpp"
#include "p7x_launch.hpp"
#include "p7x.h"
#include <algorithm>
#include <chrono>
#include <cstring>

namespace p7x {
namespace {

constexpr int kOrfThreads = 128;                       // chunks per block
constexpr int kTabBytes = kCodonLut + kNtKp;           // lookup, then the complement map
constexpr int kStreamAt = (kTabBytes + 15) / 16 * 16;  // where the staged stream starts in LDS

enum { ORF_SUMMARY = 0, ORF_COUNT = 1, ORF_HEADS = 2, ORF_TAILS = 3 };

struct OrfArgs {
  const uint8_t *dsq; int64_t T;            // the packed block: T = residues + sequences + 1 bytes, readable up to a multiple of four
  const uint8_t *tab;                       // [kTabBytes]
  const int64_t *offsets; const int32_t *lengths; int64_t n;
  int32_t crick, C, min_len; int64_t nchunks;
  int32_t *sum;                             // [nchunks][8] summaries: lead[3], tail[3], mask of the frames with a break, 0
  const int64_t *carry, *ext, *src;         // [nchunks][3] per stream frame: codons of the run entering; codons it goes on beyond; the chunk of its head
  int64_t *cc;                              // [nchunks][2] counts: ORFs headed in the chunk, their residues + 1 each
  int64_t *spre;                            // [n + 1][2] the same before the sentinel in front of sequence <slot>, within its chunk
  const int64_t *cbase;                     // [nchunks][2] exclusive prefix of cc along the stream
  const int64_t *adj;                       // [n][2] stream rank / offset -> output rank / offset, per sequence
  int64_t *open_off;                        // [nchunks][3] output offset of the ORF that leaves the chunk open, -1: none that qualifies
  uint8_t *out; int64_t out_bytes, n_orfs;
  int64_t *o_off, *o_src, *o_start, *o_end; int32_t *o_len; int8_t *o_frame;
};

__device__ inline int64_t lower_bound_i64(const int64_t *a, int64_t n, int64_t v)      // first index with a[i] >= v
{
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}

// the amino acid of the codon at LDS position i of the staged stream, -1 for a stop or a codon that touches a sentinel
__device__ inline int codon_at(const uint8_t *lut, const uint8_t *s, int i)
{
  const unsigned b0 = s[i], b1 = s[i + 1], b2 = s[i + 2];
  if (b0 >= (unsigned) kNtKp || b1 >= (unsigned) kNtKp || b2 >= (unsigned) kNtKp) return -1;
  const int aa = lut[(b0 * kNtKp + b1) * kNtKp + b2] & kLutAmino;
  return aa == kAaStop ? -1 : aa;
}

template <int MODE> __global__ __launch_bounds__(kOrfThreads) void orf_kernel(OrfArgs a)
{
  extern __shared__ __align__(16) uint8_t lds[];
  const uint8_t *lut = lds, *comp = lds + kCodonLut;
  uint8_t *s = lds + kStreamAt;
  const int tid = threadIdx.x;
  for (int i = tid; i < kTabBytes; i += kOrfThreads) lds[i] = a.tab[i];
  __syncthreads();
  // the stream positions [tb, tb + nbytes) of this block's chunks and two more for the last codons; 255 beyond the end
  const int64_t tb = (int64_t) blockIdx.x * kOrfThreads * a.C;
  const int nbytes = kOrfThreads * a.C + 2;
  const int64_t live = a.T - tb < nbytes ? a.T - tb : nbytes;        // positions of them that exist (> 0: the grid covers T)
  for (int i = (int) live + tid; i < nbytes; i += kOrfThreads) s[i] = 255;
  {
    // as aligned dwords of the packed array: its positions [plo, phi) are the live stream positions
    const int64_t plo = a.crick ? a.T - tb - live : tb, phi = plo + live;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(a.dsq);
    for (int64_t w = (plo >> 2) + tid; w <= ((phi - 1) >> 2); w += kOrfThreads) {
      const uint32_t d = words[w];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t p = 4 * w + j;
        if (p < plo || p >= phi) continue;
        uint8_t v = (uint8_t) (d >> (8 * j));
        if (a.crick && v < kNtKp) v = comp[v];
        s[a.crick ? a.T - 1 - p - tb : p - tb] = v;
      }
    }
  }
  __syncthreads();

  const int64_t g = (int64_t) blockIdx.x * kOrfThreads + tid;
  if (g >= a.nchunks) return;
  const int lo = tid * a.C, hi = lo + a.C;
  const int64_t t0 = tb + lo;
  const int ph0 = (int) (t0 % 3);               // slot j of this lane (positions lo + j, lo + j + 3, ...) is stream frame (ph0 + j) mod 3
  int fr[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) fr[j] = (ph0 + j) % 3;

  if (MODE == ORF_SUMMARY) {
    int run[3] = { 0, 0, 0 }, lead[3] = { 0, 0, 0 };
    bool has[3] = { false, false, false };
    for (int i = lo; i < hi; i += 3) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (i + j >= hi) break;
        if (codon_at(lut, s, i + j) >= 0) { ++run[j]; continue; }
        if (!has[j]) { lead[j] = run[j]; has[j] = true; }
        run[j] = 0;
      }
    }
    int32_t *o = a.sum + g * 8;
    int mask = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      o[fr[j]] = has[j] ? lead[j] : run[j];
      o[3 + fr[j]] = run[j];
      if (has[j]) mask |= 1 << fr[j];
    }
    o[6] = mask; o[7] = 0;
    return;
  }

  if (MODE == ORF_TAILS) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int64_t c = a.carry[g * 3 + fr[j]], sc = a.src[g * 3 + fr[j]];
      if (c <= 0 || sc < 0 || sc >= a.nchunks) continue;
      const int64_t off = a.open_off[sc * 3 + fr[j]];
      if (off < 0) continue;
      int64_t w = off + c;
      for (int i = lo + j; i < hi; i += 3, ++w) {
        const int aa = codon_at(lut, s, i);
        if (aa < 0) break;
        if (w < a.out_bytes) a.out[w] = (uint8_t) aa;
      }
    }
    return;
  }

  // counts and heads: the same walk
  bool in_run[3];
  int64_t wpos[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) { in_run[j] = a.carry[g * 3 + fr[j]] > 0; wpos[j] = -1; }
  int64_t cnt = 0, res = 0;
  for (int i = lo; i < hi; i += 3) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int ii = i + j;
      if (ii >= hi) break;
      const int64_t t = t0 + (ii - lo);
      if (MODE == ORF_COUNT && s[ii] == 255 && t < a.T) {
        const int64_t slot = lower_bound_i64(a.offsets, a.n, (a.crick ? a.T - 1 - t : t) + 1);
        a.spre[slot * 2] = cnt; a.spre[slot * 2 + 1] = res;
      }
      const int aa = codon_at(lut, s, ii);
      if (aa < 0) { in_run[j] = false; wpos[j] = -1; continue; }
      if (!in_run[j]) {
        in_run[j] = true;
        int64_t len = 1;
        int u = ii + 3;
        while (u < hi && codon_at(lut, s, u) >= 0) { ++len; u += 3; }
        const bool open = u >= hi;
        if (open) len += a.ext[g * 3 + fr[j]];
        if (len >= a.min_len) {
          if (MODE == ORF_HEADS) {
            const int64_t pos = a.crick ? a.T - 1 - t : t;
            const int64_t sq = lower_bound_i64(a.offsets, a.n, pos + 1) - 1;        // the last sequence that starts at or before pos
            if (sq >= 0) {
              const int64_t o = a.offsets[sq], L = a.lengths[sq];
              const int64_t rank = a.cbase[g * 2] + cnt + a.adj[sq * 2], off = a.cbase[g * 2 + 1] + res + a.adj[sq * 2 + 1];
              if (rank >= 0 && rank < a.n_orfs) {
                a.o_off[rank] = off; a.o_len[rank] = (int32_t) len; a.o_src[rank] = sq;
                const int64_t start = pos - o + 1;
                if (!a.crick) { a.o_frame[rank] = (int8_t) ((pos - o) % 3 + 1); a.o_start[rank] = start; a.o_end[rank] = start + 3 * len - 1; }
                else { a.o_frame[rank] = (int8_t) -((o + L - pos - 1) % 3 + 1); a.o_start[rank] = start; a.o_end[rank] = start - 3 * len + 1; }
              }
              if (off >= 1 && off + len < a.out_bytes) { a.out[off + len] = 255; wpos[j] = off; if (open) a.open_off[g * 3 + fr[j]] = off; }
            }
          }
          ++cnt; res += len + 1;
        }
      }
      if (MODE == ORF_HEADS && wpos[j] >= 0) { if (wpos[j] < a.out_bytes) a.out[wpos[j]] = (uint8_t) aa; ++wpos[j]; }
    }
  }
  if (MODE == ORF_COUNT) { a.cc[g * 2] = cnt; a.cc[g * 2 + 1] = res; }
}

struct XlatArgs {
  const uint8_t *dsq; const uint8_t *tab;
  const int64_t *in_off, *out_off; const int32_t *out_len; int64_t n;
  uint8_t *out; int64_t out_bytes;
  unsigned long long *err;                  // lowest packed position of a codon that cannot be translated
};

__global__ __launch_bounds__(256) void translate_kernel(XlatArgs a)
{
  __shared__ uint8_t lut[kCodonLut];
  for (int i = threadIdx.x; i < kCodonLut; i += 256) lut[i] = a.tab[i];
  __syncthreads();
  for (int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x; j < a.out_bytes; j += (int64_t) gridDim.x * 256) {
    uint8_t v = 255;
    const int64_t sq = lower_bound_i64(a.out_off, a.n, j + 1) - 1;
    if (sq >= 0) {
      const int64_t k = j - a.out_off[sq];
      if (k < a.out_len[sq]) {
        const int64_t p = a.in_off[sq] + 3 * k;
        const unsigned b0 = a.dsq[p], b1 = a.dsq[p + 1], b2 = a.dsq[p + 2];
        v = kAaX | kLutUntranslatable;
        if (b0 < (unsigned) kNtKp && b1 < (unsigned) kNtKp && b2 < (unsigned) kNtKp) v = lut[(b0 * kNtKp + b1) * kNtKp + b2];
        if (v & kLutUntranslatable) atomicMin(a.err, (unsigned long long) p);      // a minimum: the order does not matter
        v &= kLutAmino;
      }
    }
    a.out[j] = v;
  }
}

struct TranslateSet {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = { nullptr, nullptr };
  DeviceBuf in, work, out;
  // The end of a lease: everything belongs to one call and can be gigabytes, so it goes back to the slab pool.
  void on_return()
  {
    if (stream) (void) hipStreamSynchronize(stream);
    in.reset(); work.reset(); out.reset();
  }
};

// a device workspace cut into arrays: every array starts on a multiple of 16 bytes
struct Carver {
  size_t at = 0;
  size_t take(size_t bytes) { const size_t o = at; at += (bytes + 15) / 16 * 16; return o; }
};

int64_t device_budget(DeviceCtx *ctx)
{
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return -1;
  std::lock_guard<std::mutex> lk(ctx->slab_mu);
  return (int64_t) (free_b / 10 * 9 + ctx->slab_free_bytes);
}

int over_budget(const char *what, int64_t need, int64_t budget)
{
  if (budget < 0 || need <= budget) return P7X_OK;
  set_error(std::string(what) + ": " + std::to_string(need) + " bytes of device memory, " + std::to_string(budget) + " available: translate fewer sequences per call");
  return P7X_EMEM;
}

double us_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }

template <int MODE> int launch_orf(const OrfArgs &a, hipStream_t stream, hipEvent_t e0, hipEvent_t e1)
{
  const size_t lds = (size_t) kStreamAt + (size_t) kOrfThreads * (size_t) a.C + 2;
  int st = kernel_grant_lds(orf_kernel<MODE>, lds);
  if (st != P7X_OK) return st;
  const unsigned blocks = (unsigned) ((a.nchunks + kOrfThreads - 1) / kOrfThreads);
  P7X_HIP(hipEventRecord(e0, stream));
  hipLaunchKernelGGL(orf_kernel<MODE>, dim3(blocks), dim3(kOrfThreads), lds, stream, a);
  P7X_HIP(hipGetLastError());
  P7X_HIP(hipEventRecord(e1, stream));
  return P7X_OK;
}

} // namespace

int orfs_find_device(const GeneticCodeTable &gc, int device, const PackedView &in, int32_t min_length, int strands, p7x_orfs &out)
{
  out = p7x_orfs();
  out.on_device = 1;
  orf_plan(in.nres, in.n, &out.chunk, &out.chunks);
  DeviceCtx *ctx = nullptr;
  int st = get_ctx(device, &ctx);
  if (st != P7X_OK) return st;
  P7X_HIP(hipSetDevice(ctx->device));
  const int64_t T = in.nres + in.n + 1, n = in.n, nchunks = out.chunks;
  const int C = out.chunk;
  if (nchunks > (int64_t) 0x7fffffff * kOrfThreads) { set_error("translate_orfs: too many chunks for one launch"); return P7X_EINVAL; }
  const bool do_strand[2] = { strands != P7X_STRAND_BOTTOMONLY, strands != P7X_STRAND_TOPONLY };

  auto lease = LeasePool<TranslateSet>::instance().lease(ctx->device, [](const TranslateSet &, const TranslateSet *b) { return !b; });
  TranslateSet &set = *lease;
  if (!set.stream) P7X_HIP(hipStreamCreateWithFlags(&set.stream, hipStreamNonBlocking));
  for (auto &e : set.ev) if (!e) P7X_HIP(hipEventCreate(&e));
  hipStream_t q = set.stream;

  // input: the block, the tables, offsets and lengths
  Carver ci;
  const size_t i_dsq = ci.take((size_t) T + 4), i_tab = ci.take(kTabBytes), i_off = ci.take(sizeof(int64_t) * (size_t) n), i_len = ci.take(sizeof(int32_t) * (size_t) n);
  // per strand: summaries, carry / ext / src, counts (then their prefix), sentinel counts, adjustments, open offsets
  Carver cw;
  size_t w_sum[2], w_carry[2], w_ext[2], w_src[2], w_cc[2], w_spre[2], w_adj[2], w_open[2];
  for (int k = 0; k < 2; ++k) {
    w_sum[k] = cw.take(32 * (size_t) nchunks); w_carry[k] = cw.take(24 * (size_t) nchunks); w_ext[k] = cw.take(24 * (size_t) nchunks);
    w_src[k] = cw.take(24 * (size_t) nchunks); w_cc[k] = cw.take(16 * (size_t) nchunks); w_spre[k] = cw.take(16 * (size_t) (n + 1));
    w_adj[k] = cw.take(16 * (size_t) n + 16); w_open[k] = cw.take(24 * (size_t) nchunks);
  }
  const int64_t budget = device_budget(ctx);
  if ((st = over_budget("translate_orfs workspace", (int64_t) (ci.at + cw.at), budget)) != P7X_OK) return st;
  if ((st = set.in.reserve(ctx, ci.at)) != P7X_OK) return st;
  if ((st = set.work.reserve(ctx, cw.at)) != P7X_OK) return st;
  uint8_t *d_in = set.in.as<uint8_t>(), *d_w = set.work.as<uint8_t>();

  uint8_t tab[kTabBytes];
  std::memcpy(tab, gc.lut, kCodonLut);
  std::memcpy(tab + kCodonLut, kNtComplement, kNtKp);
  P7X_HIP(hipMemsetAsync(d_in + i_dsq + (size_t) T, 255, 4, q));
  P7X_HIP(hipMemcpyAsync(d_in + i_dsq, in.dsq, (size_t) T, hipMemcpyHostToDevice, q));
  P7X_HIP(hipMemcpyAsync(d_in + i_tab, tab, kTabBytes, hipMemcpyHostToDevice, q));
  if (n) {
    P7X_HIP(hipMemcpyAsync(d_in + i_off, in.offsets, sizeof(int64_t) * (size_t) n, hipMemcpyHostToDevice, q));
    P7X_HIP(hipMemcpyAsync(d_in + i_len, in.lengths, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, q));
  }
  P7X_HIP(hipStreamSynchronize(q));         // <tab> is on this frame

  OrfArgs base{};
  base.dsq = d_in + i_dsq; base.T = T; base.tab = d_in + i_tab;
  base.offsets = reinterpret_cast<const int64_t *>(d_in + i_off); base.lengths = reinterpret_cast<const int32_t *>(d_in + i_len); base.n = n;
  base.C = C; base.min_len = min_length; base.nchunks = nchunks;
  OrfArgs arg[2];
  for (int k = 0; k < 2; ++k) {
    OrfArgs &a = arg[k];
    a = base; a.crick = k;
    a.sum = reinterpret_cast<int32_t *>(d_w + w_sum[k]);
    a.carry = reinterpret_cast<const int64_t *>(d_w + w_carry[k]); a.ext = reinterpret_cast<const int64_t *>(d_w + w_ext[k]);
    a.src = reinterpret_cast<const int64_t *>(d_w + w_src[k]);
    a.cc = reinterpret_cast<int64_t *>(d_w + w_cc[k]); a.cbase = a.cc;
    a.spre = reinterpret_cast<int64_t *>(d_w + w_spre[k]);
    a.adj = reinterpret_cast<const int64_t *>(d_w + w_adj[k]);
    a.open_off = reinterpret_cast<int64_t *>(d_w + w_open[k]);
  }
  auto timed = [&](int pass) { float ms = 0.0f; if (hipEventElapsedTime(&ms, set.ev[0], set.ev[1]) == hipSuccess) out.pass_us[pass] += (double) ms * 1000.0; };

  // pass 1: summaries
  std::vector<int32_t> h_sum[2];
  for (int k = 0; k < 2; ++k) {
    if (!do_strand[k]) continue;
    if ((st = launch_orf<ORF_SUMMARY>(arg[k], q, set.ev[0], set.ev[1])) != P7X_OK) return st;
    h_sum[k].resize(8 * (size_t) nchunks);
    P7X_HIP(hipMemcpyAsync(h_sum[k].data(), arg[k].sum, 32 * (size_t) nchunks, hipMemcpyDeviceToHost, q));
    P7X_HIP(hipStreamSynchronize(q));
    timed(0);
  }
  // scan 1: what enters and what leaves every chunk, per stream frame
  auto t_host = std::chrono::steady_clock::now();
  std::vector<int64_t> h_carry[2], h_ext[2], h_src[2];
  for (int k = 0; k < 2; ++k) {
    if (!do_strand[k]) continue;
    const int32_t *sm = h_sum[k].data();
    h_carry[k].assign(3 * (size_t) nchunks, 0); h_ext[k].assign(3 * (size_t) nchunks, 0); h_src[k].assign(3 * (size_t) nchunks, -1);
    for (int f = 0; f < 3; ++f) {
      for (int64_t g = 1; g < nchunks; ++g) {
        const int32_t *p = sm + (g - 1) * 8;
        const bool has = p[6] >> f & 1;
        const int64_t c = has ? p[3 + f] : h_carry[k][3 * (g - 1) + f] + p[f];
        h_carry[k][3 * g + f] = c;
        if (c > 0) h_src[k][3 * g + f] = (has || h_carry[k][3 * (g - 1) + f] == 0) ? g - 1 : h_src[k][3 * (g - 1) + f];
      }
      for (int64_t g = nchunks - 2; g >= 0; --g) {
        const int32_t *p = sm + (g + 1) * 8;
        h_ext[k][3 * g + f] = (p[6] >> f & 1) ? p[f] : p[f] + h_ext[k][3 * (g + 1) + f];
      }
    }
  }
  out.stitch_us += us_since(t_host);
  // pass 2: counts
  std::vector<int64_t> h_cc[2], h_spre[2];
  for (int k = 0; k < 2; ++k) {
    if (!do_strand[k]) continue;
    P7X_HIP(hipMemcpyAsync(d_w + w_carry[k], h_carry[k].data(), 24 * (size_t) nchunks, hipMemcpyHostToDevice, q));
    P7X_HIP(hipMemcpyAsync(d_w + w_ext[k], h_ext[k].data(), 24 * (size_t) nchunks, hipMemcpyHostToDevice, q));
    P7X_HIP(hipMemcpyAsync(d_w + w_src[k], h_src[k].data(), 24 * (size_t) nchunks, hipMemcpyHostToDevice, q));
    if ((st = launch_orf<ORF_COUNT>(arg[k], q, set.ev[0], set.ev[1])) != P7X_OK) return st;
    h_cc[k].resize(2 * (size_t) nchunks); h_spre[k].resize(2 * (size_t) (n + 1));
    P7X_HIP(hipMemcpyAsync(h_cc[k].data(), arg[k].cc, 16 * (size_t) nchunks, hipMemcpyDeviceToHost, q));
    P7X_HIP(hipMemcpyAsync(h_spre[k].data(), arg[k].spre, 16 * (size_t) (n + 1), hipMemcpyDeviceToHost, q));
    P7X_HIP(hipStreamSynchronize(q));
    timed(1);
  }
  // scan 2: output slots.  Along a stream, P[slot] counts what lies before the sentinel in front of sequence <slot> (slot n:
  // the last sentinel); watson passes the sequences upwards, crick downwards, and the output takes a sequence's watson
  // ORFs, then its crick ORFs.
  t_host = std::chrono::steady_clock::now();
  std::vector<int64_t> h_adj[2];
  int64_t totals[2][2] = { { 0, 0 }, { 0, 0 } };
  for (int k = 0; k < 2; ++k) {
    if (!do_strand[k]) continue;
    int64_t rc = 0, rr = 0;
    for (int64_t g = 0; g < nchunks; ++g) {
      const int64_t c = h_cc[k][2 * g], r = h_cc[k][2 * g + 1];
      if (c < 0 || r < 0) { set_error("translate_orfs: the device's counts are not counts"); return P7X_EDEVICE; }
      h_cc[k][2 * g] = rc; h_cc[k][2 * g + 1] = rr; rc += c; rr += r;
    }
    totals[k][0] = rc; totals[k][1] = rr;
    for (int64_t slot = 0; slot <= n; ++slot) {
      const int64_t pos = slot < n ? in.offsets[slot] - 1 : T - 1, g = (k ? T - 1 - pos : pos) / C;
      h_spre[k][2 * slot] += h_cc[k][2 * g]; h_spre[k][2 * slot + 1] += h_cc[k][2 * g + 1];
    }
    h_adj[k].assign(2 * (size_t) n + 2, 0);
  }
  int64_t R = 0, Q = 1;
  for (int64_t s = 0; s < n; ++s) {
    if (do_strand[0]) {
      const int64_t *P = h_spre[0].data();
      h_adj[0][2 * s] = R - P[2 * s]; h_adj[0][2 * s + 1] = Q - P[2 * s + 1];
      R += P[2 * (s + 1)] - P[2 * s]; Q += P[2 * (s + 1) + 1] - P[2 * s + 1];
    }
    if (do_strand[1]) {
      const int64_t *P = h_spre[1].data();
      h_adj[1][2 * s] = R - P[2 * (s + 1)]; h_adj[1][2 * s + 1] = Q - P[2 * (s + 1) + 1];
      R += P[2 * s] - P[2 * (s + 1)]; Q += P[2 * s + 1] - P[2 * (s + 1) + 1];
    }
  }
  out.stitch_us += us_since(t_host);
  if (R != totals[0][0] + totals[1][0] || Q != 1 + totals[0][1] + totals[1][1] || R < 0 || Q < 1 + R) {
    set_error("translate_orfs: the counts at the sentinels and in the chunks do not agree");
    return P7X_EDEVICE;
  }
  const int64_t n_orfs = R, out_bytes = Q;
  if (n_orfs > 0x7fffffff) { set_error("translate_orfs: more than 2^31 ORFs in one call; raise min_length or translate fewer sequences"); return P7X_ERANGE; }

  // output: residues, then the records
  Carver co;
  const size_t o_dsq = co.take((size_t) out_bytes), o_off = co.take(8 * (size_t) n_orfs), o_src = co.take(8 * (size_t) n_orfs), o_start = co.take(8 * (size_t) n_orfs),
               o_end = co.take(8 * (size_t) n_orfs), o_len = co.take(4 * (size_t) n_orfs), o_frame = co.take((size_t) n_orfs);
  if ((st = over_budget("translate_orfs output", (int64_t) (ci.at + cw.at + co.at), budget)) != P7X_OK) return st;
  if ((st = set.out.reserve(ctx, co.at)) != P7X_OK) return st;
  uint8_t *d_o = set.out.as<uint8_t>();
  P7X_HIP(hipMemsetAsync(d_o + o_dsq, 255, 1, q));
  for (int k = 0; k < 2; ++k) {
    if (!do_strand[k]) continue;
    OrfArgs &a = arg[k];
    a.out = d_o + o_dsq; a.out_bytes = out_bytes; a.n_orfs = n_orfs;
    a.o_off = reinterpret_cast<int64_t *>(d_o + o_off); a.o_src = reinterpret_cast<int64_t *>(d_o + o_src);
    a.o_start = reinterpret_cast<int64_t *>(d_o + o_start); a.o_end = reinterpret_cast<int64_t *>(d_o + o_end);
    a.o_len = reinterpret_cast<int32_t *>(d_o + o_len); a.o_frame = reinterpret_cast<int8_t *>(d_o + o_frame);
    P7X_HIP(hipMemcpyAsync(d_w + w_cc[k], h_cc[k].data(), 16 * (size_t) nchunks, hipMemcpyHostToDevice, q));
    P7X_HIP(hipMemcpyAsync(d_w + w_adj[k], h_adj[k].data(), 16 * (size_t) n + 16, hipMemcpyHostToDevice, q));
    P7X_HIP(hipMemsetAsync(d_w + w_open[k], 0xff, 24 * (size_t) nchunks, q));
    if ((st = launch_orf<ORF_HEADS>(a, q, set.ev[0], set.ev[1])) != P7X_OK) return st;
    P7X_HIP(hipStreamSynchronize(q));
    timed(2);
    if ((st = launch_orf<ORF_TAILS>(a, q, set.ev[0], set.ev[1])) != P7X_OK) return st;
    P7X_HIP(hipStreamSynchronize(q));
    timed(3);
  }
  out.n = n_orfs; out.nres = out_bytes - 1 - n_orfs;
  out.dsq.resize((size_t) out_bytes); out.offsets.resize((size_t) n_orfs); out.source.resize((size_t) n_orfs); out.start.resize((size_t) n_orfs);
  out.end.resize((size_t) n_orfs); out.lengths.resize((size_t) n_orfs); out.frame.resize((size_t) n_orfs);
  P7X_HIP(hipMemcpyAsync(out.dsq.data(), d_o + o_dsq, (size_t) out_bytes, hipMemcpyDeviceToHost, q));
  if (n_orfs) {
    P7X_HIP(hipMemcpyAsync(out.offsets.data(), d_o + o_off, 8 * (size_t) n_orfs, hipMemcpyDeviceToHost, q));
    P7X_HIP(hipMemcpyAsync(out.source.data(), d_o + o_src, 8 * (size_t) n_orfs, hipMemcpyDeviceToHost, q));
    P7X_HIP(hipMemcpyAsync(out.start.data(), d_o + o_start, 8 * (size_t) n_orfs, hipMemcpyDeviceToHost, q));
    P7X_HIP(hipMemcpyAsync(out.end.data(), d_o + o_end, 8 * (size_t) n_orfs, hipMemcpyDeviceToHost, q));
    P7X_HIP(hipMemcpyAsync(out.lengths.data(), d_o + o_len, 4 * (size_t) n_orfs, hipMemcpyDeviceToHost, q));
    P7X_HIP(hipMemcpyAsync(out.frame.data(), d_o + o_frame, (size_t) n_orfs, hipMemcpyDeviceToHost, q));
  }
  P7X_HIP(hipStreamSynchronize(q));
  return P7X_OK;
}

int translate_block_device(const GeneticCodeTable &gc, int device, const PackedView &in, uint8_t *out_dsq, int64_t *out_offsets,
                           int32_t *out_lengths, int64_t *err_seq, int64_t *err_pos)
{
  DeviceCtx *ctx = nullptr;
  int st = get_ctx(device, &ctx);
  if (st != P7X_OK) return st;
  if ((st = translate_block_lengths(in, err_seq, err_pos)) != P7X_OK) return st;
  P7X_HIP(hipSetDevice(ctx->device));
  const int64_t T = in.nres + in.n + 1, n = in.n, out_bytes = in.nres / 3 + n + 1;
  int64_t pos = 1;
  for (int64_t s = 0; s < n; ++s) { out_offsets[s] = pos; out_lengths[s] = in.lengths[s] / 3; pos += in.lengths[s] / 3 + 1; }
  auto lease = LeasePool<TranslateSet>::instance().lease(ctx->device, [](const TranslateSet &, const TranslateSet *b) { return !b; });
  TranslateSet &set = *lease;
  if (!set.stream) P7X_HIP(hipStreamCreateWithFlags(&set.stream, hipStreamNonBlocking));
  hipStream_t q = set.stream;
  Carver ci;
  const size_t i_dsq = ci.take((size_t) T), i_tab = ci.take(kCodonLut), i_off = ci.take(8 * (size_t) n), i_ooff = ci.take(8 * (size_t) n),
               i_olen = ci.take(4 * (size_t) n), i_err = ci.take(8);
  if ((st = over_budget("translate workspace", (int64_t) ci.at + out_bytes, device_budget(ctx))) != P7X_OK) return st;
  if ((st = set.in.reserve(ctx, ci.at)) != P7X_OK) return st;
  if ((st = set.out.reserve(ctx, (size_t) out_bytes)) != P7X_OK) return st;
  uint8_t *d_in = set.in.as<uint8_t>();
  P7X_HIP(hipMemcpyAsync(d_in + i_dsq, in.dsq, (size_t) T, hipMemcpyHostToDevice, q));
  P7X_HIP(hipMemcpyAsync(d_in + i_tab, gc.lut, kCodonLut, hipMemcpyHostToDevice, q));
  if (n) {
    P7X_HIP(hipMemcpyAsync(d_in + i_off, in.offsets, 8 * (size_t) n, hipMemcpyHostToDevice, q));
    P7X_HIP(hipMemcpyAsync(d_in + i_ooff, out_offsets, 8 * (size_t) n, hipMemcpyHostToDevice, q));
    P7X_HIP(hipMemcpyAsync(d_in + i_olen, out_lengths, 4 * (size_t) n, hipMemcpyHostToDevice, q));
  }
  P7X_HIP(hipMemsetAsync(d_in + i_err, 0xff, 8, q));
  XlatArgs a{};
  a.dsq = d_in + i_dsq; a.tab = d_in + i_tab; a.in_off = reinterpret_cast<const int64_t *>(d_in + i_off);
  a.out_off = reinterpret_cast<const int64_t *>(d_in + i_ooff); a.out_len = reinterpret_cast<const int32_t *>(d_in + i_olen); a.n = n;
  a.out = set.out.as<uint8_t>(); a.out_bytes = out_bytes; a.err = reinterpret_cast<unsigned long long *>(d_in + i_err);
  const int64_t want = (out_bytes + 255) / 256, cap = (int64_t) ctx->num_cu * 16;
  hipLaunchKernelGGL(translate_kernel, dim3((unsigned) std::max<int64_t>(1, std::min(want, cap))), dim3(256), 0, q, a);
  P7X_HIP(hipGetLastError());
  unsigned long long bad = 0;
  P7X_HIP(hipMemcpyAsync(&bad, a.err, 8, hipMemcpyDeviceToHost, q));
  P7X_HIP(hipMemcpyAsync(out_dsq, a.out, (size_t) out_bytes, hipMemcpyDeviceToHost, q));
  P7X_HIP(hipStreamSynchronize(q));
  if (bad != ~0ull) {
    const int64_t s = (int64_t) (std::upper_bound(in.offsets, in.offsets + n, (int64_t) bad) - in.offsets) - 1;
    if (err_seq) *err_seq = s;
    if (err_pos) *err_pos = (int64_t) bad - in.offsets[s];
    set_error("Failed to translate codon at index " + std::to_string((int64_t) bad - in.offsets[s]) + " of sequence " + std::to_string(s));
    return P7X_EINVAL;
  }
  return P7X_OK;
}

} // namespace p7x

using namespace p7x;

// the checks of both ORF entry points, then the twin or the device
static int orfs_entry(int32_t table, int device, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, size_t n, int64_t nres,
                      int32_t min_length, int strands, bool host, int threads, p7x_orfs **out)
{
  if (!out) { set_error("p7x_orfs_find: bad arguments"); return P7X_EINVAL; }
  const GeneticCodeTable *gc = genetic_code(table);
  if (!gc) return P7X_EINVAL;
  if (min_length < 1) { set_error("min_length must be at least 1"); return P7X_EINVAL; }
  if (strands != P7X_STRAND_BOTH && strands != P7X_STRAND_TOPONLY && strands != P7X_STRAND_BOTTOMONLY) { set_error("p7x_orfs_find: bad strands"); return P7X_EINVAL; }
  const PackedView in{ dsq, offsets, lengths, (int64_t) n, nres };
  int st = check_packing(in);
  if (st != P7X_OK) return st;
  auto *o = new p7x_orfs();
  st = host ? orfs_find_host(*gc, in, min_length, strands, threads, *o) : orfs_find_device(*gc, device, in, min_length, strands, *o);
  if (st != P7X_OK) { delete o; return st; }
  *out = o;
  return P7X_OK;
}

extern "C" {

int p7x_orfs_find(int32_t table, int device, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, size_t n, int64_t nres,
                  int32_t min_length, int strands, p7x_orfs **out)
{
  return orfs_entry(table, device, dsq, offsets, lengths, n, nres, min_length, strands, debug_opt(OPT_HOST_TRANSLATE) > 0, 0, out);
}

int p7x_orfs_find_host(int32_t table, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, size_t n, int64_t nres,
                       int32_t min_length, int strands, int threads, p7x_orfs **out)
{
  return orfs_entry(table, -1, dsq, offsets, lengths, n, nres, min_length, strands, true, threads, out);
}

int p7x_translate_block(int32_t table, int device, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, size_t n, int64_t nres,
                        uint8_t *out_dsq, int64_t *out_offsets, int32_t *out_lengths, int64_t *err_seq, int64_t *err_pos)
{
  const GeneticCodeTable *gc = genetic_code(table);
  if (!gc) return P7X_EINVAL;
  if (!out_dsq || (n && (!out_offsets || !out_lengths))) { set_error("p7x_translate_block: bad arguments"); return P7X_EINVAL; }
  if (err_seq) *err_seq = -1;
  if (err_pos) *err_pos = -1;
  const PackedView in{ dsq, offsets, lengths, (int64_t) n, nres };
  const int st = check_packing(in);
  if (st != P7X_OK) return st;
  if (debug_opt(OPT_HOST_TRANSLATE) > 0) return translate_block_host(*gc, in, out_dsq, out_offsets, out_lengths, err_seq, err_pos);
  return translate_block_device(*gc, device, in, out_dsq, out_offsets, out_lengths, err_seq, err_pos);
}

} // extern "C"
