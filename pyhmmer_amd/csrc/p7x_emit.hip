// p7x_emit.hip -- HMM.emit_block: sequences sampled from a core model on the device (gfx950), one lane per sequence.
//
// A lane walks the model with the function its host twin walks it with (emit_walk, p7x_emitwalk.hpp): one Philox block
// per step, a 53-bit deviate, comparisons against the cumulative tables the host built in double.  Nothing else is
// floating point, so the bytes are the twin's.
//
//   pass 1     emit_kernel: sequence i into slot i of <cap> bytes (twice the expected length by default); the length is
//              counted in full even where the slot is full.  A path that emits nothing is drawn again at once (attempt
//              a + 1).  Residues are gathered four to a register and stored as dwords.
//   scan       emit_scan_kernel: exclusive scan of (length + 1), the offsets of the packed block with its sentinels.
//   pass 2     the sequences that outgrew their slot (the host reads the lengths): emit_kernel again over the list, each
//              from the attempt that counted -- the same stream, so the same sequence -- into a slot of its own length.
//   compact    emit_compact_kernel: one wavefront per sequence copies its slot to its place in the packed block.
// Lanes of a wavefront finish at different steps and take different branches at every step: the kernel is bound by the
// latency of the dependent table reads and by divergence, not by bandwidth.  Tables of up to 40 KiB (four blocks of 256
// lanes per CU keep theirs in the 160 KiB of LDS) are staged in LDS; longer models read theirs through L2, with no LDS
// claim on occupancy.  Option "emit_lds" = 0 reads every table through L2.
#include "p7x_emit.hpp"
#include "p7x_device.hpp"
#include "p7x_host.hpp"
#include "p7x_kernels.hpp"
#include <cstring>

namespace p7x {

constexpr size_t kEmitLdsBytes = 40 * 1024;

struct EmitArgs {
  const double *tab; int M, K; uint32_t key0, key1;
  int64_t n;                        // lanes
  int32_t cap;                      // pass 1: slot capacity, a multiple of four
  const int64_t *idx;               // pass 2: the sequence of lane j          (pass 1: nullptr, lane j is sequence j)
  const int64_t *slot_off;          // pass 2: first byte of its slot, a multiple of four   (pass 1: j * cap)
  const int32_t *slot_cap;          // pass 2: its capacity, a multiple of four
  uint8_t *dsq; int8_t *st; int32_t *node;        // the slots; st, node: nullptr without traces
  int32_t *len, *attempt, *status;  // per sequence; pass 2 starts from attempt[] and writes none of them
  int lds_doubles;                  // doubles of the table to stage in LDS; 0: read it where it is
};

struct SlotSink {
  uint32_t *d32, *s32; int32_t *node; int cap; uint32_t dbuf = 0, sbuf = 0;
  __device__ void put(int pos, int x, int s, int k)
  {
    if (pos >= cap) return;
    const int sh = (pos & 3) * 8;
    dbuf |= (uint32_t) x << sh;
    if (s32) { sbuf |= (uint32_t) s << sh; node[pos] = k; }
    if ((pos & 3) == 3) {
      d32[pos >> 2] = dbuf; dbuf = 0;
      if (s32) { s32[pos >> 2] = sbuf; sbuf = 0; }
    }
  }
  __device__ void flush(int len)
  {
    const int n = len < cap ? len : cap;       // cap is a multiple of four: the last dword of a slot is inside it
    if (n & 3) { d32[n >> 2] = dbuf; if (s32) s32[n >> 2] = sbuf; }
  }
};

__global__ __launch_bounds__(256) void emit_kernel(EmitArgs a)
{
  extern __shared__ double lds_tab[];
  const double *tab = a.tab;
  if (a.lds_doubles > 0) {
    for (int i = (int) threadIdx.x; i < a.lds_doubles; i += (int) blockDim.x) lds_tab[i] = a.tab[i];
    __syncthreads();
    tab = lds_tab;
  }
  const int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.n) return;
  const int64_t seq = a.idx ? a.idx[j] : j;
  const int64_t off = a.slot_off ? a.slot_off[j] : j * (int64_t) a.cap;
  SlotSink sink;
  sink.d32 = reinterpret_cast<uint32_t *>(a.dsq + off);
  sink.s32 = a.st ? reinterpret_cast<uint32_t *>(a.st + off) : nullptr;
  sink.node = a.node ? a.node + off : nullptr;
  sink.cap = a.slot_cap ? a.slot_cap[j] : a.cap;
  int32_t len = 0; uint32_t attempt = 0;
  const int st = emit_walk(tab, a.M, a.K, a.key0, a.key1, (uint64_t) seq, a.idx ? (uint32_t) a.attempt[seq] : 0u, sink, &len, &attempt);
  sink.flush(len);
  if (!a.idx) { a.len[seq] = len; a.attempt[seq] = (int32_t) attempt; a.status[seq] = st; }
}

// off[i] = 1 + sum over t < i of (len[t] + 1); *total = the bytes of the packed block.  One block of 1024 lanes.
__global__ __launch_bounds__(1024) void emit_scan_kernel(const int32_t *len, int64_t n, int64_t *off, int64_t *total)
{
  __shared__ int64_t sh[1024];
  const int tid = (int) threadIdx.x;
  int64_t carry = 1;
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t i = base + tid;
    const int64_t v = i < n ? (int64_t) len[i] + 1 : 0;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const int64_t t = tid >= d ? sh[tid - d] : 0;
      __syncthreads();
      sh[tid] += t;
      __syncthreads();
    }
    if (i < n) off[i] = carry + sh[tid] - v;
    carry += sh[1023];
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

struct CompactArgs {
  int64_t n; int32_t cap;
  const int64_t *idx, *slot_off;    // as EmitArgs: nullptr for the slots of pass 1 (sequences that outgrew theirs are skipped)
  const uint8_t *dsq; const int8_t *st; const int32_t *node;
  const int32_t *len; const int64_t *off;
  uint8_t *out_dsq; int8_t *out_st; int32_t *out_node;
};

__global__ __launch_bounds__(256) void emit_compact_kernel(CompactArgs a)
{
  const int64_t j = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = (int) (threadIdx.x & 63);
  if (j >= a.n) return;
  const int64_t seq = a.idx ? a.idx[j] : j;
  const int32_t L = a.len[seq];
  if (!a.idx && L > a.cap) return;
  const int64_t src = a.slot_off ? a.slot_off[j] : j * (int64_t) a.cap, dst = a.off[seq];
  for (int p = lane; p < L; p += 64) {
    a.out_dsq[dst + p] = a.dsq[src + p];
    if (a.st) { a.out_st[dst + p] = a.st[src + p]; a.out_node[dst + p] = a.node[src + p]; }
  }
  if (lane == 0) {
    a.out_dsq[dst + L] = 255;
    if (a.st) { a.out_st[dst + L] = 0; a.out_node[dst + L] = 0; }
    if (seq == 0) { a.out_dsq[0] = 255; if (a.st) { a.out_st[0] = 0; a.out_node[0] = 0; } }
  }
}

struct EmitSet {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
  DeviceBuf tab, slots, slots_st, slots_node, slots2, slots2_st, slots2_node, per_seq, list, out, out_st, out_node;
  PinnedBuf h_per_seq, h_list;
  // The end of a lease (LeasePool): the slots and the packed block belong to one call and can be gigabytes, so they go back
  // to the slab pool, where the search that follows finds them; the table and the per-sequence arrays are kept.  A call
  // that returned on an error may have left work queued: it finishes first.
  void on_return()
  {
    if (stream) (void) hipStreamSynchronize(stream);
    for (DeviceBuf *b : { &slots, &slots_st, &slots_node, &slots2, &slots2_st, &slots2_node, &out, &out_st, &out_node }) b->reset();
  }
};

static int launch_emit(const EmitArgs &a, size_t lds, hipStream_t stream)
{
  const unsigned blocks = (unsigned) ((a.n + 255) / 256);
  hipLaunchKernelGGL(emit_kernel, dim3(blocks), dim3(256), lds, stream, a);
  P7X_HIP(hipGetLastError());
  return P7X_OK;
}

static int emit_block_device(const p7x_emit_model &em, DeviceCtx *ctx, int64_t n, uint64_t seed, bool traces, p7x_emitted &out)
{
  out = p7x_emitted();
  out.n = n; out.traces = traces; out.on_device = 1; out.cap = emit_default_cap(em);
  if (n == 0) { out.dsq.assign(1, 255); if (traces) { out.st.assign(1, 0); out.node.assign(1, 0); } return P7X_OK; }
  if (n > (int64_t) 0x7fffffff * 4) { set_error("emit_block: more than 2^33 sequences in one call"); return P7X_EINVAL; }
  P7X_HIP(hipSetDevice(ctx->device));
  const int64_t cap = out.cap;
  auto lease = LeasePool<EmitSet>::instance().lease(ctx->device, [](const EmitSet &, const EmitSet *b) { return !b; });
  EmitSet &set = *lease;
  // nine tenths of the free memory, and what the slab pool has parked (an earlier call's slots among it)
  size_t free_b = 0, total_b = 0;
  int64_t budget = -1, need = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
    std::lock_guard<std::mutex> lk(ctx->slab_mu);
    budget = (int64_t) (free_b / 10 * 9 + ctx->slab_free_bytes);
  }
  int st = emit_workspace_bytes(n, cap, traces, budget, &need);
  if (st != P7X_OK) return st;
  if (!set.stream) P7X_HIP(hipStreamCreateWithFlags(&set.stream, hipStreamNonBlocking));
  for (auto &e : set.ev) if (!e) P7X_HIP(hipEventCreate(&e));

  const size_t tab_bytes = em.tab.size() * sizeof(double), slot_bytes = (size_t) n * (size_t) cap;
  // per sequence: len, attempt, status (int32 each), then the offsets (int64), then the scan's total
  const size_t o_len = 0, o_att = sizeof(int32_t) * (size_t) n, o_sta = 2 * o_att, o_off = (3 * o_att + 7) / 8 * 8,
               o_tot = o_off + sizeof(int64_t) * (size_t) n, per_seq_bytes = o_tot + sizeof(int64_t);
  if ((st = set.tab.reserve(ctx, tab_bytes)) != P7X_OK) return st;
  if ((st = set.slots.reserve(ctx, slot_bytes)) != P7X_OK) return st;
  if (traces) {
    if ((st = set.slots_st.reserve(ctx, slot_bytes)) != P7X_OK) return st;
    if ((st = set.slots_node.reserve(ctx, slot_bytes * sizeof(int32_t))) != P7X_OK) return st;
  }
  if ((st = set.per_seq.reserve(ctx, per_seq_bytes)) != P7X_OK) return st;
  if ((st = set.h_per_seq.reserve(per_seq_bytes)) != P7X_OK) return st;
  unsigned char *d_ps = set.per_seq.as<unsigned char>(), *h_ps = set.h_per_seq.as<unsigned char>();

  EmitArgs a{};
  a.tab = set.tab.as<double>(); a.M = em.M; a.K = em.K; a.key0 = (uint32_t) seed; a.key1 = (uint32_t) (seed >> 32);
  a.n = n; a.cap = (int32_t) cap;
  a.dsq = set.slots.as<uint8_t>(); a.st = traces ? set.slots_st.as<int8_t>() : nullptr; a.node = traces ? set.slots_node.as<int32_t>() : nullptr;
  a.len = reinterpret_cast<int32_t *>(d_ps + o_len); a.attempt = reinterpret_cast<int32_t *>(d_ps + o_att); a.status = reinterpret_cast<int32_t *>(d_ps + o_sta);
  const bool use_lds = debug_opt(OPT_EMIT_LDS) != 0 && tab_bytes <= kEmitLdsBytes;
  a.lds_doubles = use_lds ? (int) em.tab.size() : 0;
  const size_t lds = use_lds ? tab_bytes : 0;
  int64_t *d_off = reinterpret_cast<int64_t *>(d_ps + o_off), *d_tot = reinterpret_cast<int64_t *>(d_ps + o_tot);

  P7X_HIP(hipMemcpyAsync(set.tab.as<double>(), em.tab.data(), tab_bytes, hipMemcpyHostToDevice, set.stream));
  P7X_HIP(hipEventRecord(set.ev[0], set.stream));
  if ((st = launch_emit(a, lds, set.stream)) != P7X_OK) return st;
  P7X_HIP(hipEventRecord(set.ev[1], set.stream));
  hipLaunchKernelGGL(emit_scan_kernel, dim3(1), dim3(1024), 0, set.stream, a.len, n, d_off, d_tot);
  P7X_HIP(hipGetLastError());
  P7X_HIP(hipMemcpyAsync(h_ps, d_ps, per_seq_bytes, hipMemcpyDeviceToHost, set.stream));
  P7X_HIP(hipStreamSynchronize(set.stream));

  const int32_t *h_len = reinterpret_cast<const int32_t *>(h_ps + o_len), *h_att = reinterpret_cast<const int32_t *>(h_ps + o_att),
                *h_sta = reinterpret_cast<const int32_t *>(h_ps + o_sta);
  const int64_t *h_off = reinterpret_cast<const int64_t *>(h_ps + o_off);
  const int64_t total = *reinterpret_cast<const int64_t *>(h_ps + o_tot);
  out.lengths.assign(h_len, h_len + n); out.attempts.assign(h_att, h_att + n); out.offsets.assign(h_off, h_off + n);
  std::vector<int64_t> redo;
  int64_t pos = 1;
  for (int64_t i = 0; i < n; ++i) {
    if (h_sta[i] != EMIT_OK) return emit_status_error(h_sta[i], i);
    if (h_len[i] < 1 || h_len[i] > kEmitMaxLen || h_off[i] != pos) { set_error("emit_block: the device's lengths and offsets do not agree"); return P7X_EDEVICE; }
    pos += h_len[i] + 1;
    if (h_len[i] > cap) redo.push_back(i);
  }
  if (total != pos) { set_error("emit_block: the device's lengths and offsets do not agree"); return P7X_EDEVICE; }
  out.nres = total - 1 - n; out.nredrawn = (int64_t) redo.size();

  if ((st = set.out.reserve(ctx, (size_t) total)) != P7X_OK) return st;
  if (traces) {
    if ((st = set.out_st.reserve(ctx, (size_t) total)) != P7X_OK) return st;
    if ((st = set.out_node.reserve(ctx, (size_t) total * sizeof(int32_t))) != P7X_OK) return st;
  }
  CompactArgs c{};
  c.n = n; c.cap = (int32_t) cap; c.dsq = a.dsq; c.st = a.st; c.node = a.node; c.len = a.len; c.off = d_off;
  c.out_dsq = set.out.as<uint8_t>(); c.out_st = traces ? set.out_st.as<int8_t>() : nullptr; c.out_node = traces ? set.out_node.as<int32_t>() : nullptr;
  // pass 2: list entries are idx, slot_off (int64 each), then slot_cap (int32); everything it needs is reserved before the
  // first compaction is queued, so that nothing returns with work in flight
  DeviceBuf &slots2 = set.slots2, &slots2_st = set.slots2_st, &slots2_node = set.slots2_node;
  const size_t nr = redo.size();
  const size_t o_so = sizeof(int64_t) * nr, o_sc = 2 * o_so, list_bytes = o_sc + sizeof(int32_t) * nr;
  unsigned char *h_l = nullptr, *d_l = nullptr;
  if (nr) {
    if ((st = set.h_list.reserve(list_bytes)) != P7X_OK) return st;
    if ((st = set.list.reserve(ctx, list_bytes)) != P7X_OK) return st;
    h_l = set.h_list.as<unsigned char>(); d_l = set.list.as<unsigned char>();
    int64_t *l_idx = reinterpret_cast<int64_t *>(h_l), *l_off = reinterpret_cast<int64_t *>(h_l + o_so);
    int32_t *l_cap = reinterpret_cast<int32_t *>(h_l + o_sc);
    int64_t bytes2 = 0;
    for (size_t r = 0; r < nr; ++r) {
      const int32_t c4 = (h_len[redo[r]] + 3) / 4 * 4;
      l_idx[r] = redo[r]; l_off[r] = bytes2; l_cap[r] = c4; bytes2 += c4;
    }
    // the second pass's slots are as long as the sequences that outgrew the first's: with a small cap far more than those
    const int64_t w = traces ? 6 : 1, need2 = n * cap * w + total * w + bytes2 * w + n * 20 + 4096;
    if (budget >= 0 && need2 > budget) {
      set_error("emit workspace: " + std::to_string(need2) + " bytes with the slots of the " + std::to_string(nr) + " sequences that outgrew " +
                std::to_string(cap) + " residues, " + std::to_string(budget) + " available: emit fewer sequences per call");
      return P7X_EMEM;
    }
    if ((st = slots2.reserve(ctx, (size_t) bytes2)) != P7X_OK) return st;
    if (traces) {
      if ((st = slots2_st.reserve(ctx, (size_t) bytes2)) != P7X_OK) return st;
      if ((st = slots2_node.reserve(ctx, (size_t) bytes2 * sizeof(int32_t))) != P7X_OK) return st;
    }
  }
  hipLaunchKernelGGL(emit_compact_kernel, dim3((unsigned) ((n + 3) / 4)), dim3(256), 0, set.stream, c);
  P7X_HIP(hipGetLastError());

  if (nr) {
    P7X_HIP(hipMemcpyAsync(d_l, h_l, list_bytes, hipMemcpyHostToDevice, set.stream));
    EmitArgs b = a;
    b.n = (int64_t) nr; b.idx = reinterpret_cast<const int64_t *>(d_l); b.slot_off = reinterpret_cast<const int64_t *>(d_l + o_so);
    b.slot_cap = reinterpret_cast<const int32_t *>(d_l + o_sc);
    b.dsq = slots2.as<uint8_t>(); b.st = traces ? slots2_st.as<int8_t>() : nullptr; b.node = traces ? slots2_node.as<int32_t>() : nullptr;
    P7X_HIP(hipEventRecord(set.ev[2], set.stream));
    if ((st = launch_emit(b, lds, set.stream)) != P7X_OK) return st;
    P7X_HIP(hipEventRecord(set.ev[3], set.stream));
    CompactArgs c2 = c;
    c2.n = (int64_t) nr; c2.idx = b.idx; c2.slot_off = b.slot_off; c2.dsq = b.dsq; c2.st = b.st; c2.node = b.node;
    hipLaunchKernelGGL(emit_compact_kernel, dim3((unsigned) ((nr + 3) / 4)), dim3(256), 0, set.stream, c2);
    P7X_HIP(hipGetLastError());
  }
  out.dsq.resize((size_t) total);
  P7X_HIP(hipMemcpyAsync(out.dsq.data(), c.out_dsq, (size_t) total, hipMemcpyDeviceToHost, set.stream));
  if (traces) {
    out.st.resize((size_t) total); out.node.resize((size_t) total);
    P7X_HIP(hipMemcpyAsync(out.st.data(), c.out_st, (size_t) total, hipMemcpyDeviceToHost, set.stream));
    P7X_HIP(hipMemcpyAsync(out.node.data(), c.out_node, (size_t) total * sizeof(int32_t), hipMemcpyDeviceToHost, set.stream));
  }
  P7X_HIP(hipStreamSynchronize(set.stream));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, set.ev[0], set.ev[1]) == hipSuccess) out.kernel_us = (double) ms * 1000.0;
  if (nr && hipEventElapsedTime(&ms, set.ev[2], set.ev[3]) == hipSuccess) out.kernel_us += (double) ms * 1000.0;
  return P7X_OK;
}

} // namespace p7x

using namespace p7x;

extern "C" {

int p7x_emit_block(const p7x_emit_model *em, int device, int64_t n, uint64_t seed, int want_traces, p7x_emitted **out)
{
  if (!em || !out) { set_error("p7x_emit_block: bad arguments"); return P7X_EINVAL; }
  if (n < 0) { set_error("the number of sequences to emit is negative"); return P7X_EINVAL; }
  if (em->M > p7x_max_model_length()) { set_error(model_too_long("model too long for the emit kernel")); return P7X_EINVAL; }
  if (debug_opt(OPT_HOST_EMIT) > 0) return p7x_emit_block_host(em, n, seed, want_traces, 0, out);
  DeviceCtx *ctx = nullptr;
  int st = get_ctx(device, &ctx);
  if (st != P7X_OK) return st;
  auto *blk = new p7x_emitted();
  st = emit_block_device(*em, ctx, n, seed, want_traces != 0, *blk);
  if (st != P7X_OK) { delete blk; return st; }
  *out = blk;
  return P7X_OK;
}

} // extern "C"
