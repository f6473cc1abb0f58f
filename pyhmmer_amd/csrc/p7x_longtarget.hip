// p7x_longtarget.hip -- device half of the long-target (nhmmer) search: the SSV scan of every target strand
// (p7x_ssvlong.hip) and the hand-over of the rows it reports to the host tail (p7x_longtarget_host.cpp).
// Reference: LongTargetsPipeline._search_loop_longtargets, plan7.pyx:7541-7664; p7_Pipeline_LongTarget,
// p7_pipeline.pxd:131-143.
#include "p7x_device.hpp"
#include "p7x_kernels.hpp"
#include "p7x_host.hpp"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>

namespace p7x {

namespace {

// a scratch array of a stage, from the context's slab pool; never empty, whatever the count
static int alloc(DeviceBuf &b, DeviceCtx *ctx, size_t want) { return b.reserve(ctx, std::max<size_t>(want, 16)); }
static hipStream_t lt_window_stream(DeviceCtx *ctx)
{
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int k = ctx->lt_next; ctx->lt_next = (k + 1) % DeviceCtx::kLtStreams;
  if (!ctx->lt_stream[k] && hipStreamCreateWithFlags(&ctx->lt_stream[k], hipStreamNonBlocking) != hipSuccess) { (void) hipGetLastError(); return ctx->stream; }
  return ctx->lt_stream[k];
}

struct ScanRow { int64_t pos; int strand, k, sc; };

// The rows of a scan in order of (strand, position), one per row.  The parts of a scan in parts each report the best of
// their own cells of a row: the row's cell is the one upstream would pick among them -- the highest byte score, on a tie
// the first in the order in which p7_SSVFilter_longtarget unstripes the row (the kernel's key, with the whole model's Q16).
static void merge_scan_rows(std::vector<ScanRow> &rows, int Q16)
{
  auto key = [Q16](const ScanRow &r) { return ((r.k - 1) % Q16) * 16 + (r.k - 1) / Q16; };
  std::sort(rows.begin(), rows.end(), [&](const ScanRow &x, const ScanRow &y) {
    if (x.strand != y.strand) return x.strand < y.strand;
    if (x.pos != y.pos) return x.pos < y.pos;
    if (x.sc != y.sc) return x.sc > y.sc;
    return key(x) < key(y);
  });
  rows.erase(std::unique(rows.begin(), rows.end(), [](const ScanRow &x, const ScanRow &y) { return x.strand == y.strand && x.pos == y.pos; }), rows.end());
}

// A scan in parts parks one 16-bit cell per row and chunk between two parts (SsvLongArgs.bnd): 2.25 bytes per residue and
// strand with chunks of 8 M rows and M rows of warm-up.  The buffer is held to this many bytes; a scan that wants more goes
// in rounds of chunks, every part over the chunks of a round before the next round.
constexpr size_t kSsvBoundaryBudget = (size_t) 256 << 20;

// The device copy of a target set that its owner promised not to change (cfg.lt_resident_key): one per device, kept
// until a set with another key arrives.  Searches hold a reference while they run, so replacing the copy never pulls it
// from under a search still scanning it.
struct ResidentTargets {
  uint64_t key = 0; int device = -1; void *p = nullptr; size_t bytes = 0;
  ~ResidentTargets() { if (p) { (void) hipSetDevice(device); (void) hipFree(p); } }
};
static std::mutex g_resident_mu;
static std::map<int, std::shared_ptr<ResidentTargets>> &resident_by_device()
{ // never destroyed: at process exit the HIP runtime may be gone before a static destructor could free device memory
  static auto *m = new std::map<int, std::shared_ptr<ResidentTargets>>();
  return *m;
}

// Lets go of the kept copy of <device> (-1: every device) if it carries <key> (0: whatever it carries).  A search still
// scanning it holds its own reference: the memory goes when that search is done.
extern "C" int p7x_longtargets_release_resident(int device, uint64_t key)
{
  std::lock_guard<std::mutex> lk(g_resident_mu);
  auto &m = resident_by_device();
  for (auto it = m.begin(); it != m.end(); ) {
    if ((device < 0 || it->first == device) && (key == 0 || it->second->key == key)) it = m.erase(it);
    else ++it;
  }
  return P7X_OK;
}

// <seq1> (1-based, L residues) on the device: the kept copy when the key and the size match, else a fresh upload --
// kept in its place when there is a key.  *uploaded tells which it was (timing, tests).
static int resident_targets(DeviceCtx *ctx, int device, uint64_t key, const uint8_t *seq1, int64_t L, std::shared_ptr<ResidentTargets> &out, bool *uploaded)
{
  const size_t bytes = (size_t) L + 2;
  if (key != 0) {
    std::lock_guard<std::mutex> lk(g_resident_mu);
    auto it = resident_by_device().find(device);
    if (it != resident_by_device().end() && it->second->key == key && it->second->bytes == bytes) { out = it->second; *uploaded = false; return P7X_OK; }
  }
  auto r = std::make_shared<ResidentTargets>();
  r->key = key; r->device = device; r->bytes = bytes;
  P7X_HIP(hipMalloc(&r->p, std::max<size_t>(bytes, 16)));
  P7X_HIP(hipMemcpyAsync(static_cast<uint8_t *>(r->p) + 1, seq1 + 1, (size_t) L, hipMemcpyHostToDevice, ctx->stream));
  P7X_HIP(hipStreamSynchronize(ctx->stream));            // another search may pick the copy up as soon as it is published
  *uploaded = true;
  if (key != 0) {
    std::lock_guard<std::mutex> lk(g_resident_mu);
    resident_by_device()[device] = r;                      // the previous copy goes when its last search is done
  }
  out = std::move(r);
  return P7X_OK;
}

// The reset-free SSV scan of one target (both strands, or one): every row whose best diagonal reaches the threshold.
// <ms>: kernel time by HIP events.
// <ranges>, when given: only the chunks that touch one of these (strand, first, last) position ranges are scanned
// (a search dealt over several devices: every device scans the blocks of its own units).
struct ScanRange { int strand; int64_t first, last; };
static int scan_target(const p7x_pipeline_cfg &cfg, const Profile &p, DeviceCtx *ctx, const uint8_t *seq1 /* 1-based */, int64_t L,
                       int sc_thresh, int xB, int strands_mask, std::vector<ScanRow> &rows, double *ms, const std::vector<ScanRange> *ranges = nullptr,
                       int device = 0, uint64_t resident_key = 0)
{
  // The row maximum in every second row only (PAIR) tests against a threshold lowered by the most a cell can lose in one
  // row, and every group of rows that reaches the lowered threshold is run again: it pays while that loss is a few score
  // units (9 for bmyD, 12 for RF00001: 2^(loss/3) times as many groups are repeated as reach the threshold itself) and is
  // a loss for models with near-impossible emissions (60-110 units for the tests' Dirichlet models: every block would be
  // repeated).  Option ssv_kernel (tests, A/B): 3 = every row, 4 = every second row whatever the loss.
  constexpr int kMaxPairSlack = 16;
  int opt = debug_opt(OPT_SSV_KERNEL);
  const bool half = !(opt >= 5 && opt <= 7);       // 5, 6, 7: the int16 flavour of the kernel with the library's choice of rows / every row / every second row
  if (!half) opt = opt == 5 ? -1 : (opt == 6 ? 3 : 4);
  bool pair = opt != 3;
  const int forced = debug_opt(OPT_SSV_PARTS);
  std::vector<SsvPart> plan = ssvlong_plan(p.M, pair, forced);
  if (plan.empty()) { set_error(model_too_long("model too long for the long-target SSV kernel")); return P7X_EINVAL; }
  int pair_slack = 0;
  {
    std::vector<uint32_t> t4, tf;
    ssvlong_build_tables(p, plan[0].R, false, t4, tf, &pair_slack, 1, 1);       // the loss per row is the whole model's, whatever the part
  }
  if (pair && opt != 4 && pair_slack > kMaxPairSlack) {
    pair = false;
    plan = ssvlong_plan(p.M, false, forced);
  }
  const size_t P = plan.size();
  std::lock_guard<std::mutex> scan_turn(ctx->lt_scan_mu);      // one scan at a time per device (see DeviceCtx)
  DeviceBuf d_comp, d_nrec, d_pos, d_strand, d_k, d_sc, d_bnd;
  std::vector<DeviceBuf> d_tab4q(P), d_full(P);
  int st;
  if ((st = alloc(d_comp, ctx, 32)) || (st = alloc(d_nrec, ctx, 4))) return st;
  hipStream_t s = ctx->stream;
  std::shared_ptr<ResidentTargets> d_seq;
  bool uploaded = false;
  if ((st = resident_targets(ctx, device, resident_key, seq1, L, d_seq, &uploaded)) != P7X_OK) return st;
  if ((debug_opt(OPT_TRACE_LONGTARGET) > 0)) std::fprintf(stderr, "[lt] targets on the device: %s (%lld bytes, key %llu)\n", uploaded ? "uploaded" : "resident", (long long) L, (unsigned long long) resident_key);
  std::vector<std::vector<uint32_t>> tab4q(P), tab_full(P);
  {
    for (size_t q = 0; q < P; ++q) {
      ssvlong_build_tables(p, plan[q].R, pair && q + 1 == P, tab4q[q], tab_full[q], nullptr, plan[q].lo, plan[q].hi);
      if ((st = alloc(d_tab4q[q], ctx, tab4q[q].size() * 4)) || (st = alloc(d_full[q], ctx, tab_full[q].size() * 4))) return st;
      P7X_HIP(hipMemcpyAsync(d_tab4q[q].as<void>(), tab4q[q].data(), tab4q[q].size() * 4, hipMemcpyHostToDevice, s));
      P7X_HIP(hipMemcpyAsync(d_full[q].as<void>(), tab_full[q].data(), tab_full[q].size() * 4, hipMemcpyHostToDevice, s));
    }
    P7X_HIP(hipMemcpyAsync(d_comp.as<void>(), longtarget_complement(p.abc_type), 18, hipMemcpyHostToDevice, s));
  }
  // chunks: long enough that the M warm-up rows are a small overhead.  The kernel's wavefronts all stay on the device and
  // take the chunks in turn, so the number of chunks is made a multiple of the wavefronts (a last round that only some
  // of them take is paid in full: 16,384 chunks on 3,072 wavefronts were six rounds, the last a third full)
  const int nstrands_plan = strands_mask == 3 ? 2 : 1;
  long long waves = 0;
  if ((st = ssvlong_capacity(plan[0].R, pair, half, ctx->num_cu, &waves)) != P7X_OK) return st;
  const int64_t rounds = std::max<int64_t>(1, (L * nstrands_plan + waves * 49152 - 1) / (waves * 49152));
  const int64_t want_chunks = (waves * rounds + nstrands_plan - 1) / nstrands_plan;             // per strand
  int chunk_len = (int) std::max<int64_t>(8 * (int64_t) p.M, std::min<int64_t>(1 << 16, (L + want_chunks - 1) / want_chunks));
  chunk_len = ((chunk_len + 63) / 64) * 64;
  const int nstrands = strands_mask == 3 ? 2 : 1;
  SsvLongArgs a{};
  a.dsq = static_cast<const uint8_t *>(d_seq->p); a.comp = d_comp.as<const uint8_t>();
  a.L = L; a.M = p.M; a.Kp = p.Kp; a.chunk_len = chunk_len;
  a.chunks_per_strand = (L + chunk_len - 1) / chunk_len; a.nchunks = a.chunks_per_strand * nstrands;
  a.thresh_s = sc_thresh - xB - 32768; a.xB = xB; a.Q16 = p.Q16();
  a.nrec = d_nrec.as<int>();
  a.strand0 = strands_mask == 2 ? 1 : 0;
  a.pair_slack = pair_slack;
  DeviceBuf d_chunks;
  if (ranges) {
    std::vector<long long> list;
    for (const ScanRange &r : *ranges) {
      const long long s_off = (long long) (r.strand - a.strand0) * a.chunks_per_strand;
      for (long long c = (r.first - 1) / chunk_len; c <= (r.last - 1) / chunk_len && c < a.chunks_per_strand; ++c) list.push_back(s_off + c);
    }
    std::sort(list.begin(), list.end());
    list.erase(std::unique(list.begin(), list.end()), list.end());
    rows.clear();
    if (list.empty()) { if (ms) *ms = 0.0; return P7X_OK; }
    if ((st = alloc(d_chunks, ctx, list.size() * 8)) != P7X_OK) return st;
    P7X_HIP(hipMemcpyAsync(d_chunks.as<void>(), list.data(), list.size() * 8, hipMemcpyHostToDevice, s));
    P7X_HIP(hipStreamSynchronize(s));                       // <list> leaves scope
    a.chunk_list = d_chunks.as<const long long>(); a.nchunks = (long long) list.size();
  }
  // a scan in parts: the boundary buffer, and the chunks of a round
  const long long nchunks_all = a.nchunks;
  const long long *const list_all = a.chunk_list;
  long long per_round = nchunks_all;
  if (P > 1) {
    a.bnd_stride = (((long long) chunk_len + p.M + 63) / 64) * 64;                  // rows of a chunk: up to M of warm-up, then its own
    per_round = std::max<long long>(1, std::min<long long>(nchunks_all, (long long) (kSsvBoundaryBudget / ((size_t) a.bnd_stride * 2))));
    if ((st = alloc(d_bnd, ctx, (size_t) per_round * (size_t) a.bnd_stride * 2)) != P7X_OK) return st;
    a.bnd = d_bnd.as<unsigned short>();
  }
  struct Events {                     // destroyed on every way out
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() { if (e0) (void) hipEventDestroy(e0); if (e1) (void) hipEventDestroy(e1); }
  } ev;
  P7X_HIP(hipEventCreate(&ev.e0)); P7X_HIP(hipEventCreate(&ev.e1));
  hipEvent_t e0 = ev.e0, e1 = ev.e1;
  int cap = (int) std::min<int64_t>(std::max<int64_t>(1 << 16, L / 64), 1 << 28);
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((st = alloc(d_pos, ctx, (size_t) cap * 8)) || (st = alloc(d_strand, ctx, (size_t) cap)) || (st = alloc(d_k, ctx, (size_t) cap * 4)) || (st = alloc(d_sc, ctx, (size_t) cap * 4))) return st;
    a.rec_pos = d_pos.as<long long>(); a.rec_strand = d_strand.as<uint8_t>();
    a.rec_k = d_k.as<int>(); a.rec_sc = d_sc.as<int>(); a.rec_cap = cap;
    P7X_HIP(hipMemsetAsync(d_nrec.as<void>(), 0, 4, s));
    P7X_HIP(hipEventRecord(e0, s));
    for (long long c0 = 0; c0 < nchunks_all; c0 += per_round) {            // one round unless the scan is in parts
      a.nchunks = std::min(per_round, nchunks_all - c0);
      a.chunk_list = list_all ? list_all + c0 : nullptr; a.chunk0 = c0;
      for (size_t q = 0; q < P; ++q) {                                     // the parts of a round in order, on the one stream
        a.tab4q = d_tab4q[q].as<const uint32_t>(); a.tab_full = d_full[q].as<const uint32_t>();
        a.node0 = plan[q].lo - 1; a.nloc = plan[q].hi - plan[q].lo + 1; a.out_lane = plan[q].out_lane;
        if ((st = ssvlong_launch(plan[q].R, pair, half, a, ctx->num_cu, s, q > 0, q + 1 < P)) != P7X_OK) return st;
      }
    }
    P7X_HIP(hipEventRecord(e1, s));
    int nrec = 0;
    P7X_HIP(hipMemcpyAsync(&nrec, d_nrec.as<void>(), 4, hipMemcpyDeviceToHost, s));
    P7X_HIP(hipStreamSynchronize(s));
    float t = 0; (void) hipEventElapsedTime(&t, e0, e1);
    if (ms) *ms = t;
    if (nrec <= cap) {
      std::vector<long long> pos((size_t) nrec); std::vector<uint8_t> strand((size_t) nrec); std::vector<int> k((size_t) nrec), sc((size_t) nrec);
      if (nrec) {
        P7X_HIP(hipMemcpy(pos.data(), d_pos.as<void>(), (size_t) nrec * 8, hipMemcpyDeviceToHost));
        P7X_HIP(hipMemcpy(strand.data(), d_strand.as<void>(), (size_t) nrec, hipMemcpyDeviceToHost));
        P7X_HIP(hipMemcpy(k.data(), d_k.as<void>(), (size_t) nrec * 4, hipMemcpyDeviceToHost));
        P7X_HIP(hipMemcpy(sc.data(), d_sc.as<void>(), (size_t) nrec * 4, hipMemcpyDeviceToHost));
      }
      rows.resize((size_t) nrec);
      for (int i = 0; i < nrec; ++i) rows[(size_t) i] = ScanRow{ pos[(size_t) i], strand[(size_t) i], k[(size_t) i], sc[(size_t) i] };
      if (P > 1) merge_scan_rows(rows, p.Q16());
      else std::sort(rows.begin(), rows.end(), [](const ScanRow &x, const ScanRow &y) { return x.strand != y.strand ? x.strand < y.strand : x.pos < y.pos; });
      return P7X_OK;
    }
    cap = nrec + 1024;              // more rows than the buffer holds: once more with room for all of them
  }
  set_error("long-target SSV scan: record buffer could not be sized");
  return P7X_EMEM;
}

// seeds of one block of one strand from the rows of the whole-strand scan
// <shift>: what the scan's row positions are ahead of the target's own strand positions (a scan over several targets
// laid end to end)
static void block_seeds(const Profile &p, const uint8_t *seq1, int64_t Lt, int64_t i, int64_t bn, int strand, const std::vector<ScanRow> &rows,
                        int sc_thresh, int xB, std::vector<int64_t> &seeds3, int64_t shift = 0)
{
  // block rows 1..bn: strand 0: original positions i+1 .. i+bn; strand 1: reverse-strand positions (Lt-i-bn)+1 .. (Lt-i-bn)+bn
  const int64_t base = (strand == 0 ? i : Lt - i - bn) + shift;
  std::vector<LongTargetRow> br;
  auto lo = std::lower_bound(rows.begin(), rows.end(), ScanRow{ base + 1, strand, 0, 0 },
                             [](const ScanRow &x, const ScanRow &y) { return x.strand != y.strand ? x.strand < y.strand : x.pos < y.pos; });
  for (auto it = lo; it != rows.end() && it->strand == strand && it->pos <= base + bn; ++it) br.push_back(LongTargetRow{ it->pos - base, it->k, it->sc });
  if (br.empty()) return;
  const uint8_t *comp = longtarget_complement(p.abc_type);
  std::vector<uint8_t> buf((size_t) bn + 2, 255);
  if (strand == 0) std::memcpy(buf.data() + 1, seq1 + i + 1, (size_t) bn);
  else for (int64_t q = 1; q <= bn; ++q) buf[(size_t) q] = comp[seq1[i + bn - q + 1]];
  longtarget_seeds_from_rows(p, buf.data(), bn, br.data(), br.size(), sc_thresh, xB, seeds3);
}

// The windows of a target as one block of "targets" through the batch filter kernels: exact MSV scores (u8), the bias
// filter score, the standard Viterbi filter score (an upper bound for every row of the long-target Viterbi scan), and
// then the long-target Viterbi scan itself (vit_kernel with per-window row thresholds) for the windows that need it.
struct DeviceWindowScorer final : LongTargetWindowScorer {
  const p7x_oprofile *om; int device;
  p7x_seqdb *db = nullptr;
  p7x_seqdb *rdb = nullptr;             // the windows of the last regions() call: envelopes() refers to them
  float oa_guard = 0.0f;
  double ms = 0.0; size_t nwindows = 0;
  hipStream_t stream = nullptr;         // this search's own, for the long-target Viterbi scan of its windows
  DeviceWindowScorer(const p7x_oprofile *o, int d, float guard) : om(o), device(d), oa_guard(guard) {}
  ~DeviceWindowScorer() override { if (db) p7x_seqdb_destroy(db); if (rdb) p7x_seqdb_destroy(rdb); }
  int score(const uint8_t *seq1, int64_t L, const uint8_t *comp, const LongTargetWindowRef *w, size_t nw, double F1, bool do_bias,
            LongTargetWindowScore *sc) override
  {
    (void) L; (void) F1;
    const auto t0 = std::chrono::steady_clock::now();
    const Profile &p = om->p;
    std::vector<uint8_t> dsq; std::vector<int64_t> off; std::vector<int32_t> len;
    pack_windows(seq1, comp, w, nw, dsq, off, len);
    if (db) { p7x_seqdb_destroy(db); db = nullptr; }
    int st = p7x_seqdb_create(device, p.abc_type, dsq.data(), off.data(), len.data(), nw, &db);
    if (st != P7X_OK) return st;
    std::vector<int32_t> xJ(nw), xC(nw); std::vector<float> bias(nw);
    st = p7x_filters_batch(om, db, xJ.data(), xC.data(), nullptr, do_bias ? bias.data() : nullptr);
    if (st != P7X_OK) return st;
    for (size_t q = 0; q < nw; ++q) {
      sc[q].usc = msv_score_nats(xJ[q], tjb_of(p.scale_b, len[q]), p.base_b, p.scale_b);
      sc[q].vfsc = vit_score_nats(xC[q], xw_move_of(p.scale_w, len[q]), p.base_w, p.scale_w);
      sc[q].bias_filtersc = do_bias ? bias[q] : 0.0f; sc[q].have_vit = 1;
    }
    ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    nwindows += nw;
    return P7X_OK;
  }

  static void pack_windows(const uint8_t *seq1, const uint8_t *comp, const LongTargetWindowRef *w, size_t nw, std::vector<uint8_t> &dsq,
                           std::vector<int64_t> &off, std::vector<int32_t> &len)
  {
    size_t tot = 1;
    for (size_t q = 0; q < nw; ++q) tot += (size_t) w[q].length + 1;
    dsq.assign(tot, 255); off.resize(nw); len.resize(nw);
    size_t pos = 1;
    for (size_t q = 0; q < nw; ++q) {
      off[q] = (int64_t) pos; len[q] = (int32_t) w[q].length;
      if (w[q].strand == 0) std::memcpy(dsq.data() + pos, seq1 + w[q].start, (size_t) w[q].length);
      else for (int64_t r = 0; r < w[q].length; ++r) dsq[pos + (size_t) r] = comp[seq1[w[q].start - r]];
      pos += (size_t) w[q].length + 1;
    }
  }

  int forward(const uint8_t *seq1, const uint8_t *comp, const LongTargetWindowRef *w, size_t nw, float *fwdsc) override
  {
    if (nw == 0) return P7X_OK;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> dsq; std::vector<int64_t> off; std::vector<int32_t> len;
    pack_windows(seq1, comp, w, nw, dsq, off, len);
    p7x_seqdb *fdb = nullptr;
    int st = p7x_seqdb_create(device, om->p.abc_type, dsq.data(), off.data(), len.data(), nw, &fdb);
    if (st != P7X_OK) return st;
    st = p7x_filters_batch(om, fdb, nullptr, nullptr, fwdsc, nullptr);
    p7x_seqdb_destroy(fdb);
    ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st;
  }

  int regions(const uint8_t *seq1, const uint8_t *comp, const LongTargetWindowRef *w, size_t nw, std::vector<LongTargetWindowRegions> &out) override
  {
    out.assign(nw, LongTargetWindowRegions{});
    if (nw == 0) return P7X_OK;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> dsq; std::vector<int64_t> off; std::vector<int32_t> len;
    pack_windows(seq1, comp, w, nw, dsq, off, len);
    if (rdb) { p7x_seqdb_destroy(rdb); rdb = nullptr; }
    int st = p7x_seqdb_create(device, om->p.abc_type, dsq.data(), off.data(), len.data(), nw, &rdb);
    if (st != P7X_OK) return st;
    st = device_regions_of_all(om, rdb, out);
    ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st;
  }

  int envelopes(const LongTargetEnvRequest *req, size_t n, std::vector<LongTargetEnvResult> &out) override
  {
    out.assign(n, LongTargetEnvResult{});
    if (n == 0) return P7X_OK;
    if (!rdb) { set_error("long-target envelopes before the windows' region scan"); return P7X_EINVAL; }
    const auto t0 = std::chrono::steady_clock::now();
    const Profile &p = om->p;
    DeviceCtx *ctx = nullptr; DevProfile *dp = nullptr;
    int st;
    if ((st = get_ctx(device, &ctx)) != P7X_OK || (st = get_dev_profile(om, ctx, &dp)) != P7X_OK) return st;
    const int C = dp->vitC, Mpad = 64 * C, nrows = p.Kp + 1;
    if (C <= 0) { set_error(model_too_long("model too long for the envelope kernel")); return P7X_EINVAL; }
    // the envelopes' match odds in the kernel's table layout: [row x][position of node k], node k of lane z, slot c at c * 64 + z
    const size_t stride = (size_t) nrows * Mpad;
    std::vector<float> tables(n * stride, 0.0f);
    host_parallel_for((int) n, 0, [&](int e) {
      float *t = tables.data() + (size_t) e * stride;
      const float *rf = req[(size_t) e].rf;
      for (int x = 0; x < p.Kp; ++x)
        for (int k = 1; k <= p.M; ++k) t[(size_t) x * Mpad + ((k - 1) % C) * 64 + (k - 1) / C] = rf[(size_t) x * (p.M + 1) + k];
    });
    std::vector<EnvelopeRequest> rq(n);
    std::vector<int32_t> targets((size_t) rdb->n);
    for (int64_t t = 0; t < rdb->n; ++t) targets[(size_t) t] = (int32_t) t;
    for (size_t e = 0; e < n; ++e) rq[e] = EnvelopeRequest{ req[e].window, req[e].i, req[e].j };
    std::unique_ptr<EnvelopeScorer> scorer = make_device_envelope_scorer(ctx, rdb, oa_guard);
    std::vector<EnvelopeJob> jobs(1);
    jobs[0].om = om; jobs[0].req = &rq; jobs[0].targets = &targets; jobs[0].lt_tables = tables.data(); jobs[0].lt_stride = stride;
    if ((st = scorer->begin(jobs)) != P7X_OK) return st;
    std::vector<std::vector<EnvelopeResult>> res;
    if ((st = scorer->wait(res)) != P7X_OK) return st;
    for (size_t e = 0; e < n; ++e) {
      const EnvelopeResult &r = res[0][e];
      LongTargetEnvResult &o = out[e];
      o.envsc = r.envsc; o.oasc = r.oasc; o.orig = r.orig; o.status = r.status;
      if (r.ntrace > 0) { o.ta.assign(r.ta, r.ta + r.ntrace); o.ti.assign(r.ti, r.ti + r.ntrace); o.tp.assign(r.tp, r.tp + r.ntrace); }
    }
    ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return P7X_OK;
  }

  int viterbi(const int *which, const int *thresh, size_t n, std::vector<int> &rec) override
  {
    rec.clear();
    if (n == 0 || !db) return P7X_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const Profile &p = om->p;
    DeviceCtx *ctx = nullptr; DevProfile *dp = nullptr;
    int st;
    if ((st = get_ctx(device, &ctx)) != P7X_OK || (st = get_dev_profile(om, ctx, &dp)) != P7X_OK) return st;
    if (dp->vitC <= 0) { set_error(model_too_long("model too long for the wave-per-target Viterbi kernel")); return P7X_EINVAL; }
    // caller index -> slot of the window block (slots are sorted by decreasing length)
    std::vector<int32_t> slot_of((size_t) db->n, -1);
    for (int64_t sl = 0; sl < db->nslots; ++sl) slot_of[(size_t) db->h_order[(size_t) sl]] = (int32_t) sl;
    std::vector<int32_t> list(n);
    for (size_t i = 0; i < n; ++i) list[i] = slot_of[(size_t) which[i]];
    hipStream_t s = stream ? stream : (stream = lt_window_stream(ctx));
    DeviceBuf d_list, d_thr, d_xc, d_nrec, d_rec, d_args;
    if ((st = alloc(d_list, ctx, n * 4)) || (st = alloc(d_thr, ctx, n * 4)) || (st = alloc(d_xc, ctx, n * 4)) || (st = alloc(d_nrec, ctx, 4)) || (st = alloc(d_args, ctx, sizeof(WaveSeqArgs)))) return st;
    P7X_HIP(hipMemcpyAsync(d_list.as<void>(), list.data(), n * 4, hipMemcpyHostToDevice, s));
    P7X_HIP(hipMemcpyAsync(d_thr.as<void>(), thresh, n * 4, hipMemcpyHostToDevice, s));
    int cap = (int) std::max<size_t>(1 << 16, 64 * n);
    for (int attempt = 0; attempt < 2; ++attempt) {
      if ((st = alloc(d_rec, ctx, (size_t) cap * 12)) != P7X_OK) return st;
      WaveSeqArgs a{};
      a.M = p.M; a.C = dp->vitC; a.nrows = p.Kp + 1;
      a.trans = dp->vit_trans; a.emis = dp->vit_emis;
      a.dsq = db->d_dsq; a.slot_off = db->d_slot_off; a.slot_len = db->d_slot_len;
      a.list = d_list.as<const int32_t>(); a.nlist = (int) n;
      a.xwmove_tab = ctx->lt.xwmove; a.base_w = p.base_w; a.xw_e = p.xw[XE][MOVE]; a.ddbound = p.ddbound_w;
      a.out_xC = d_xc.as<int32_t>();
      a.lt_thresh = d_thr.as<const int>(); a.lt_nrec = d_nrec.as<int>(); a.lt_rec = d_rec.as<int>(); a.lt_cap = cap;
      P7X_HIP(hipMemcpyAsync(d_args.as<void>(), &a, sizeof(a), hipMemcpyHostToDevice, s));
      P7X_HIP(hipMemsetAsync(d_nrec.as<void>(), 0, 4, s));
      ArgRun<WaveSeqArgs> run; run.host = &a; run.dev = d_args.as<void>(); run.stride = (uint32_t) sizeof(WaveSeqArgs); run.n = 1;
      if ((st = vit_launch(run, ctx->num_cu, s)) != P7X_OK) return st;
      int nrec = 0;
      P7X_HIP(hipMemcpyAsync(&nrec, d_nrec.as<void>(), 4, hipMemcpyDeviceToHost, s));
      P7X_HIP(hipStreamSynchronize(s));
      if (nrec <= cap) {
        rec.resize((size_t) nrec * 3);
        if (nrec) P7X_HIP(hipMemcpy(rec.data(), d_rec.as<void>(), (size_t) nrec * 12, hipMemcpyDeviceToHost));
        // (item, row, node) ascending, as the host scan emits them
        std::vector<int> ord((size_t) nrec);
        for (int i = 0; i < nrec; ++i) ord[(size_t) i] = i;
        std::sort(ord.begin(), ord.end(), [&](int x, int y) {
          for (int f = 0; f < 3; ++f) if (rec[(size_t) x * 3 + f] != rec[(size_t) y * 3 + f]) return rec[(size_t) x * 3 + f] < rec[(size_t) y * 3 + f];
          return false;
        });
        std::vector<int> sorted((size_t) nrec * 3);
        for (int i = 0; i < nrec; ++i) for (int f = 0; f < 3; ++f) sorted[(size_t) i * 3 + f] = rec[(size_t) ord[(size_t) i] * 3 + f];
        rec.swap(sorted);
        ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return P7X_OK;
      }
      cap = nrec + 1024;
    }
    set_error("long-target Viterbi scan: record buffer could not be sized");
    return P7X_EMEM;
  }
};

} // namespace
} // namespace p7x

using namespace p7x;

extern "C" {

int p7x_search_longtargets(const p7x_pipeline_cfg *cfg, const p7x_oprofile *om, int device,
                           const uint8_t *dsq, const int64_t *offsets, const int64_t *lengths, size_t n,
                           const char *const *names, const char *const *accs, const char *const *descs, p7x_tophits **out)
{
  if (!cfg || !om || !out || (n && (!dsq || !offsets || !lengths))) { set_error("p7x_search_longtargets: bad arguments"); return P7X_EINVAL; }
  if (!cfg->long_targets) { set_error("p7x_search_longtargets: cfg.long_targets is not set"); return P7X_EINVAL; }
  if (cfg->lt_nparts > 1 && (cfg->lt_part < 0 || cfg->lt_part >= cfg->lt_nparts)) { set_error("p7x_search_longtargets: cfg.lt_part is not one of the cfg.lt_nparts parts"); return P7X_EINVAL; }
  const Profile &p = om->p;
  int max_length = 0, sc_thresh = 0, xB = 0;
  int st = longtarget_setup(*cfg, p, &max_length, &sc_thresh, &xB);
  if (st != P7X_OK) return st;
  DeviceCtx *ctx = nullptr;
  if ((st = get_ctx(device, &ctx)) != P7X_OK) return st;
  const int mask = cfg->strands == P7X_STRAND_TOPONLY ? 1 : (cfg->strands == P7X_STRAND_BOTTOMONLY ? 2 : 3);
  const int64_t W = cfg->block_length, C = max_length;
  const auto t_begin = std::chrono::steady_clock::now();
  std::vector<LongTargetSeed> seeds;
  double scan_ms = 0.0;
  // One scan for the whole target set: the records lie end to end in <dsq> with a sentinel between them, which the scan
  // kernels take as the end of every diagonal, so a file of 1e5 contigs costs one launch, one upload and one set of
  // buffers like a single chromosome does.  Scan position q of strand 0 is dsq[q]; of strand 1 it is dsq[Ltot - q + 1]
  // (the whole buffer read backwards: the last target's reverse strand comes first).
  std::vector<uint8_t> packed;                    // only when the caller's records do not lie end to end
  std::vector<int64_t> poff;
  const int64_t *off = offsets;
  const uint8_t *base = dsq;
  {
    bool contiguous = n == 0 || offsets[0] >= 1;
    for (size_t t = 0; contiguous && t + 1 < n; ++t) contiguous = offsets[t + 1] == offsets[t] + lengths[t] + 1;
    for (size_t t = 0; contiguous && t + 1 < n; ++t) contiguous = dsq[offsets[t] + lengths[t]] >= (uint8_t) p.Kp;
    if (!contiguous) {
      poff.resize(n);
      int64_t at = 1;
      for (size_t t = 0; t < n; ++t) { poff[t] = at; at += std::max<int64_t>(lengths[t], 0) + 1; }
      packed.assign((size_t) at + 1, 255);
      for (size_t t = 0; t < n; ++t) if (lengths[t] > 0) std::memcpy(packed.data() + poff[t], dsq + offsets[t], (size_t) lengths[t]);
      off = poff.data(); base = packed.data();
    }
  }
  const int64_t first_at = n ? off[0] : 1;                                  // the scan starts at the first record
  const int64_t Ltot = n ? off[n - 1] + std::max<int64_t>(lengths[n - 1], 0) - first_at : 0;   // scan positions 1..Ltot
  const uint8_t *scan1 = base + first_at - 1;                               // scan1[q] = position q of strand 0
  LongTargetUnits all_units; all_units.count(*cfg, max_length, lengths, n);
  uint64_t unit = 0;
  // upstream's bookkeeping per (target, block, strand): the units are independent, the host workers take them side by
  // side; with the search dealt over several devices (cfg.lt_nparts) this call only has the units of its part
  struct Unit { size_t t; int64_t i, bn; int strand; int64_t shift; std::vector<int64_t> s3; };
  std::vector<Unit> units;
  std::vector<ScanRange> ranges;
  for (size_t t = 0; t < n; ++t) {
    const int64_t Lt = lengths[t];
    if (Lt <= 0) continue;
    const int64_t at = off[t] - first_at + 1;                 // scan position of the target's first residue on strand 0
    for (int64_t i = 0; i < Lt; i += W - C) {
      const int64_t bc = i == 0 ? 0 : std::min<int64_t>(C, Lt - i);
      const int64_t bw = std::min<int64_t>(W, Lt - i - bc);
      const int64_t bn = bc + bw;
      if (bn <= 0) break;
      for (int strand = 0; strand < 2; ++strand) if (mask & (1 << strand)) {
        if (!all_units.mine(unit++)) continue;
        // the target's strand position ps is scan position ps + shift
        const int64_t shift = strand == 0 ? at - 1 : Ltot - (at + Lt - 1);
        units.push_back(Unit{ t, i, bn, strand, shift, {} });
        const int64_t b0 = (strand == 0 ? i : Lt - i - bn) + shift;  // the block's rows in scan coordinates: b0 + 1 .. b0 + bn
        ranges.push_back(ScanRange{ strand, b0 + 1, b0 + bn });
      }
    }
  }
  if (!units.empty() && Ltot > 0) {
    std::vector<ScanRow> rows;
    double ms = 0.0;
    const auto ts0 = std::chrono::steady_clock::now();
    // the kept copy is of the caller's buffer as it lies: a set that had to be packed first is uploaded per call
    const uint64_t rkey = packed.empty() ? cfg->lt_resident_key : 0;
    if ((st = scan_target(*cfg, p, ctx, scan1, Ltot, sc_thresh, xB, mask, rows, &ms, all_units.nparts > 1 ? &ranges : nullptr, device, rkey)) != P7X_OK) return st;
    scan_ms += ms;
    const auto ts1 = std::chrono::steady_clock::now();
    host_parallel_for((int) units.size(), cfg->host_threads, [&](int u) {
      Unit &un = units[(size_t) u];
      block_seeds(p, base + off[un.t] - 1, lengths[un.t], un.i, un.bn, un.strand, rows, sc_thresh, xB, un.s3, un.shift);
    });
    for (const Unit &un : units)
      for (size_t q = 0; q + 2 < un.s3.size(); q += 3) seeds.push_back(LongTargetSeed{ (int64_t) un.t, un.i, un.strand, un.s3[q], (int) un.s3[q + 1], un.s3[q + 2] });
    if ((debug_opt(OPT_TRACE_LONGTARGET) > 0))
      std::fprintf(stderr, "[lt] %zu targets, %lld positions: scan call %.1f ms (kernel %.1f), %zu rows, %zu seeds, seed bookkeeping %.1f ms\n", n,
                   (long long) Ltot, std::chrono::duration<double, std::milli>(ts1 - ts0).count(), ms, rows.size(), seeds.size(),
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts1).count());
  }
  const auto t_host = std::chrono::steady_clock::now();
  DeviceWindowScorer scorer(om, device, cfg->oa_guard);
  st = longtarget_run_host(*cfg, om, dsq, offsets, lengths, n, names, accs, descs, seeds, out, &scorer);
  if (st == P7X_OK && *out) {
    (*out)->ms[P7X_MS_MSV_KERNEL] = scan_ms;                   // (enum p7x_timing, the long-target meanings) the SSV scan kernels (HIP events)
    (*out)->ms[P7X_MS_MSV] = std::chrono::duration<double, std::milli>(t_host - t_begin).count();      // scan + seeds, wall
    (*out)->ms[P7X_MS_BIAS] = scorer.ms;                       // window MSV / bias / Viterbi batch on the device, wall
    (*out)->ms[P7X_MS_HOST_DOMAINDEF] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host).count();   // host tail incl. P7X_MS_BIAS
  }
  return st;
}

int64_t p7x_ssv_longtarget_seeds(const p7x_pipeline_cfg *cfg, const p7x_oprofile *om, int device, const uint8_t *dsq, int64_t L,
                                 int complement, int64_t *seeds, size_t cap)
{
  if (!cfg || !om || !dsq || L <= 0 || (cap && !seeds)) { set_error("p7x_ssv_longtarget_seeds: bad arguments"); return -P7X_EINVAL; }
  const Profile &p = om->p;
  int max_length = 0, sc_thresh = 0, xB = 0;
  int st = longtarget_setup(*cfg, p, &max_length, &sc_thresh, &xB);
  if (st != P7X_OK) return -st;
  DeviceCtx *ctx = nullptr;
  if ((st = get_ctx(device, &ctx)) != P7X_OK) return -st;
  std::vector<ScanRow> rows;
  if ((st = scan_target(*cfg, p, ctx, dsq - 1, L, sc_thresh, xB, complement ? 2 : 1, rows, nullptr, nullptr, device, 0)) != P7X_OK) return -st;
  std::vector<int64_t> s3;
  block_seeds(p, dsq - 1, L, 0, L, complement ? 1 : 0, rows, sc_thresh, xB, s3);
  const size_t ns = s3.size() / 3;
  for (size_t q = 0; q < ns && q < cap; ++q) { seeds[3 * q] = s3[3 * q]; seeds[3 * q + 1] = s3[3 * q + 1]; seeds[3 * q + 2] = s3[3 * q + 2]; }
  return (int64_t) ns;
}

int64_t p7x_debug_ssv_tables(const p7x_oprofile *om, int pair, int32_t *R, int32_t *pair_slack, uint32_t *tab4q, size_t cap_words)
{
  if (!om) { set_error("p7x_debug_ssv_tables: no profile"); return -P7X_EINVAL; }
  const Profile &p = om->p;
  const int r = ssvlong_pick_R(p.M, pair != 0);
  if (p.M > max_model_length()) { set_error(model_too_long("model too long for the long-target SSV kernel")); return -P7X_EINVAL; }
  if (r < 0) { set_error("p7x_debug_ssv_tables: the model is scanned in parts, see p7x_debug_ssv_part_tables"); return -P7X_EINVAL; }
  std::vector<uint32_t> quads, full;
  int slack = 0;
  ssvlong_build_tables(p, r, pair != 0, quads, full, &slack);
  if (R) *R = r;
  if (pair_slack) *pair_slack = slack;
  if (tab4q && cap_words >= quads.size()) std::copy(quads.begin(), quads.end(), tab4q);
  return (int64_t) quads.size();
}

int p7x_debug_ssv_plan(int M, int pair, int parts_forced, int32_t *lo, int32_t *hi, int32_t *R, int cap)
{
  const std::vector<SsvPart> plan = ssvlong_plan(M, pair != 0, parts_forced);
  if (plan.empty()) { set_error(model_too_long("model too long for the long-target SSV kernel")); return -P7X_EINVAL; }
  for (size_t q = 0; q < plan.size() && (int) q < cap; ++q) {
    if (lo) lo[q] = plan[q].lo;
    if (hi) hi[q] = plan[q].hi;
    if (R) R[q] = plan[q].R;
  }
  return (int) plan.size();
}

int64_t p7x_debug_ssv_part_tables(const p7x_oprofile *om, int pair, int parts_forced, int part, int32_t *lo, int32_t *hi, int32_t *R, uint32_t *tab4q, size_t cap_words)
{
  if (!om) { set_error("p7x_debug_ssv_part_tables: no profile"); return -P7X_EINVAL; }
  const Profile &p = om->p;
  const std::vector<SsvPart> plan = ssvlong_plan(p.M, pair != 0, parts_forced);
  if (plan.empty()) { set_error(model_too_long("model too long for the long-target SSV kernel")); return -P7X_EINVAL; }
  if (part < 0 || (size_t) part >= plan.size()) { set_error("p7x_debug_ssv_part_tables: no such part"); return -P7X_EINVAL; }
  const SsvPart &sp = plan[(size_t) part];
  std::vector<uint32_t> quads, full;
  ssvlong_build_tables(p, sp.R, pair != 0 && (size_t) part + 1 == plan.size(), quads, full, nullptr, sp.lo, sp.hi);
  if (lo) *lo = sp.lo;
  if (hi) *hi = sp.hi;
  if (R) *R = sp.R;
  if (tab4q && cap_words >= quads.size()) std::copy(quads.begin(), quads.end(), tab4q);
  return (int64_t) quads.size();
}

int64_t p7x_debug_ssv_merge_rows(int Q16, size_t n, const int64_t *pos, const int32_t *strand, const int32_t *k, const int32_t *sc,
                                 int64_t *out_pos, int32_t *out_strand, int32_t *out_k, int32_t *out_sc)
{
  if (Q16 < 1 || (n && (!pos || !strand || !k || !sc || !out_pos || !out_strand || !out_k || !out_sc))) { set_error("p7x_debug_ssv_merge_rows: bad arguments"); return -P7X_EINVAL; }
  std::vector<ScanRow> rows(n);
  for (size_t i = 0; i < n; ++i) rows[i] = ScanRow{ pos[i], strand[i], k[i], sc[i] };
  merge_scan_rows(rows, Q16);
  for (size_t i = 0; i < rows.size(); ++i) { out_pos[i] = rows[i].pos; out_strand[i] = rows[i].strand; out_k[i] = rows[i].k; out_sc[i] = rows[i].sc; }
  return (int64_t) rows.size();
}

} // extern "C"

// ------------------------------------------------------------------------------------------------- nhmmscan
// One query sequence against a library of models: the scan orientation of the search above (an extension: the reference's
// LongTargetsPipeline.scan_seq raises).  The SSV scan of all models is one launch per (R, PAIR) group of
// ssvlong_multi_kernel over one upload of the sequence; everything behind the rows is the search's own code, per model.
#include <atomic>
#include <thread>

namespace {

// how the options choose cells and rows, as scan_target reads them
struct SsvFlavour { bool half; int opt; int forced; };
SsvFlavour ssv_flavour()
{
  SsvFlavour f{ true, debug_opt(OPT_SSV_KERNEL), debug_opt(OPT_SSV_PARTS) };
  f.half = !(f.opt >= 5 && f.opt <= 7);
  if (!f.half) f.opt = f.opt == 5 ? -1 : (f.opt == 6 ? 3 : 4);
  return f;
}
// the row flavour of a model (scan_target: kMaxPairSlack and the overrides of option ssv_kernel)
bool ssv_pair_of(const SsvFlavour &f, int pair_slack)
{
  constexpr int kMaxPairSlack = 16;
  bool pair = f.opt != 3;
  if (pair && f.opt != 4 && pair_slack > kMaxPairSlack) pair = false;
  return pair;
}
int ssv_pair_slack(const Profile &p)
{
  std::vector<uint32_t> t4, tf;
  int slack = 0;
  ssvlong_build_tables(p, 2, false, t4, tf, &slack, 1, 1);
  return slack;
}

// The launches of a batch: the models grouped by (R, PAIR), groups in order of their first model.  A model that the scan
// takes in chained parts is in no launch (launch_of = -1): it goes through scan_target.  One rule for both row flavours --
// a model is batched when one launch holds it WITH the virtual node of PAIR (M <= 6,141) --, so the path a model takes
// depends on its length and on option ssv_parts, never on its emissions.
struct SsvBatchLaunch { int R; bool pair; std::vector<int> models; };
void ssv_batch_plan(const int *M, const int *slack, int n, const SsvFlavour &f, std::vector<SsvBatchLaunch> &launches, std::vector<int> &launch_of)
{
  launches.clear(); launch_of.assign((size_t) std::max(n, 0), -1);
  std::map<std::pair<int, int>, int> at;
  for (int i = 0; i < n; ++i) {
    if (M[i] < 1) continue;
    const bool pair = ssv_pair_of(f, slack[i]);
    if (ssvlong_plan(M[i], true, f.forced).size() != 1 || ssvlong_plan(M[i], pair, f.forced).size() != 1) continue;
    const int R = ssvlong_pick_R(M[i], pair);
    if (R < 0) continue;
    auto it = at.find({ R, pair ? 1 : 0 });
    if (it == at.end()) { it = at.emplace(std::make_pair(R, pair ? 1 : 0), (int) launches.size()).first; launches.push_back(SsvBatchLaunch{ R, pair, {} }); }
    launches[(size_t) it->second].models.push_back(i);
    launch_of[(size_t) i] = it->second;
  }
}

std::atomic<int64_t> g_batch_stats[8];

} // namespace

struct p7x_lt_library {
  int device = 0;
  DeviceCtx *ctx = nullptr;
  SsvFlavour flavour{};
  int Kp = 0, abc_type = 0;
  std::vector<const p7x_oprofile *> oms;
  std::vector<int> slack, M;
  std::vector<std::string> names;
  std::vector<SsvBatchLaunch> launches;
  std::vector<int> launch_of;
  std::vector<long long> tab4q_off, full_off;      // per model: uint4 / dwords into the two buffers
  DeviceBuf d_tab4q, d_full, d_comp;
};

namespace {

int lt_library_build(const p7x_oprofile *const *oms, size_t n, int device, std::unique_ptr<p7x_lt_library> &out)
{
  auto lib = std::make_unique<p7x_lt_library>();
  int st;
  if ((st = get_ctx(device, &lib->ctx)) != P7X_OK) return st;
  lib->device = device; lib->flavour = ssv_flavour();
  lib->oms.assign(oms, oms + n);
  lib->slack.resize(n);
  std::vector<int> M(n);
  for (size_t m = 0; m < n; ++m) {
    if (!oms[m]) { set_error("long-target library: missing profile"); return P7X_EINVAL; }
    const Profile &p = oms[m]->p;
    if (p.abc_type != P7X_DNA && p.abc_type != P7X_RNA) { set_error("long-target pipeline needs a nucleotide model"); return P7X_EINVAL; }
    if (m == 0) { lib->Kp = p.Kp; lib->abc_type = p.abc_type; }
    else if (p.Kp != lib->Kp) { set_error("long-target library: models of different alphabets"); return P7X_EINVAL; }
    M[m] = p.M;
  }
  host_parallel_for((int) n, 0, [&](int m) { lib->slack[(size_t) m] = ssv_pair_slack(oms[m]->p); });
  lib->M = M;
  lib->names.resize(n);
  for (size_t m = 0; m < n; ++m) lib->names[m] = oms[m]->p.name;
  ssv_batch_plan(M.data(), lib->slack.data(), (int) n, lib->flavour, lib->launches, lib->launch_of);
  lib->tab4q_off.assign(n, -1); lib->full_off.assign(n, -1);
  long long q_at = 0, f_at = 0;
  for (const SsvBatchLaunch &ln : lib->launches)
    for (int m : ln.models) {
      lib->tab4q_off[(size_t) m] = q_at; lib->full_off[(size_t) m] = f_at;
      q_at += (long long) (ssvlong_lds_bytes(ln.R) / 16);
      f_at += (long long) 2 * lib->Kp * ln.R * 64;
    }
  if (q_at == 0) { out = std::move(lib); return P7X_OK; }           // nothing batched: no device tables
  std::vector<uint32_t> h4((size_t) q_at * 4), hf((size_t) f_at);
  for (const SsvBatchLaunch &ln : lib->launches)
    host_parallel_for((int) ln.models.size(), 0, [&](int j) {
      const int m = ln.models[(size_t) j];
      std::vector<uint32_t> t4, tf;
      ssvlong_build_tables(oms[m]->p, ln.R, ln.pair, t4, tf, nullptr);
      std::memcpy(h4.data() + (size_t) lib->tab4q_off[(size_t) m] * 4, t4.data(), t4.size() * 4);
      std::memcpy(hf.data() + (size_t) lib->full_off[(size_t) m], tf.data(), tf.size() * 4);
    });
  DeviceCtx *ctx = lib->ctx;
  if ((st = alloc(lib->d_tab4q, ctx, h4.size() * 4)) || (st = alloc(lib->d_full, ctx, hf.size() * 4)) || (st = alloc(lib->d_comp, ctx, 32))) return st;
  {
    std::lock_guard<std::mutex> turn(ctx->lt_scan_mu);
    P7X_HIP(hipSetDevice(device));
    P7X_HIP(hipMemcpyAsync(lib->d_tab4q.as<void>(), h4.data(), h4.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    P7X_HIP(hipMemcpyAsync(lib->d_full.as<void>(), hf.data(), hf.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    P7X_HIP(hipMemcpyAsync(lib->d_comp.as<void>(), longtarget_complement(lib->abc_type), 18, hipMemcpyHostToDevice, ctx->stream));
    P7X_HIP(hipStreamSynchronize(ctx->stream));
  }
  g_batch_stats[0]++;
  out = std::move(lib);
  return P7X_OK;
}

bool lt_library_matches(const p7x_lt_library *lib, const p7x_oprofile *const *oms, size_t n, int device)
{
  if (!lib || lib->device != device || lib->oms.size() != n) return false;
  // the same profile objects, and still the models the tables were built from (a freed profile's address may come back)
  for (size_t m = 0; m < n; ++m) if (lib->oms[m] != oms[m] || !oms[m] || oms[m]->p.M != lib->M[m] || oms[m]->p.name != lib->names[m]) return false;
  const SsvFlavour f = ssv_flavour();
  return f.half == lib->flavour.half && f.opt == lib->flavour.opt && f.forced == lib->flavour.forced;
}

// The reset-free scan of one target with every model of <lib>: rows[m] = the rows of model m that reach its threshold, in
// order of (strand, position).  Chunks: per model at least 8 M rows, a multiple of 64, and short enough that the chunk
// lists of a launch's models together fill the device once; option ssv_scan_chunk forces the length.  The rows do not
// depend on it.
int scan_target_batched(const p7x_pipeline_cfg &cfg, p7x_lt_library *lib, const uint8_t *seq1, int64_t L, const int *sc_thresh, const int *xB,
                        int strands_mask, std::vector<std::vector<ScanRow>> &rows, double *ms, uint64_t resident_key)
{
  const size_t n = lib->oms.size();
  DeviceCtx *ctx = lib->ctx;
  const int device = lib->device;
  rows.assign(n, {});
  if (ms) *ms = 0.0;
  g_batch_stats[1]++;
  const int nstrands = strands_mask == 3 ? 2 : 1;
  int st;
  size_t nbatched = 0;
  for (const SsvBatchLaunch &ln : lib->launches) nbatched += ln.models.size();
  if (nbatched) {
    std::lock_guard<std::mutex> scan_turn(ctx->lt_scan_mu);      // one scan, single or batched, per device at a time
    P7X_HIP(hipSetDevice(device));
    hipStream_t s = ctx->stream;
    std::shared_ptr<ResidentTargets> d_seq;
    bool uploaded = false;
    if ((st = resident_targets(ctx, device, resident_key, seq1, L, d_seq, &uploaded)) != P7X_OK) return st;
    // the records of every launch, end to end
    const int forced_chunk = debug_opt(OPT_SSV_SCAN_CHUNK);
    std::vector<SsvModelRec> recs; recs.reserve(nbatched);
    std::vector<long long> max_chunks(lib->launches.size(), 0);
    double cells = 0.0;
    for (size_t g = 0; g < lib->launches.size(); ++g) {
      const SsvBatchLaunch &ln = lib->launches[g];
      long long waves = 0;
      if ((st = ssvlong_multi_capacity(ln.R, ln.pair, lib->flavour.half, ctx->num_cu, &waves)) != P7X_OK) return st;
      const int64_t want = std::max<int64_t>(1, waves / (int64_t) ln.models.size() / nstrands);      // chunks per model and strand
      for (int m : ln.models) {
        const Profile &p = lib->oms[(size_t) m]->p;
        int64_t len = std::max<int64_t>(8 * (int64_t) p.M, std::min<int64_t>(1 << 16, (L + want - 1) / want));
        if (forced_chunk > 0) len = forced_chunk;
        len = std::max<int64_t>(64, ((len + 63) / 64) * 64);
        SsvModelRec r{};
        r.tab4q_off = lib->tab4q_off[(size_t) m]; r.full_off = lib->full_off[(size_t) m];
        r.chunk_len = (int) len; r.chunks_per_strand = (L + len - 1) / len;
        r.M = p.M; r.Q16 = p.Q16(); r.thresh_s = sc_thresh[m] - xB[m] - 32768; r.xB = xB[m];
        r.pair_slack = lib->slack[(size_t) m]; r.index = m;
        max_chunks[g] = std::max(max_chunks[g], r.chunks_per_strand * nstrands);
        recs.push_back(r);
        cells += (double) L * nstrands * p.M;
      }
    }
    DeviceBuf d_recs, d_nrec, d_pos, d_strand, d_k, d_sc, d_model;
    if ((st = alloc(d_recs, ctx, recs.size() * sizeof(SsvModelRec))) || (st = alloc(d_nrec, ctx, 4))) return st;
    P7X_HIP(hipMemcpyAsync(d_recs.as<void>(), recs.data(), recs.size() * sizeof(SsvModelRec), hipMemcpyHostToDevice, s));
    SsvMultiArgs a{};
    a.tab4q = lib->d_tab4q.as<const uint32_t>(); a.tab_full = lib->d_full.as<const uint32_t>();
    a.dsq = static_cast<const uint8_t *>(d_seq->p); a.comp = lib->d_comp.as<const uint8_t>();
    a.L = L; a.Kp = lib->Kp; a.nstrands = nstrands; a.strand0 = strands_mask == 2 ? 1 : 0;
    a.nrec = d_nrec.as<int>();
    struct Events {
      hipEvent_t e0 = nullptr, e1 = nullptr;
      ~Events() { if (e0) (void) hipEventDestroy(e0); if (e1) (void) hipEventDestroy(e1); }
    } ev;
    P7X_HIP(hipEventCreate(&ev.e0)); P7X_HIP(hipEventCreate(&ev.e1));
    // one record counter per scan; a buffer that turns out too small is grown to what the scan counted and the scan repeated
    int cap = (int) std::min<int64_t>(std::max<int64_t>(4096, (L * nstrands / 256 + 16) * (int64_t) nbatched), 1 << 24);
    bool done = false;
    for (int attempt = 0; attempt < 2 && !done; ++attempt) {
      if ((st = alloc(d_pos, ctx, (size_t) cap * 8)) || (st = alloc(d_strand, ctx, (size_t) cap)) || (st = alloc(d_k, ctx, (size_t) cap * 4)) ||
          (st = alloc(d_sc, ctx, (size_t) cap * 4)) || (st = alloc(d_model, ctx, (size_t) cap * 4))) return st;
      a.rec_pos = d_pos.as<long long>(); a.rec_strand = d_strand.as<uint8_t>(); a.rec_k = d_k.as<int>(); a.rec_sc = d_sc.as<int>();
      a.rec_model = d_model.as<int>(); a.rec_cap = cap;
      P7X_HIP(hipMemsetAsync(d_nrec.as<void>(), 0, 4, s));
      P7X_HIP(hipEventRecord(ev.e0, s));
      size_t at = 0;
      for (size_t g = 0; g < lib->launches.size(); ++g) {
        const SsvBatchLaunch &ln = lib->launches[g];
        for (size_t j0 = 0; j0 < ln.models.size(); j0 += 32768) {          // gridDim.y holds 65,535
          const int nm = (int) std::min<size_t>(32768, ln.models.size() - j0);
          a.models = d_recs.as<const SsvModelRec>() + at + j0;
          if ((st = ssvlong_multi_launch(ln.R, ln.pair, lib->flavour.half, a, nm, max_chunks[g], ctx->num_cu, s)) != P7X_OK) return st;
          if (attempt == 0) g_batch_stats[2]++;
        }
        at += ln.models.size();
      }
      P7X_HIP(hipEventRecord(ev.e1, s));
      int nrec = 0;
      P7X_HIP(hipMemcpyAsync(&nrec, d_nrec.as<void>(), 4, hipMemcpyDeviceToHost, s));
      P7X_HIP(hipStreamSynchronize(s));
      float t = 0; (void) hipEventElapsedTime(&t, ev.e0, ev.e1);
      if (ms) *ms = t;
      g_batch_stats[6] = (int64_t) (t * 1000.0f); g_batch_stats[7] = (int64_t) cells;
      if (nrec > cap) { cap = nrec + 1024; g_batch_stats[5]++; continue; }
      std::vector<long long> pos((size_t) nrec); std::vector<uint8_t> strand((size_t) nrec); std::vector<int> k((size_t) nrec), sc((size_t) nrec), mo((size_t) nrec);
      if (nrec) {
        P7X_HIP(hipMemcpy(pos.data(), d_pos.as<void>(), (size_t) nrec * 8, hipMemcpyDeviceToHost));
        P7X_HIP(hipMemcpy(strand.data(), d_strand.as<void>(), (size_t) nrec, hipMemcpyDeviceToHost));
        P7X_HIP(hipMemcpy(k.data(), d_k.as<void>(), (size_t) nrec * 4, hipMemcpyDeviceToHost));
        P7X_HIP(hipMemcpy(sc.data(), d_sc.as<void>(), (size_t) nrec * 4, hipMemcpyDeviceToHost));
        P7X_HIP(hipMemcpy(mo.data(), d_model.as<void>(), (size_t) nrec * 4, hipMemcpyDeviceToHost));
      }
      for (int i = 0; i < nrec; ++i) {
        if (mo[(size_t) i] < 0 || (size_t) mo[(size_t) i] >= n) { set_error("batched long-target SSV scan: a row of no model"); return P7X_EDEVICE; }
        rows[(size_t) mo[(size_t) i]].push_back(ScanRow{ pos[(size_t) i], strand[(size_t) i], k[(size_t) i], sc[(size_t) i] });
      }
      done = true;
    }
    if (!done) { set_error("batched long-target SSV scan: record buffer could not be sized"); return P7X_EMEM; }
    g_batch_stats[3] += (int64_t) nbatched;
    if ((debug_opt(OPT_TRACE_LONGTARGET) > 0))
      std::fprintf(stderr, "[lt] batched scan: %zu models in %zu launches, %lld positions (%s), kernel %.2f ms\n", nbatched, lib->launches.size(), (long long) L,
                   uploaded ? "uploaded" : "resident", ms ? *ms : 0.0);
  }
  host_parallel_for((int) n, cfg.host_threads, [&](int m) {
    std::sort(rows[(size_t) m].begin(), rows[(size_t) m].end(), [](const ScanRow &x, const ScanRow &y) { return x.strand != y.strand ? x.strand < y.strand : x.pos < y.pos; });
  });
  // the models one launch does not hold: the chained parts of the single-model scan, one model at a time
  for (size_t m = 0; m < n; ++m) {
    if (lib->launch_of[m] >= 0) continue;
    double t = 0.0;
    if ((st = scan_target(cfg, lib->oms[m]->p, ctx, seq1, L, sc_thresh[m], xB[m], strands_mask, rows[m], &t, nullptr, device, resident_key)) != P7X_OK) return st;
    if (ms) *ms += t;
    g_batch_stats[4]++;
  }
  return P7X_OK;
}

// the (block, strand) units of one sequence of L residues, as p7x_search_longtargets counts them for one target
struct ScanUnit { int64_t i, bn; int strand; };
void scan_units(int64_t L, int64_t W, int64_t C, int mask, std::vector<ScanUnit> &units)
{
  units.clear();
  for (int64_t i = 0; i < L; i += W - C) {
    const int64_t bc = i == 0 ? 0 : std::min<int64_t>(C, L - i);
    const int64_t bw = std::min<int64_t>(W, L - i - bc);
    const int64_t bn = bc + bw;
    if (bn <= 0) break;
    for (int strand = 0; strand < 2; ++strand) if (mask & (1 << strand)) units.push_back(ScanUnit{ i, bn, strand });
  }
}

} // namespace

extern "C" {

int p7x_lt_library_create(const p7x_oprofile *const *oms, size_t nmodels, int device, p7x_lt_library **out)
{
  if (!out || (nmodels && !oms)) { set_error("p7x_lt_library_create: bad arguments"); return P7X_EINVAL; }
  *out = nullptr;
  std::unique_ptr<p7x_lt_library> lib;
  const int st = lt_library_build(oms, nmodels, device, lib);
  if (st != P7X_OK) return st;
  *out = lib.release();
  return P7X_OK;
}

void p7x_lt_library_destroy(p7x_lt_library *lib) { delete lib; }

int p7x_scan_longtargets(const p7x_pipeline_cfg *cfg, const p7x_oprofile *const *oms, size_t nmodels, int device,
                         const uint8_t *dsq, int64_t L, const char *name, const char *acc, const char *desc,
                         const int32_t *evalue_window_lengths, p7x_lt_library *lib_in, uint64_t resident_key, p7x_tophits **out)
{
  if (!cfg || !out || !dsq || L < 0 || (nmodels && !oms)) { set_error("p7x_scan_longtargets: bad arguments"); return P7X_EINVAL; }
  if (!cfg->long_targets) { set_error("p7x_scan_longtargets: cfg.long_targets is not set"); return P7X_EINVAL; }
  for (size_t m = 0; m < nmodels; ++m) out[m] = nullptr;
  if (nmodels == 0) return P7X_OK;
  const auto t_begin = std::chrono::steady_clock::now();
  std::unique_ptr<p7x_lt_library> own;
  p7x_lt_library *lib = lib_in;
  int st;
  if (!lt_library_matches(lib, oms, nmodels, device)) {
    if ((st = lt_library_build(oms, nmodels, device, own)) != P7X_OK) return st;
    lib = own.get();
  }
  std::vector<int> max_length(nmodels), sc_thresh(nmodels), xB(nmodels);
  for (size_t m = 0; m < nmodels; ++m)
    if ((st = longtarget_setup(*cfg, oms[m]->p, &max_length[m], &sc_thresh[m], &xB[m])) != P7X_OK) return st;
  const int mask = cfg->strands == P7X_STRAND_TOPONLY ? 1 : (cfg->strands == P7X_STRAND_BOTTOMONLY ? 2 : 3);
  std::vector<std::vector<ScanRow>> rows;
  double scan_ms = 0.0;
  if (L > 0 && (st = scan_target_batched(*cfg, lib, dsq, L, sc_thresh.data(), xB.data(), mask, rows, &scan_ms, resident_key)) != P7X_OK) return st;
  rows.resize(nmodels);
  const auto t_scan = std::chrono::steady_clock::now();
  // seeds: upstream's bookkeeping per (model, block, strand), all of them side by side
  struct Job { size_t m; ScanUnit u; std::vector<int64_t> s3; };
  std::vector<Job> jobs;
  std::vector<ScanUnit> units;
  for (size_t m = 0; m < nmodels; ++m) {
    if (rows[m].empty()) continue;
    scan_units(L, cfg->block_length, max_length[m], mask, units);
    for (const ScanUnit &u : units) jobs.push_back(Job{ m, u, {} });
  }
  host_parallel_for((int) jobs.size(), cfg->host_threads, [&](int j) {
    Job &jb = jobs[(size_t) j];
    block_seeds(oms[jb.m]->p, dsq, L, jb.u.i, jb.u.bn, jb.u.strand, rows[jb.m], sc_thresh[jb.m], xB[jb.m], jb.s3, 0);
  });
  std::vector<std::vector<LongTargetSeed>> seeds(nmodels);
  for (const Job &jb : jobs)
    for (size_t q = 0; q + 2 < jb.s3.size(); q += 3) seeds[jb.m].push_back(LongTargetSeed{ 0, jb.u.i, jb.u.strand, jb.s3[q], (int) jb.s3[q + 1], jb.s3[q + 2] });
  const auto t_seeds = std::chrono::steady_clock::now();
  // the tails: the search's own code per model, several models at a time on threads of their own (a tail waits for its
  // small device batches; its host phases share the workers)
  const int64_t offsets[1] = { 1 }, lengths[1] = { L };
  const char *names[1] = { name ? name : "" }, *accs[1] = { acc ? acc : "" }, *descs[1] = { desc ? desc : "" };
  std::vector<size_t> busy;
  for (size_t m = 0; m < nmodels; ++m) if (!seeds[m].empty()) busy.push_back(m);
  const int usable = cfg->host_threads > 0 ? cfg->host_threads : tophits_usable_cpus();
  const int side = (int) std::max<size_t>(1, std::min<size_t>(std::min<size_t>(busy.size(), 8), (size_t) usable));
  std::atomic<size_t> next{ 0 };
  std::atomic<int> failed{ P7X_OK };
  std::mutex err_mu; std::string err;
  auto tail = [&](size_t m, bool with_device) -> int {
    p7x_pipeline_cfg c = *cfg;
    c.lt_part = 0; c.lt_nparts = 1;
    c.evalue_window_length = evalue_window_lengths ? evalue_window_lengths[m] : cfg->evalue_window_length;
    if (with_device) c.host_threads = std::max(1, usable / side);
    DeviceWindowScorer scorer(oms[m], device, cfg->oa_guard);
    const int rc = longtarget_run_host(c, oms[m], dsq, offsets, lengths, 1, names, accs, descs, seeds[m], &out[m], with_device ? &scorer : nullptr);
    if (rc == P7X_OK && out[m]) {
      out[m]->cfg.host_threads = cfg->host_threads;
      out[m]->ms[P7X_MS_BIAS] = scorer.ms;
    }
    return rc;
  };
  auto worker = [&]() {
    const hipError_t de = hipSetDevice(device);
    if (de != hipSuccess) {
      std::lock_guard<std::mutex> lk(err_mu);
      if (failed.load() == P7X_OK) { failed = P7X_EDEVICE; err = std::string("hipSetDevice: ") + hipGetErrorString(de); }
      return;
    }
    for (;;) {
      const size_t j = next.fetch_add(1);
      if (j >= busy.size() || failed.load() != P7X_OK) break;
      const int rc = tail(busy[j], true);
      if (rc != P7X_OK) { std::lock_guard<std::mutex> lk(err_mu); if (failed.load() == P7X_OK) { failed = rc; err = p7x_last_error(); } }
    }
  };
  {
    std::vector<std::thread> th;
    for (int w = 1; w < side; ++w) th.emplace_back(worker);
    worker();
    for (std::thread &t : th) t.join();
  }
  st = failed.load();
  if (st != P7X_OK) set_error(err);
  // a model without seeds: its empty list, no device
  for (size_t m = 0; st == P7X_OK && m < nmodels; ++m) if (seeds[m].empty()) st = tail(m, false);
  if (st != P7X_OK) { p7x_tophits_destroy_many(out, nmodels); return st; }
  const auto t_end = std::chrono::steady_clock::now();
  // the scan's timing slots on the first list (enum p7x_timing, the long-target meanings): kernel, scan + seeds, tails
  if (out[0]) {
    out[0]->ms[P7X_MS_MSV_KERNEL] = scan_ms;
    out[0]->ms[P7X_MS_MSV] = std::chrono::duration<double, std::milli>(t_seeds - t_begin).count();
    out[0]->ms[P7X_MS_STAGE1] = std::chrono::duration<double, std::milli>(t_scan - t_begin).count();
    out[0]->ms[P7X_MS_HOST_DOMAINDEF] = std::chrono::duration<double, std::milli>(t_end - t_seeds).count();
  }
  return P7X_OK;
}

int64_t p7x_ssv_longtarget_seeds_batch(const p7x_pipeline_cfg *cfg, const p7x_oprofile *const *oms, size_t nmodels, int device,
                                       const uint8_t *dsq, int64_t L, int complement, int64_t *seeds, size_t cap, int64_t *count)
{
  if (!cfg || !oms || !nmodels || !dsq || L <= 0 || !count || (cap && !seeds)) { set_error("p7x_ssv_longtarget_seeds_batch: bad arguments"); return -P7X_EINVAL; }
  std::unique_ptr<p7x_lt_library> lib;
  int st = lt_library_build(oms, nmodels, device, lib);
  if (st != P7X_OK) return -st;
  std::vector<int> max_length(nmodels), sc_thresh(nmodels), xB(nmodels);
  for (size_t m = 0; m < nmodels; ++m)
    if ((st = longtarget_setup(*cfg, oms[m]->p, &max_length[m], &sc_thresh[m], &xB[m])) != P7X_OK) return -st;
  std::vector<std::vector<ScanRow>> rows;
  if ((st = scan_target_batched(*cfg, lib.get(), dsq - 1, L, sc_thresh.data(), xB.data(), complement ? 2 : 1, rows, nullptr, 0)) != P7X_OK) return -st;
  std::vector<std::vector<int64_t>> s3(nmodels);
  host_parallel_for((int) nmodels, cfg->host_threads, [&](int m) {
    block_seeds(oms[m]->p, dsq - 1, L, 0, L, complement ? 1 : 0, rows[(size_t) m], sc_thresh[(size_t) m], xB[(size_t) m], s3[(size_t) m]);
  });
  size_t at = 0;
  for (size_t m = 0; m < nmodels; ++m) {
    count[m] = (int64_t) (s3[m].size() / 3);
    for (size_t q = 0; q < s3[m].size(); ++q, ++at) if (at < cap * 3) seeds[at] = s3[m][q];
  }
  return (int64_t) (at / 3);
}

int p7x_debug_ssv_batch_plan(const int32_t *M, const int32_t *pair_slack, int n, int32_t *launch_of, int32_t *launch_R,
                             int32_t *launch_pair, int64_t *launch_lds, int cap, int64_t *lds_limit)
{
  if (n < 0 || (n && (!M || !pair_slack || !launch_of))) { set_error("p7x_debug_ssv_batch_plan: bad arguments"); return -P7X_EINVAL; }
  std::vector<SsvBatchLaunch> launches; std::vector<int> of;
  ssv_batch_plan(M, pair_slack, n, ssv_flavour(), launches, of);
  for (int i = 0; i < n; ++i) launch_of[i] = of[(size_t) i];
  for (size_t g = 0; g < launches.size() && (int) g < cap; ++g) {
    if (launch_R) launch_R[g] = launches[g].R;
    if (launch_pair) launch_pair[g] = launches[g].pair ? 1 : 0;
    if (launch_lds) launch_lds[g] = (int64_t) ssvlong_lds_bytes(launches[g].R);
  }
  if (lds_limit) *lds_limit = (int64_t) ssvlong_lds_bytes(ssvlong_tile(ssvlong_tile_count() - 1));
  return (int) launches.size();
}

int p7x_debug_ssv_batch_stats(int64_t out[8], int reset)
{
  if (!out) { set_error("p7x_debug_ssv_batch_stats: bad arguments"); return P7X_EINVAL; }
  for (int i = 0; i < 8; ++i) { out[i] = g_batch_stats[i].load(); if (reset) g_batch_stats[i] = 0; }
  return P7X_OK;
}

} // extern "C"
