// p7x_emit.cpp -- sampling sequences from a model on the host: the cumulative tables every emitter draws from, the two
// emitters of the reference's interface (p7_CoreEmit, p7_ProfileEmit; HMMER 3 emit.c) on Easel's generators, and the host
// twin of the device emitter (p7x_emit.hip), which walks the same tables with the same counter-based generator
// (p7x_emitwalk.hpp) and gives the same bytes.
//
// Every choice is an inverse-CDF lookup in double on a table built here once per model: one cumulative row per transition
// row (match, insert, delete), one per match emission row and one per insert emission row, each over its own sum, the
// entry of the last path of positive probability -- and every entry after it -- exactly 1.0, so that a deviate below one
// always finds its path and never one of probability zero.
#include "p7x_emit.hpp"
#include "p7x_host.hpp"
#include "p7x_rng.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace p7x {

// cumulative row of n probabilities over their sum; a row without mass (an unused state) takes its first path
static void cum_row(const float *p, int n, double *out)
{
  double tot = 0.0;
  for (int i = 0; i < n; ++i) if (p[i] > 0.0f) tot += (double) p[i];
  if (!(tot > 0.0) || !std::isfinite(tot)) { for (int i = 0; i < n; ++i) out[i] = 1.0; return; }
  double s = 0.0;
  int last = 0;
  for (int i = 0; i < n; ++i) {
    if (p[i] > 0.0f) { s += (double) p[i]; last = i; }
    out[i] = s / tot;
  }
  for (int i = last; i < n; ++i) out[i] = 1.0;
}

static int build_emit_model(const p7x_hmm_view *h, p7x_emit_model &em)
{
  const Alphabet &abc = Alphabet::get(h->abc_type);
  const int M = h->M, K = abc.K, S = emit_stride(K);
  em.M = M; em.K = K; em.abc_type = h->abc_type;
  em.tab.assign((size_t) (M + 1) * S, 1.0);
  em.occ.assign((size_t) M + 1, 0.0);
  // the probability that a path visits M_k / D_k, and the residues it emits (an insert run of I_k: tMI / (1 - tII))
  double pm = 1.0, pd = 0.0, elen = 0.0;
  for (int k = 0; k <= M; ++k) {
    const float *t = h->t + (size_t) k * 7;
    double *row = em.tab.data() + (size_t) k * S, c[3];
    cum_row(t, 3, c);     row[0] = c[0]; row[1] = c[1];
    cum_row(t + 3, 2, c); row[2] = c[0];
    cum_row(t + 5, 2, c); row[3] = c[0];
    cum_row(h->mat + (size_t) k * K, K, row + kEmitTrans);
    cum_row(h->ins + (size_t) k * K, K, row + kEmitTrans + K);
    const double mm = row[0], mi = row[1] - row[0], md = 1.0 - row[1], im = row[2], dm = row[3];
    em.occ[(size_t) k] = pm;
    if (k > 0) elen += pm;
    if (pm * mi > 0.0) {
      if (!(im > 0.0)) { set_error("the model cannot be sampled: insert state " + std::to_string(k) + " is entered and never left"); return P7X_EINVAL; }
      elen += pm * mi / im;
    }
    const double nm = pm * (mm + mi) + pd * dm, nd = pm * md + pd * (1.0 - dm);
    pm = nm; pd = nd;
  }
  if (!(elen > 0.0) || !std::isfinite(elen)) { set_error("the model cannot be sampled: it emits no residue"); return P7X_EINVAL; }
  em.expected_length = elen;
  return P7X_OK;
}

int32_t emit_default_cap(const p7x_emit_model &em)
{
  const int forced = debug_opt(OPT_EMIT_CAP);
  int64_t cap = forced > 0 ? forced : (int64_t) std::ceil(2.0 * em.expected_length);
  cap = std::max<int64_t>(4, std::min<int64_t>((cap + 3) / 4 * 4, kEmitMaxLen));
  return (int32_t) cap;
}

int emit_workspace_bytes(int64_t n, int64_t cap, bool traces, int64_t budget, int64_t *bytes)
{
  if (n < 0 || cap < 4 || cap % 4 != 0) { set_error("emit workspace: bad arguments"); return P7X_EINVAL; }
  // per sequence: a slot of residues (with traces one of states and one of 32-bit nodes as well), and length, attempt, status
  // and 64-bit offset; the packed output is no larger than the slots it is compacted from, plus the sentinels
  const int64_t per_slot = cap * (traces ? 6 : 1), per_seq = 2 * per_slot + (traces ? 6 : 1) + 3 * 4 + 8;
  if (n > 0 && per_seq > (INT64_MAX - 4096) / n) { set_error("emit workspace: " + std::to_string(n) + " sequences of " + std::to_string(cap) + " residues do not fit"); return P7X_EMEM; }
  const int64_t need = n * per_seq + 4096;
  if (bytes) *bytes = need;
  if (budget >= 0 && need > budget) {
    set_error("emit workspace: " + std::to_string(need) + " bytes for " + std::to_string(n) + " sequences of up to " + std::to_string(cap) +
              " residues, " + std::to_string(budget) + " available: emit fewer sequences per call");
    return P7X_EMEM;
  }
  return P7X_OK;
}

int emit_status_error(int status, int64_t seq)
{
  if (status == EMIT_TOO_LONG) set_error("sequence " + std::to_string(seq) + " grew beyond " + std::to_string(kEmitMaxLen) + " residues: the model's insert states are all but closed");
  else set_error("sequence " + std::to_string(seq) + ": " + std::to_string(kEmitMaxAttempts) + " paths in a row emitted nothing");
  return P7X_ERANGE;
}

// ---------------------------------------------------------------- the host twin of the device emitter
namespace {
struct ChunkSink {
  std::vector<uint8_t> *dsq; std::vector<int8_t> *st; std::vector<int32_t> *node;
  void put(int, int x, int s, int k)
  {
    dsq->push_back((uint8_t) x);
    if (st) { st->push_back((int8_t) s); node->push_back(k); }
  }
};
struct Chunk { std::vector<uint8_t> dsq; std::vector<int8_t> st; std::vector<int32_t> node; int status = EMIT_OK; int64_t bad = 0; };
constexpr int64_t kChunk = 1024;
}

int emit_block_host(const p7x_emit_model &em, int64_t n, uint64_t seed, bool traces, int threads, p7x_emitted &out)
{
  out = p7x_emitted();
  out.n = n; out.traces = traces; out.cap = emit_default_cap(em);
  out.lengths.assign((size_t) n, 0); out.attempts.assign((size_t) n, 0); out.offsets.assign((size_t) n, 0);
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  std::vector<Chunk> chunks((size_t) nchunks);
  const uint32_t k0 = (uint32_t) seed, k1 = (uint32_t) (seed >> 32);
  host_parallel_for((int) nchunks, threads, [&](int c) {
    Chunk &ch = chunks[(size_t) c];
    ChunkSink sink{ &ch.dsq, traces ? &ch.st : nullptr, traces ? &ch.node : nullptr };
    for (int64_t i = c * kChunk; i < std::min(n, (c + 1) * kChunk) && ch.status == EMIT_OK; ++i) {
      uint32_t a = 0;
      const int st = emit_walk(em.tab.data(), em.M, em.K, k0, k1, (uint64_t) i, 0u, sink, &out.lengths[(size_t) i], &a);
      out.attempts[(size_t) i] = (int32_t) a;
      if (st != EMIT_OK) { ch.status = st; ch.bad = i; }
    }
  });
  for (const Chunk &ch : chunks) if (ch.status != EMIT_OK) return emit_status_error(ch.status, ch.bad);
  int64_t pos = 1;
  for (int64_t i = 0; i < n; ++i) {
    out.offsets[(size_t) i] = pos; pos += out.lengths[(size_t) i] + 1;
    if (out.lengths[(size_t) i] > out.cap) ++out.nredrawn;
  }
  out.nres = pos - 1 - n;
  out.dsq.assign((size_t) pos, 255);
  if (traces) { out.st.assign((size_t) pos, 0); out.node.assign((size_t) pos, 0); }
  host_parallel_for((int) nchunks, threads, [&](int c) {
    const Chunk &ch = chunks[(size_t) c];
    size_t src = 0;
    for (int64_t i = c * kChunk; i < std::min(n, (c + 1) * kChunk); ++i) {
      const size_t L = (size_t) out.lengths[(size_t) i], o = (size_t) out.offsets[(size_t) i];
      std::memcpy(out.dsq.data() + o, ch.dsq.data() + src, L);
      if (traces) { std::memcpy(out.st.data() + o, ch.st.data() + src, L); std::memcpy(out.node.data() + o, ch.node.data() + src, L * sizeof(int32_t)); }
      src += L;
    }
  });
  return P7X_OK;
}

// ---------------------------------------------------------------- the reference's emitters, on Easel's generators
namespace {
struct OutBuf {
  uint8_t *dsq; int8_t *st; int32_t *node; size_t cap; int64_t n = 0;
  void put(int x, int s, int k)
  {
    if ((size_t) n < cap) { dsq[n] = (uint8_t) x; if (st) st[n] = (int8_t) s; if (node) node[n] = k; }
    ++n;
  }
};
}

// p7_CoreEmit: one deviate per transition, one per residue; a path that emits nothing is drawn again
static int core_emit(const p7x_emit_model &em, EaselRng &r, OutBuf &out)
{
  const int M = em.M, K = em.K, S = emit_stride(K);
  for (int attempt = 0; attempt < kEmitMaxAttempts; ++attempt) {
    int k = 0, st = EMIT_ST_M;
    for (;;) {
      const double u = r.next();
      const double *t = em.tab.data() + (size_t) k * S;
      if (st == EMIT_ST_M)      { if (u < t[0]) { st = EMIT_ST_M; ++k; } else if (u < t[1]) st = EMIT_ST_I; else { st = EMIT_ST_D; ++k; } }
      else if (st == EMIT_ST_I) { if (u < t[2]) { st = EMIT_ST_M; ++k; } }
      else                      { ++k; if (u < t[3]) st = EMIT_ST_M; }
      if (k > M) break;
      if (st != EMIT_ST_D) {
        if (out.n >= kEmitMaxLen) return emit_status_error(EMIT_TOO_LONG, 0);
        const double *e = em.tab.data() + (size_t) k * S + kEmitTrans + (st == EMIT_ST_I ? K : 0);
        out.put(emit_pick(e, K, r.next()), st, k);
      }
    }
    if (out.n > 0) return P7X_OK;
  }
  return emit_status_error(EMIT_NEVER, 0);
}

// p7_ProfileEmit through the local multihit profile of length model L: S N.. B (core fragment) E (J.. B (fragment) E)* C.. T.
// N, J and C emit from the background on their loops (L / (L + 3) each); a fragment enters at match state k with the
// profile's entry probability occ[k] / Z times its M - k + 1 exits and leaves from a node drawn evenly from k .. M
// (upstream's sample_endpoints: the implicit probabilistic model of local alignment); inside it the core model's own
// transitions decide; E goes on to J or to C with one half each.
static int profile_emit(const p7x_emit_model &em, int L, const float *bg_f, EaselRng &r, OutBuf &out, int32_t counts[2])
{
  const int M = em.M, K = em.K, S = emit_stride(K);
  std::vector<double> bg((size_t) K), entry((size_t) M + 1, 0.0);
  cum_row(bg_f, K, bg.data());
  {
    double z = 0.0, s = 0.0;
    int last = 1;
    for (int k = 1; k <= M; ++k) z += em.occ[(size_t) k] * (double) (M - k + 1);
    if (!(z > 0.0)) { set_error("the profile has no entry: no match state is ever occupied"); return P7X_EINVAL; }
    for (int k = 1; k <= M; ++k) { const double p = em.occ[(size_t) k] * (double) (M - k + 1); if (p > 0.0) { s += p; last = k; } entry[(size_t) k] = s / z; }
    for (int k = last; k <= M; ++k) entry[(size_t) k] = 1.0;
  }
  const double ploop = (double) L / ((double) L + 3.0);
  counts[0] = counts[1] = 0;
  auto loop_state = [&]() -> int {              // N, J or C: background residues until the state moves on
    while (r.next() < ploop) {
      if (out.n >= kEmitMaxLen) return emit_status_error(EMIT_TOO_LONG, 0);
      out.put(emit_pick(bg.data(), K, r.next()), 0, 0);
    }
    return P7X_OK;
  };
  int rc = loop_state();                        // N
  if (rc != P7X_OK) return rc;
  for (;;) {
    int k = 1 + emit_pick(entry.data() + 1, M, r.next());
    const int kend = k + std::min(M - k, (int) (r.next() * (double) (M - k + 1)));
    int st = EMIT_ST_M;
    ++counts[1];
    for (;;) {
      if (st != EMIT_ST_D) {
        if (out.n >= kEmitMaxLen) return emit_status_error(EMIT_TOO_LONG, 0);
        const double *e = em.tab.data() + (size_t) k * S + kEmitTrans + (st == EMIT_ST_I ? K : 0);
        out.put(emit_pick(e, K, r.next()), st, k);
        ++counts[0];
      }
      if (st != EMIT_ST_I && k == kend) break;  // M or D of the last node of the fragment: E
      const double u = r.next();
      const double *t = em.tab.data() + (size_t) k * S;
      if (st == EMIT_ST_M)      { if (u < t[0]) { st = EMIT_ST_M; ++k; } else if (u < t[1]) st = EMIT_ST_I; else { st = EMIT_ST_D; ++k; } }
      else if (st == EMIT_ST_I) { if (u < t[2]) { st = EMIT_ST_M; ++k; } }
      else                      { ++k; if (u < t[3]) st = EMIT_ST_M; }
    }
    if (r.next() < 0.5) break;                  // E -> C
    if ((rc = loop_state()) != P7X_OK) return rc;       // E -> J
  }
  return loop_state();                          // C
}

} // namespace p7x

using namespace p7x;

extern "C" {

int p7x_emit_model_create(const p7x_hmm_view *hmm, p7x_emit_model **out)
{
  if (!hmm || !out || hmm->M < 1 || !hmm->t || !hmm->mat || !hmm->ins) { set_error("p7x_emit_model_create: bad arguments"); return P7X_EINVAL; }
  if (hmm->abc_type != P7X_AMINO && hmm->abc_type != P7X_DNA && hmm->abc_type != P7X_RNA) { set_error("unknown alphabet"); return P7X_EINVAL; }
  auto *em = new p7x_emit_model();
  const int st = build_emit_model(hmm, *em);
  if (st != P7X_OK) { delete em; return st; }
  *out = em;
  return P7X_OK;
}

void p7x_emit_model_destroy(p7x_emit_model *em) { delete em; }

int p7x_emit_model_info(const p7x_emit_model *em, double *expected_length, int32_t *cap)
{
  if (!em) { set_error("p7x_emit_model_info: bad arguments"); return P7X_EINVAL; }
  if (expected_length) *expected_length = em->expected_length;
  if (cap) *cap = emit_default_cap(*em);
  return P7X_OK;
}

int p7x_emit_core(const p7x_emit_model *em, int generator, uint32_t *state, uint8_t *dsq, int8_t *st, int32_t *node, size_t cap, int64_t *len)
{
  if (!em || !state || !len || (cap && !dsq)) { set_error("p7x_emit_core: bad arguments"); return P7X_EINVAL; }
  if (generator != P7X_RNG_MERSENNE && generator != P7X_RNG_FAST) { set_error("unknown generator"); return P7X_EINVAL; }
  EaselRng r;
  r.load(generator, state);
  OutBuf out{ dsq, st, node, cap };
  const int rc = core_emit(*em, r, out);
  if (rc != P7X_OK) return rc;
  r.save(state);
  *len = out.n;
  return P7X_OK;
}

int p7x_emit_profile(const p7x_emit_model *em, int32_t L, const float *bg_f, int generator, uint32_t *state, uint8_t *dsq, size_t cap,
                     int64_t *len, int32_t *counts)
{
  if (!em || !bg_f || !state || !len || (cap && !dsq) || L < 0) { set_error("p7x_emit_profile: bad arguments"); return P7X_EINVAL; }
  if (generator != P7X_RNG_MERSENNE && generator != P7X_RNG_FAST) { set_error("unknown generator"); return P7X_EINVAL; }
  EaselRng r;
  r.load(generator, state);
  OutBuf out{ dsq, nullptr, nullptr, cap };
  int32_t c[2];
  const int rc = profile_emit(*em, L, bg_f, r, out, c);
  if (rc != P7X_OK) return rc;
  r.save(state);
  *len = out.n;
  if (counts) { counts[0] = c[0]; counts[1] = c[1]; }
  return P7X_OK;
}

int p7x_emit_block_host(const p7x_emit_model *em, int64_t n, uint64_t seed, int want_traces, int threads, p7x_emitted **out)
{
  if (!em || !out) { set_error("p7x_emit_block_host: bad arguments"); return P7X_EINVAL; }
  if (n < 0) { set_error("the number of sequences to emit is negative"); return P7X_EINVAL; }
  auto *blk = new p7x_emitted();
  const int st = emit_block_host(*em, n, seed, want_traces != 0, threads, *blk);
  if (st != P7X_OK) { delete blk; return st; }
  *out = blk;
  return P7X_OK;
}

int64_t p7x_emitted_info(const p7x_emitted *b, int which)
{
  if (!b) return -1;
  switch (which) {
    case 0: return b->n;
    case 1: return b->nres;
    case 2: return b->cap;
    case 3: return b->nredrawn;
    case 4: return b->on_device;
    case 5: return b->traces ? 1 : 0;
    case 6: return (int64_t) b->kernel_us;
    default: return -1;
  }
}

int p7x_emitted_copy(const p7x_emitted *b, uint8_t *dsq, int64_t *offsets, int32_t *lengths, int32_t *attempts, int8_t *st, int32_t *node)
{
  if (!b || !dsq || (b->n && (!offsets || !lengths))) { set_error("p7x_emitted_copy: bad arguments"); return P7X_EINVAL; }
  if ((st || node) && !b->traces) { set_error("p7x_emitted_copy: the block was emitted without traces"); return P7X_EINVAL; }
  std::memcpy(dsq, b->dsq.data(), b->dsq.size());
  if (b->n) {
    std::memcpy(offsets, b->offsets.data(), sizeof(int64_t) * (size_t) b->n);
    std::memcpy(lengths, b->lengths.data(), sizeof(int32_t) * (size_t) b->n);
    if (attempts) std::memcpy(attempts, b->attempts.data(), sizeof(int32_t) * (size_t) b->n);
  }
  if (st) std::memcpy(st, b->st.data(), b->st.size());
  if (node) std::memcpy(node, b->node.data(), sizeof(int32_t) * b->node.size());
  return P7X_OK;
}

void p7x_emitted_destroy(p7x_emitted *b) { delete b; }

int p7x_debug_philox(const uint32_t *key2, const uint32_t *ctr4, uint32_t *out4)
{
  if (!key2 || !ctr4 || !out4) { set_error("p7x_debug_philox: bad arguments"); return P7X_EINVAL; }
  const Philox4 r = philox4x32_10(key2[0], key2[1], ctr4[0], ctr4[1], ctr4[2], ctr4[3]);
  std::memcpy(out4, r.v, sizeof(r.v));
  return P7X_OK;
}

int p7x_debug_emit_bytes(int64_t n, int64_t cap, int traces, int64_t budget, int64_t *bytes)
{
  return emit_workspace_bytes(n, cap, traces != 0, budget, bytes);
}

} // extern "C"
