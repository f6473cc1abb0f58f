// p7x_tracealign.cpp -- hmmalign (upstream tracealign.c: p7_tracealign_computeTraces, p7_tracealign_Seqs; pyhmmer
// plan7.TraceAligner, hmmer/_hmmalign.py): optimal-accuracy traces of whole sequences against one profile, on the device
// (p7x_align.hip, driven through the envelope driver of p7x_envscore.hip) with the host twin (p7x_domaindef.cpp,
// align_trace_upstream) for every sequence the device flags; the multiple alignment built from the traces; and its
// Stockholm text as Easel's writer prints it (esl_msafile_stockholm.c).
#include "p7x_wave.hpp"
#include "p7x_host.hpp"
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace p7x;

namespace p7x { int vit_pick_C(int M); }

struct p7x_traces {
  int32_t M = 0;
  std::vector<AlignTrace> tr;          // forward order, float posteriors
  std::vector<int32_t> L, status;      // status: the device's status word (0 for the host twin's traces)
  std::vector<uint8_t> origin;         // P7X_TRACE_* bits
  int64_t nflagged = 0;                // device traces the host twin repeated
  int64_t nrounds = 0;                 // device rounds (launches of the alignment kernel)
  int64_t work_bytes = 0;              // the largest device workspace a round laid out
  int64_t nlogspace = 0;               // sequences aligned by the float64 log-space path (P7X_ALIGN_LOGSPACE)
  int64_t nlogspace_flagged = 0;       // ... of those, device traces the host log twin repeated
};

struct p7x_msa {
  int64_t alen = 0;
  std::vector<std::string> aseq, pp;   // pp[idx] empty: that row has no posterior annotation
  std::string pp_cons, rf, ss_cons;
  std::vector<std::string> name, acc, desc;   // per row; filled by p7x_tophits_to_msa only
  std::string msa_name;
  std::vector<uint8_t> codes;          // P7X_MSA_DIGITIZE: the rows as digital codes, [n][alen] (p7x_msa_codes)
};

namespace {

// Near-tie guard of the device's optimal-accuracy choices: the envelope kernel's default (p7x_pipeline_cfg.oa_guard)
constexpr float kAlignGuard = 4e-6f;

char encode_pp(float p) { return (p + 0.05 >= 1.0) ? '*' : (char) ((int) ((p + 0.05) * 10.0) + '0'); }     // p7_alidisplay_EncodePostProb

// a PP_cons mean within align_pp_guard(M) of a digit boundary (p7x_kernels.hpp)
bool pp_near_boundary(double mean, int M)
{
  const double v = ((double) (float) mean + 0.05) * 10.0;
  return std::fabs(v - std::nearbyint(v)) < (double) align_pp_guard(M) * 10.0;
}

// the host twin for a set of sequences, in parallel; the error of the lowest sequence index wins (that index in *bad).
// twin: the scaled float32 engines in upstream's order, the same giving up (P7X_ERANGE) as soon as Backward leaves Forward's
// scale factors, or the float64 log-space twin.  each: the sequences' own statuses, in <which>'s order.
enum class Twin { Scaled, ScaledOrLeave, Log };
int host_traces(const Profile &p, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, const std::vector<int> &which,
                std::vector<AlignTrace> &out, int64_t *bad, int threads = 0, Twin twin = Twin::Scaled, std::vector<int> *each = nullptr)
{
  std::vector<int> st(which.size(), P7X_OK);
  const int nthreads = std::max(1, std::min<int>(threads > 0 ? threads : tophits_usable_cpus(), (int) which.size()));
  host_parallel_for((int) which.size(), nthreads, [&](int w) {
    const int t = which[(size_t) w];
    std::vector<uint8_t> seq((size_t) lengths[t] + 2, 255);           // 1-based, sentinel-framed
    std::memcpy(seq.data() + 1, dsq + offsets[t], (size_t) lengths[t]);
    st[(size_t) w] = twin == Twin::Log ? align_trace_logspace(p, seq.data(), lengths[t], out[(size_t) t])
                                       : align_trace_upstream(p, seq.data(), lengths[t], out[(size_t) t], 0, twin == Twin::ScaledOrLeave);
  });
  // the failure reported is that of the lowest input index, whatever order <which> lists the sequences in (the device path
  // lists what it flagged longest first, the test seam in input order: both name the same sequence)
  int first = P7X_OK;
  for (size_t w = 0; w < which.size(); ++w)
    if (st[w] != P7X_OK && (first == P7X_OK || which[w] < *bad)) { *bad = which[w]; first = st[w]; }
  if (each) *each = std::move(st);
  return first;
}

int report_host_error(int st, int64_t idx, int L)
{
  char buf[256];
  if (st == P7X_ERANGE)
    std::snprintf(buf, sizeof buf, "hmmalign: posterior decoding overflowed on sequence %lld (L = %d); upstream's generic-DP fallback is not implemented", (long long) idx, L);
  else
    std::snprintf(buf, sizeof buf, "hmmalign: the optimal-accuracy traceback failed on sequence %lld (L = %d)", (long long) idx, L);
  set_error(buf);
  return st;
}

// esl_abc_DigitizeSymbol over the input map Easel builds for the alphabet: both letter cases, '_' and '.' for the gap, and
// the nucleic synonyms (T / U for each other, X for N, I for A); 255 = not a symbol
struct InputMap {
  uint8_t code[256];
  explicit InputMap(int abc_type)
  {
    const Alphabet &abc = Alphabet::get(abc_type);
    std::memset(code, 255, sizeof code);
    for (int x = 0; x < abc.Kp; ++x) {
      code[(unsigned char) abc.sym[x]] = (uint8_t) x;
      code[(unsigned char) std::tolower((unsigned char) abc.sym[x])] = (uint8_t) x;
    }
    auto equiv = [&](char c, char to) { code[(unsigned char) c] = code[(unsigned char) std::tolower((unsigned char) c)] = code[(unsigned char) to]; };
    equiv('_', '-'); equiv('.', '-');
    if (abc_type != P7X_AMINO) { equiv(abc_type == P7X_RNA ? 'T' : 'U', abc_type == P7X_RNA ? 'U' : 'T'); equiv('X', 'N'); equiv('I', 'A'); }
  }
  static const InputMap &get(int abc_type)
  {
    static const InputMap amino(P7X_AMINO), dna(P7X_DNA), rna(P7X_RNA);
    return abc_type == P7X_AMINO ? amino : (abc_type == P7X_RNA ? rna : dna);
  }
};

float decode_pp(char c)       // p7_alidisplay_DecodePostProb
{
  if (c == '*') return 1.0f;
  if (c == '.') return 0.0f;
  return (float) ((float) (c - '0') / 10.);
}

// p7_alidisplay_Backconvert (see include/p7x.h); steps as p7_trace_AppendWithPP stores them
int backconvert(int abc_type, const char *model, const char *aseq, const char *ppline, int hmmfrom, int hmmto, int64_t sqfrom, int64_t sqto,
                int64_t L, bool whole, std::vector<int8_t> &st, std::vector<int32_t> &tk, std::vector<int32_t> &ti, std::vector<float> &tpp,
                std::vector<uint8_t> &dsq)
{
  enum { tM = 1, tD = 2, tI = 3, tS = 4, tN = 5, tB = 6, tE = 7, tC = 8, tT = 9 };
  const Alphabet &abc = Alphabet::get(abc_type);
  const InputMap &in = InputMap::get(abc_type);
  const size_t n = std::strlen(model);
  if (n == 0 || std::strlen(aseq) != n || (ppline && std::strlen(ppline) != n)) { set_error("back-conversion: the lines of the alignment display differ in length"); return P7X_EINVAL; }
  auto is_residue = [&](uint8_t x) { return x < abc.K || (x > abc.K && x < abc.Kp - 2); };
  st.clear(); tk.clear(); ti.clear(); tpp.clear(); dsq.clear();
  auto append = [&](int s, int k, int64_t i, float p) { st.push_back((int8_t) s); tk.push_back(k); ti.push_back((int32_t) i); tpp.push_back(p); };
  if (whole && !(sqfrom >= 1 && sqfrom <= sqto && sqto <= L && L <= INT32_MAX)) {
    set_error("back-conversion to a trace of the whole target needs 1 <= sqfrom <= sqto <= L"); return P7X_EINVAL;
  }
  const int64_t shift = whole ? sqfrom - 1 : 0;
  append(tS, 0, 0, 0.0f);
  append(tN, 0, 0, 0.0f);
  for (int64_t r = 1; r <= shift; ++r) append(tN, 0, r, 1.0f);
  append(tB, 0, 0, 0.0f);
  int k = hmmfrom;
  int64_t i = 1;
  for (size_t a = 0; a < n; ++a) {
    const uint8_t xm = in.code[(unsigned char) model[a]], xa = in.code[(unsigned char) aseq[a]];
    if (xm == 255 || xa == 255) {
      set_error(std::string("back-conversion: '") + (xm == 255 ? model[a] : aseq[a]) + "' in column " + std::to_string(a + 1) + " is not a symbol of the alphabet");
      return P7X_EINVAL;
    }
    if (ppline && ppline[a] != '*' && ppline[a] != '.' && !std::isdigit((unsigned char) ppline[a])) { set_error("back-conversion: the posterior line holds something else than digits, '*' and '.'"); return P7X_EINVAL; }
    const int cur = is_residue(xm) ? (is_residue(xa) ? tM : tD) : tI;
    const float p = ppline ? decode_pp(ppline[a]) : 0.0f;
    switch (cur) {
      case tM: append(tM, k, i + shift, p); dsq.push_back(xa); k++; i++; break;
      case tI:
        if (xa == abc.K) { set_error("back-conversion: column " + std::to_string(a + 1) + " of the display has neither a model position nor a residue"); return P7X_EINVAL; }
        append(tI, k - 1, i + shift, p); dsq.push_back(xa); i++; break;     // the insert state of the node before it (k is the next node's)
      default: append(tD, k, 0, 0.0f); k++; break;
    }
  }
  append(tE, 0, 0, 0.0f);
  append(tC, 0, 0, 0.0f);
  if (whole) for (int64_t r = sqto + 1; r <= L; ++r) append(tC, 0, r, 1.0f);
  append(tT, 0, 0, 0.0f);
  size_t nres = 0;                                   // upstream's first pass: what is not a gap is a residue of the subsequence
  for (size_t a = 0; a < n; ++a) nres += in.code[(unsigned char) aseq[a]] != abc.K ? 1 : 0;
  if (k != hmmto + 1 || (size_t) (i - 1) != nres) { set_error("back-conversion: the display's coordinates do not match its columns"); return P7X_EINVAL; }
  if (whole && sqto - sqfrom + 1 != (int64_t) nres) { set_error("back-conversion: sqfrom..sqto does not span the display's residues"); return P7X_EINVAL; }
  return P7X_OK;
}

struct SeqdbDeleter { void operator()(p7x_seqdb *db) const { p7x_seqdb_destroy(db); } };

// Device path: sequences longest first, in rounds of lengths within a factor of two (the workspace of a wavefront is sized
// for the longest sequence of its round); the envelope driver runs each round on a leased stream within the HBM budget.
// logq (the log-space path is on): the sequences whose decoding overflowed (status bit 1) -- the log kernel's, not the
// scaled twin's.
int device_traces(const p7x_oprofile *om, DeviceCtx *ctx, const p7x_seqdb *sdb, const int32_t *lengths, size_t n,
                  p7x_traces &out, std::vector<int> &redo, std::vector<int> *logq)
{
  const Profile &p = om->p;
  int st = P7X_OK;
  std::vector<int> order;
  for (size_t t = 0; t < n; ++t) if (lengths[t] > 0) order.push_back((int) t);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return lengths[x] > lengths[y]; });
  const int C = vit_pick_C(p.M);
  if (C <= 0) { set_error(model_too_long("hmmalign: model too long for the alignment kernel")); return P7X_EINVAL; }
  const size_t budget = align_budget_bytes();
  std::vector<EnvelopeRequest> req;
  std::vector<int32_t> targets;
  std::vector<std::vector<EnvelopeResult>> res;
  for (size_t pos = 0; pos < order.size();) {
    const int first = order[pos], Lr = lengths[first];
    if (env_work_floats(C, Lr) * 4 * (size_t) env_waves(C) > budget) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "hmmalign: sequence %d (L = %d) alone does not fit the alignment workspace (%.1f GB)", first, Lr, budget / 1e9);
      set_error(buf);
      return P7X_EMEM;
    }
    size_t end = pos;
    while (end < order.size() && 2 * (int64_t) lengths[order[end]] >= Lr) ++end;
    req.clear(); targets.clear();
    for (size_t r = pos; r < end; ++r) {
      req.push_back(EnvelopeRequest{ (int) (r - pos), 1, lengths[order[r]] });
      targets.push_back(order[r]);
    }
    EnvelopeJob job;
    job.om = om; job.req = &req; job.targets = &targets;
    auto scorer = make_device_align_scorer(ctx, sdb, kAlignGuard);     // one lease per round (released when it ends)
    if ((st = scorer->begin({ job })) != P7X_OK) return st;
    if ((st = scorer->wait(res)) != P7X_OK) return st;
    out.nrounds++;
    out.work_bytes = std::max<int64_t>(out.work_bytes, (int64_t) scorer->workspace_bytes());
    for (size_t r = 0; r < req.size(); ++r) {
      const EnvelopeResult &e = res[0][r];
      const int t = targets[r];
      out.status[(size_t) t] = e.status;
      if (logq && (e.status & 2)) { logq->push_back(t); continue; }
      if (e.status != 0) { redo.push_back(t); continue; }     // a near-tie, a posterior digit in the guard band, a failure
      AlignTrace &a = out.tr[(size_t) t];
      align_trace_from_device(e.ta, e.ti, e.tp, e.ntrace, a);
      a.fwdsc = e.envsc; a.oasc = e.oasc;
      out.origin[(size_t) t] = P7X_TRACE_HAS_PP | P7X_TRACE_DEVICE;
    }
    pos = end;
  }
  return P7X_OK;
}

} // namespace

extern "C" {

int p7x_tracealign_compute(const p7x_oprofile *om, int device, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths,
                           size_t n, int host_threads, p7x_traces **out)
{
  return p7x_tracealign_compute_opts(om, device, dsq, offsets, lengths, n, host_threads, 0, out);
}

int p7x_tracealign_compute_opts(const p7x_oprofile *om, int device, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths,
                                size_t n, int host_threads, int flags, p7x_traces **out)
{
  if (!om || !out || (n && (!dsq || !offsets || !lengths))) { set_error("p7x_tracealign_compute: bad arguments"); return P7X_EINVAL; }
  *out = nullptr;
  for (size_t t = 0; t < n; ++t) if (lengths[t] < 0) { set_error("p7x_tracealign_compute: negative sequence length"); return P7X_EINVAL; }
  const Profile &p = om->p;
  const bool everything = debug_opt(OPT_ALIGN_LOGSPACE) > 0;               // test seam: every non-empty sequence takes the log-space path
  const bool logspace = (flags & P7X_ALIGN_LOGSPACE) != 0 || everything;
  const bool on_host = debug_opt(OPT_HOST_ALIGN) > 0;                      // test seam: every trace from the host twins
  auto tr = std::make_unique<p7x_traces>();
  tr->M = p.M;
  tr->tr.assign(n, AlignTrace{});
  tr->L.assign(lengths, lengths + n);
  tr->status.assign(n, 0);
  tr->origin.assign(n, P7X_TRACE_HAS_PP);
  // redo: the scaled host twin's; logq: the log kernel's; logredo: the host log twin's
  std::vector<int> redo, logq, logredo, all;
  for (size_t t = 0; t < n; ++t) if (lengths[t] > 0) all.push_back((int) t);
  DeviceCtx *ctx = nullptr;
  std::unique_ptr<p7x_seqdb, SeqdbDeleter> db;
  if (on_host) {
    (everything ? logredo : redo) = all;
  } else {
    int st = get_ctx(device, &ctx);
    if (st != P7X_OK) return st;
    p7x_seqdb *raw = nullptr;
    if ((st = p7x_seqdb_create(device, p.abc_type, dsq, offsets, lengths, n, &raw)) != P7X_OK) return st;
    db.reset(raw);
    if (everything) logq = all;
    else {
      if ((st = device_traces(om, ctx, db.get(), lengths, n, *tr, redo, logspace ? &logq : nullptr)) != P7X_OK) return st;
      tr->nflagged = (int64_t) redo.size();
      if (logspace) {
        // The other trigger: Backward on its own scale factors.  The scaled kernel aligns such a sequence (and degrades
        // from about 80 nats per domain) without saying so, so the traces it kept are checked on the host, rows only.
        // Few need it: Backward's B cell of row i is at most Forward's total / (ploop^i pmove) <= total x 5 (L + 2), so
        // xB > 1e16 takes a Forward score above ln 1e16 - ln(5 (L + 2)); half a nat of margin for float32.
        std::vector<int> cand;
        for (int t : all)
          if (tr->status[(size_t) t] == 0 && tr->tr[(size_t) t].fwdsc >= 36.84f - std::log(5.0f * ((float) lengths[t] + 2.0f)) - 0.5f) cand.push_back(t);
        std::vector<char> own(cand.size(), 0);
        const int nthreads = std::max(1, std::min<int>(host_threads > 0 ? host_threads : tophits_usable_cpus(), (int) cand.size()));
        host_parallel_for((int) cand.size(), nthreads, [&](int w) {
          const int t = cand[(size_t) w];
          std::vector<uint8_t> seq((size_t) lengths[t] + 2, 255);
          std::memcpy(seq.data() + 1, dsq + offsets[t], (size_t) lengths[t]);
          own[(size_t) w] = align_leaves_forward_scales(p, seq.data(), lengths[t]) ? 1 : 0;
        });
        for (size_t w = 0; w < cand.size(); ++w)
          if (own[w]) { const int t = cand[w]; tr->tr[(size_t) t] = AlignTrace{}; tr->origin[(size_t) t] = P7X_TRACE_HAS_PP; logq.push_back(t); }
      }
    }
  }
  int64_t bad = -1;
  if (!logspace) {
    const int st = host_traces(p, dsq, offsets, lengths, redo, tr->tr, &bad, host_threads);
    if (st != P7X_OK) return report_host_error(st, bad, lengths[bad]);
  } else if (!redo.empty()) {
    // what the scaled twin cannot finish -- Backward on its own scale factors, a range error -- is the log twin's
    std::vector<int> each;
    (void) host_traces(p, dsq, offsets, lengths, redo, tr->tr, &bad, host_threads, Twin::ScaledOrLeave, &each);
    for (size_t w = 0; w < redo.size(); ++w) {
      if (each[w] == P7X_ERANGE) logredo.push_back(redo[w]);
      else if (each[w] != P7X_OK) return report_host_error(each[w], redo[w], lengths[redo[w]]);
    }
  }
  if (!logq.empty()) {
    std::stable_sort(logq.begin(), logq.end(), [&](int x, int y) { return lengths[x] > lengths[y]; });
    const int st = device_align_logspace(om, ctx, db.get(), logq, tr->tr, tr->status, &tr->nrounds, &tr->work_bytes);
    if (st != P7X_OK) return st;
    for (int t : logq) {
      if (tr->status[(size_t) t] != 0) { logredo.push_back(t); tr->nlogspace_flagged++; }     // a close call on the trace (or a failure: the twin names it)
      else tr->origin[(size_t) t] = P7X_TRACE_HAS_PP | P7X_TRACE_DEVICE | P7X_TRACE_LOGSPACE;
    }
    tr->nlogspace += (int64_t) logq.size() - tr->nlogspace_flagged;
  }
  if (!logredo.empty()) {
    const int st = host_traces(p, dsq, offsets, lengths, logredo, tr->tr, &bad, host_threads, Twin::Log);
    if (st != P7X_OK) return report_host_error(st, bad, lengths[bad]);
    for (int t : logredo) tr->origin[(size_t) t] = P7X_TRACE_HAS_PP | P7X_TRACE_LOGSPACE;
    tr->nlogspace += (int64_t) logredo.size();
  }
  *out = tr.release();
  return P7X_OK;
}

int64_t p7x_traces_count(const p7x_traces *tr) { return tr ? (int64_t) tr->tr.size() : -1; }
int64_t p7x_traces_nflagged(const p7x_traces *tr) { return tr ? tr->nflagged : -1; }

int p7x_traces_stats(const p7x_traces *tr, int64_t out4[4])
{
  if (!tr || !out4) { set_error("p7x_traces_stats: bad arguments"); return P7X_EINVAL; }
  int64_t ndev = 0;
  for (uint8_t o : tr->origin) ndev += (o & P7X_TRACE_DEVICE) ? 1 : 0;
  out4[0] = ndev; out4[1] = tr->nflagged; out4[2] = tr->nrounds; out4[3] = tr->work_bytes;
  return P7X_OK;
}

int p7x_traces_logspace_stats(const p7x_traces *tr, int64_t out2[2])
{
  if (!tr || !out2) { set_error("p7x_traces_logspace_stats: bad arguments"); return P7X_EINVAL; }
  out2[0] = tr->nlogspace; out2[1] = tr->nlogspace_flagged;
  return P7X_OK;
}

int p7x_traces_get(const p7x_traces *tr, int64_t idx, int32_t *N, int32_t *M, int32_t *L, float *sc2, int32_t *status, uint8_t *origin)
{
  if (!tr || idx < 0 || idx >= (int64_t) tr->tr.size()) { set_error("p7x_traces_get: index out of range"); return P7X_EINVAL; }
  const AlignTrace &a = tr->tr[(size_t) idx];
  if (N) *N = (int32_t) a.st.size();
  if (M) *M = tr->M;
  if (L) *L = tr->L[(size_t) idx];
  if (sc2) { sc2[0] = a.fwdsc; sc2[1] = a.oasc; }
  if (status) *status = tr->status[(size_t) idx];
  if (origin) *origin = tr->origin[(size_t) idx];
  return P7X_OK;
}

int p7x_traces_copy(const p7x_traces *tr, int64_t idx, int8_t *st, int32_t *k, int32_t *i, float *pp)
{
  if (!tr || idx < 0 || idx >= (int64_t) tr->tr.size()) { set_error("p7x_traces_copy: index out of range"); return P7X_EINVAL; }
  const AlignTrace &a = tr->tr[(size_t) idx];
  const size_t N = a.st.size();
  if (st) std::memcpy(st, a.st.data(), N);
  if (k) std::copy(a.k.begin(), a.k.end(), k);
  if (i) std::copy(a.i.begin(), a.i.end(), i);
  if (pp) std::copy(a.pp.begin(), a.pp.end(), pp);
  return P7X_OK;
}

void p7x_traces_destroy(p7x_traces *tr) { delete tr; }

// p7_tracealign_Seqs: map_new_msa, make_text_msa, annotate_rf, annotate_posteriors, annotate_model_cs, rejustify_insertions_text
int p7x_msa_from_traces(int32_t M, size_t n, const int8_t *st, const int32_t *tk, const int32_t *ti, const float *tpp, const int64_t *toff,
                        const uint8_t *origin, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, int32_t abc_type,
                        const char *cs, int flags, const p7x_oprofile *om, p7x_msa **out)
{
  if (!out || M < 1 || (n && (!st || !tk || !ti || !toff || !origin || !dsq || !offsets || !lengths))) {
    set_error("p7x_msa_from_traces: bad arguments"); return P7X_EINVAL;
  }
  *out = nullptr;
  const Alphabet &abc = Alphabet::get(abc_type);
  const bool trim = (flags & P7X_MSA_TRIM) != 0, allcons = (flags & P7X_MSA_ALL_CONSENSUS_COLS) != 0;
  for (size_t idx = 0; idx < n; ++idx)
    for (int64_t z = toff[idx]; z < toff[idx + 1]; ++z) {
      if (st[z] == 10) { set_error("p7x_msa_from_traces: J state unsupported"); return P7X_EINVAL; }
      if ((st[z] == 1 || st[z] == 2 || st[z] == 3) && (tk[z] < 1 || tk[z] > M)) { set_error("p7x_msa_from_traces: trace node out of range"); return P7X_EINVAL; }
      if ((st[z] == 1 || st[z] == 3 || st[z] == 5 || st[z] == 8) && (ti[z] < 0 || ti[z] > lengths[idx])) { set_error("p7x_msa_from_traces: trace residue out of range"); return P7X_EINVAL; }
    }
  // map_new_msa
  std::vector<int> inscount((size_t) M + 1, 0), insnum((size_t) M + 1), matuse((size_t) M + 1, allcons ? 1 : 0), matmap((size_t) M + 1, 0);
  matuse[0] = 0;
  for (size_t idx = 0; idx < n; ++idx) {
    std::fill(insnum.begin(), insnum.end(), 0);
    for (int64_t z = toff[idx] + 1; z < toff[idx + 1]; ++z)
      switch (st[z]) {
        case 3: insnum[(size_t) tk[z]]++; break;
        case 5: if (st[z - 1] == 5) insnum[0]++; break;
        case 8: if (st[z - 1] == 8) insnum[(size_t) M]++; break;
        case 1: matuse[(size_t) tk[z]] = 1; break;
        default: break;
      }
    for (int k = 0; k <= M; ++k) inscount[(size_t) k] = std::max(inscount[(size_t) k], insnum[(size_t) k]);
  }
  if (trim) inscount[0] = inscount[(size_t) M] = 0;
  int64_t alen = inscount[0];
  for (int k = 1; k <= M; ++k) {
    if (matuse[(size_t) k]) { matmap[(size_t) k] = (int) alen + 1; alen += 1 + inscount[(size_t) k]; }
    else                    { matmap[(size_t) k] = (int) alen;     alen += inscount[(size_t) k]; }
  }
  // Traces are user-constructible (plan7.Trace): every M / I step must name a residue, and every column the placement below
  // writes to must lie inside the alignment (an N / C emission that does not follow its own state is not counted by the
  // column map above), or the traces are refused
  for (size_t idx = 0; idx < n; ++idx) {
    int64_t apos = 0;
    for (int64_t z = toff[idx]; z < toff[idx + 1]; ++z) {
      bool ok = true;
      switch (st[z]) {
        case 1: ok = ti[z] >= 1; apos = matmap[(size_t) tk[z]]; break;
        case 2: apos = matmap[(size_t) tk[z]]; break;
        case 3: ok = ti[z] >= 1 && apos < alen; apos++; break;
        case 5: case 8: if (!trim && ti[z] > 0) { ok = apos < alen; apos++; } break;
        case 7: apos = matmap[(size_t) M]; break;
        default: break;
      }
      if (!ok) {
        set_error("p7x_msa_from_traces: trace " + std::to_string(idx) + " is not a valid alignment of its sequence (step " + std::to_string(z - toff[idx]) + ")");
        return P7X_EINVAL;
      }
    }
  }
  auto msa = std::make_unique<p7x_msa>();
  msa->alen = alen;
  msa->aseq.assign(n, std::string());
  msa->pp.assign(n, std::string());
  // make_text_msa
  for (size_t idx = 0; idx < n; ++idx) {
    std::string &a = msa->aseq[idx];
    a.assign((size_t) alen, '.');
    for (int k = 1; k <= M; ++k) if (matuse[(size_t) k]) a[(size_t) matmap[(size_t) k] - 1] = '-';
    const uint8_t *sq = dsq + offsets[idx] - 1;                  // 1-based residues
    int64_t apos = 0;
    for (int64_t z = toff[idx]; z < toff[idx + 1]; ++z)
      switch (st[z]) {
        case 1: a[(size_t) matmap[(size_t) tk[z]] - 1] = (char) std::toupper(abc.sym[sq[ti[z]]]); apos = matmap[(size_t) tk[z]]; break;
        case 2: if (matuse[(size_t) tk[z]]) a[(size_t) matmap[(size_t) tk[z]] - 1] = '-'; apos = matmap[(size_t) tk[z]]; break;
        case 3: a[(size_t) apos] = (char) std::tolower(abc.sym[sq[ti[z]]]); apos++; break;
        case 5: case 8: if (!trim && ti[z] > 0) { a[(size_t) apos] = (char) std::tolower(abc.sym[sq[ti[z]]]); apos++; } break;
        case 7: apos = matmap[(size_t) M]; break;
        default: break;
      }
  }
  // annotate_rf
  msa->rf.assign((size_t) alen, '.');
  for (int k = 1; k <= M; ++k) if (matuse[(size_t) k]) msa->rf[(size_t) matmap[(size_t) k] - 1] = 'x';
  // annotate_posteriors
  bool any_pp = false;
  for (size_t idx = 0; idx < n; ++idx) any_pp = any_pp || (origin[idx] & P7X_TRACE_HAS_PP);
  if (any_pp && tpp) {
    std::vector<double> totp((size_t) alen, 0.0);
    std::vector<int> nuse((size_t) alen, 0);
    for (size_t idx = 0; idx < n; ++idx) {
      if (!(origin[idx] & P7X_TRACE_HAS_PP)) continue;
      std::string &pl = msa->pp[idx];
      pl.assign((size_t) alen, '.');
      int64_t apos = 0;
      for (int64_t z = toff[idx]; z < toff[idx + 1]; ++z)
        switch (st[z]) {
          case 1: {
            const size_t col = (size_t) matmap[(size_t) tk[z]] - 1;
            pl[col] = encode_pp(tpp[z]); totp[col] += tpp[z]; nuse[col]++;
            apos = matmap[(size_t) tk[z]];
            break;
          }
          case 2: apos = matmap[(size_t) tk[z]]; break;
          case 3: pl[(size_t) apos] = encode_pp(tpp[z]); apos++; break;
          case 5: case 8: if (!trim && ti[z] > 0) { pl[(size_t) apos] = encode_pp(tpp[z]); apos++; } break;
          case 7: apos = matmap[(size_t) M]; break;
          default: break;
        }
    }
    // columns whose mean lies within the guard of a digit boundary: averaged again over the host twin's posteriors of the
    // device traces that contribute to them (the twin's trace is the device's: a trace that differed was flagged)
    if (om) {
      std::vector<char> near((size_t) alen, 0);
      bool any_near = false;
      for (int64_t c = 0; c < alen; ++c) if (nuse[(size_t) c] && pp_near_boundary(totp[(size_t) c] / (double) nuse[(size_t) c], M)) { near[(size_t) c] = 1; any_near = true; }
      if (any_near) {
        std::vector<int> which;
        for (size_t idx = 0; idx < n; ++idx) {
          if ((origin[idx] & (P7X_TRACE_HAS_PP | P7X_TRACE_DEVICE)) != (P7X_TRACE_HAS_PP | P7X_TRACE_DEVICE)) continue;
          bool hit = false;
          for (int64_t z = toff[idx]; z < toff[idx + 1] && !hit; ++z) if (st[z] == 1 && near[(size_t) matmap[(size_t) tk[z]] - 1]) hit = true;
          if (hit) which.push_back((int) idx);
        }
        std::vector<AlignTrace> host(n);
        int64_t bad = -1;
        // rows of the log-space path are averaged again from the log twin, the others from the scaled one
        std::vector<int> scaled, logrows;
        for (int idx : which) ((origin[idx] & P7X_TRACE_LOGSPACE) ? logrows : scaled).push_back(idx);
        int hst = host_traces(om->p, dsq, offsets, lengths, scaled, host, &bad);
        if (hst == P7X_OK) hst = host_traces(om->p, dsq, offsets, lengths, logrows, host, &bad, 0, Twin::Log);
        if (hst != P7X_OK) return report_host_error(hst, bad, lengths[bad]);
        for (int idx : which) {
          const AlignTrace &h = host[(size_t) idx];
          const int64_t N = toff[idx + 1] - toff[idx];
          if ((int64_t) h.st.size() != N) continue;
          bool same = true;
          for (int64_t z = 0; z < N && same; ++z) same = h.st[(size_t) z] == st[toff[idx] + z] && h.k[(size_t) z] == tk[toff[idx] + z] && h.i[(size_t) z] == ti[toff[idx] + z];
          if (!same) continue;
          for (int64_t z = 0; z < N; ++z) {
            if (st[toff[idx] + z] != 1) continue;
            const size_t col = (size_t) matmap[(size_t) tk[toff[idx] + z]] - 1;
            if (near[col]) totp[col] += (double) h.pp[(size_t) z] - (double) tpp[toff[idx] + z];
          }
        }
      }
    }
    msa->pp_cons.assign((size_t) alen, '.');
    for (int64_t c = 0; c < alen; ++c) if (nuse[(size_t) c]) msa->pp_cons[(size_t) c] = encode_pp((float) (totp[(size_t) c] / (double) nuse[(size_t) c]));
  }
  // annotate_model_cs
  if (cs) {
    msa->ss_cons.assign((size_t) alen, '.');
    for (int k = 1; k <= M; ++k) if (matuse[(size_t) k]) msa->ss_cons[(size_t) matmap[(size_t) k] - 1] = cs[k];
  }
  // rejustify_insertions_text: inserts split in half around their node's columns, the N-terminal ones right-justified
  for (size_t idx = 0; idx < n; ++idx) {
    std::string &a = msa->aseq[idx];
    std::string *pl = msa->pp[idx].empty() ? nullptr : &msa->pp[idx];
    for (int k = 0; k < M; ++k) {
      if (inscount[(size_t) k] <= 1) continue;
      const int64_t lo = k == 0 ? 0 : matmap[(size_t) k], hi = matmap[(size_t) k + 1] - matuse[(size_t) k + 1];
      int64_t nins = 0;
      for (int64_t apos = lo; apos < hi; ++apos) if (std::isalnum((unsigned char) a[(size_t) apos])) nins++;
      nins = (k == 0) ? 0 : nins / 2;
      int64_t opos = hi - 1, npos = hi - 1;
      while (opos >= lo + nins) {
        if (std::isalnum((unsigned char) a[(size_t) opos])) {
          a[(size_t) npos] = a[(size_t) opos];
          if (pl) (*pl)[(size_t) npos] = (*pl)[(size_t) opos];
          npos--;
        }
        opos--;
      }
      while (npos >= lo + nins) {
        a[(size_t) npos] = '.';
        if (pl) (*pl)[(size_t) npos] = '.';
        npos--;
      }
    }
  }
  // P7X_MSA_DIGITIZE: the rows once more as digital codes (a residue in either case is its code, both gap characters the
  // alphabet's gap code), so that a caller that counts over the alignment need not encode the text again
  if (flags & P7X_MSA_DIGITIZE) {
    uint8_t lut[256];
    std::memset(lut, 255, sizeof lut);
    for (int x = 0; x < abc.Kp; ++x) lut[(unsigned char) std::toupper(abc.sym[x])] = lut[(unsigned char) std::tolower(abc.sym[x])] = (uint8_t) x;
    lut[(unsigned char) '.'] = lut[(unsigned char) '-'] = (uint8_t) abc.K;
    msa->codes.resize(n * (size_t) alen);
    for (size_t idx = 0; idx < n; ++idx)
      for (int64_t c = 0; c < alen; ++c) msa->codes[idx * (size_t) alen + (size_t) c] = lut[(unsigned char) msa->aseq[idx][(size_t) c]];
  }
  *out = msa.release();
  return P7X_OK;
}

int64_t p7x_msa_codes(const p7x_msa *msa, uint8_t *out, size_t nbytes)
{
  if (!msa || msa->codes.empty() || debug_opt(OPT_MSA_CODES) == 0) return -1;
  if (out && nbytes >= msa->codes.size()) std::memcpy(out, msa->codes.data(), msa->codes.size());
  return (int64_t) msa->codes.size();
}

int64_t p7x_msa_alen(const p7x_msa *msa) { return msa ? msa->alen : -1; }

int64_t p7x_msa_get(const p7x_msa *msa, int64_t idx, int which, char *buf, size_t cap)
{
  if (!msa) return -1;
  const std::string *s = nullptr;
  switch (which) {
    case 0: case 1:
      if (idx < 0 || idx >= (int64_t) msa->aseq.size()) return -1;
      s = which == 0 ? &msa->aseq[(size_t) idx] : &msa->pp[(size_t) idx];
      break;
    case 2: s = &msa->pp_cons; break;
    case 3: s = &msa->rf; break;
    case 4: s = &msa->ss_cons; break;
    case 5: case 6: case 7: {
      static const std::string none;
      const std::vector<std::string> &v = which == 5 ? msa->name : (which == 6 ? msa->acc : msa->desc);
      if (idx < 0 || idx >= (int64_t) msa->aseq.size()) return -1;
      s = (size_t) idx < v.size() ? &v[(size_t) idx] : &none;
      break;
    }
    case 8: s = &msa->msa_name; break;
    default: return -1;
  }
  if (buf && cap > 0) { const size_t m = std::min(cap - 1, s->size()); std::memcpy(buf, s->data(), m); buf[m] = '\0'; }
  return (int64_t) s->size();
}

void p7x_msa_destroy(p7x_msa *msa) { delete msa; }

// p7_alidisplay_Backconvert
int p7x_alidisplay_backconvert(int32_t abc_type, const char *model, const char *aseq, const char *ppline, int32_t hmmfrom, int32_t hmmto,
                               int64_t sqfrom, int64_t sqto, int64_t L, int whole, int32_t *N, int32_t *subL, int8_t *st, int32_t *k,
                               int32_t *i, float *pp, uint8_t *dsq, size_t cap)
{
  if (!model || !aseq || !N || !subL || (abc_type != P7X_AMINO && abc_type != P7X_DNA && abc_type != P7X_RNA)) {
    set_error("p7x_alidisplay_backconvert: bad arguments"); return P7X_EINVAL;
  }
  std::vector<int8_t> vst; std::vector<int32_t> vk, vi; std::vector<float> vpp; std::vector<uint8_t> vdsq;
  const int rc = backconvert(abc_type, model, aseq, ppline, hmmfrom, hmmto, sqfrom, sqto, L, whole != 0, vst, vk, vi, vpp, vdsq);
  if (rc != P7X_OK) return rc;
  *N = (int32_t) vst.size(); *subL = (int32_t) vdsq.size();
  if (cap >= vst.size()) {
    if (st) std::memcpy(st, vst.data(), vst.size());
    if (k) std::copy(vk.begin(), vk.end(), k);
    if (i) std::copy(vi.begin(), vi.end(), i);
    if (pp) std::copy(vpp.begin(), vpp.end(), pp);
    if (dsq) std::copy(vdsq.begin(), vdsq.end(), dsq);
  }
  return P7X_OK;
}

// p7_tophits_Alignment
int p7x_tophits_to_msa(const p7x_tophits *th, int32_t abc_type, int32_t M, size_t nextra, const int8_t *xst, const int32_t *xk,
                       const int32_t *xi, const float *xpp, const int64_t *xtoff, const uint8_t *xorigin, const uint8_t *xdsq,
                       const int64_t *xoffsets, const int32_t *xlengths, const char *const *xnames, const char *const *xaccs,
                       const char *const *xdescs, int flags, p7x_msa **out)
{
  if (!th || !out || (nextra && (!xst || !xk || !xi || !xtoff || !xorigin || !xdsq || !xoffsets || !xlengths)) ||
      (abc_type != P7X_AMINO && abc_type != P7X_DNA && abc_type != P7X_RNA)) {
    set_error("p7x_tophits_to_msa: bad arguments"); return P7X_EINVAL;
  }
  *out = nullptr;
  if (th->cfg.mode == P7X_SCAN_MODELS && th->scan_collected) { set_error("p7x_tophits_to_msa: the hits of a scan belong to different models"); return P7X_EINVAL; }
  if (th->abc_type != 0 && th->abc_type != abc_type) { set_error("p7x_tophits_to_msa: alphabet mismatch with the hits' alphabet"); return P7X_EINVAL; }
  if (M <= 0) M = th->M;
  if (M < 1 || (th->M > 0 && M != th->M && !th->hits.empty())) { set_error("p7x_tophits_to_msa: the model length of the traces is not the hits'"); return P7X_EINVAL; }
  // the rows: the caller's first, then the included domains of the included hits in the list's order
  std::vector<int8_t> st; std::vector<int32_t> tk, ti; std::vector<float> tpp;
  std::vector<int64_t> toff{ 0 }, offsets;
  std::vector<int32_t> lengths;
  std::vector<uint8_t> origin, dsq{ 255 };
  auto msa_rows = std::make_unique<p7x_msa>();          // carries the row texts until the alignment exists
  for (size_t y = 0; y < nextra; ++y) {
    if (xtoff[y + 1] < xtoff[y] || xlengths[y] < 0) { set_error("p7x_tophits_to_msa: bad arguments"); return P7X_EINVAL; }
    st.insert(st.end(), xst + xtoff[y], xst + xtoff[y + 1]);
    tk.insert(tk.end(), xk + xtoff[y], xk + xtoff[y + 1]);
    ti.insert(ti.end(), xi + xtoff[y], xi + xtoff[y + 1]);
    if (xpp) tpp.insert(tpp.end(), xpp + xtoff[y], xpp + xtoff[y + 1]); else tpp.insert(tpp.end(), (size_t) (xtoff[y + 1] - xtoff[y]), 0.0f);
    toff.push_back((int64_t) st.size());
    origin.push_back((uint8_t) (xpp ? (xorigin[y] & P7X_TRACE_HAS_PP) : 0));     // no host-twin averaging: there is no profile here
    offsets.push_back((int64_t) dsq.size()); lengths.push_back(xlengths[y]);
    dsq.insert(dsq.end(), xdsq + xoffsets[y], xdsq + xoffsets[y] + xlengths[y]);
    dsq.push_back(255);
    msa_rows->name.emplace_back(xnames && xnames[y] ? xnames[y] : "");
    msa_rows->acc.emplace_back(xaccs && xaccs[y] ? xaccs[y] : "");
    msa_rows->desc.emplace_back(xdescs && xdescs[y] ? xdescs[y] : "");
  }
  std::vector<int8_t> vst; std::vector<int32_t> vk, vi; std::vector<float> vpp; std::vector<uint8_t> vdsq;
  for (size_t r = 0; r < th->hits.size(); ++r) {
    const Hit &h = th->hits[th->order.size() == th->hits.size() ? (size_t) th->order[r] : r];
    if (!(h.flags & P7X_IS_INCLUDED)) continue;
    for (const Domain &d : h.dcl) {
      if (!d.is_included) continue;
      const int rc = backconvert(abc_type, d.model.c_str(), d.aseq.c_str(), d.ppline.empty() ? nullptr : d.ppline.c_str(), d.hmmfrom, d.hmmto,
                                 d.sqfrom, d.sqto, d.L, false, vst, vk, vi, vpp, vdsq);
      if (rc != P7X_OK) { set_error(std::string(p7x_last_error()) + " (" + h.name + ")"); return rc; }
      st.insert(st.end(), vst.begin(), vst.end()); tk.insert(tk.end(), vk.begin(), vk.end());
      ti.insert(ti.end(), vi.begin(), vi.end()); tpp.insert(tpp.end(), vpp.begin(), vpp.end());
      toff.push_back((int64_t) st.size());
      origin.push_back((uint8_t) (d.ppline.empty() ? 0 : P7X_TRACE_HAS_PP));
      offsets.push_back((int64_t) dsq.size()); lengths.push_back((int32_t) vdsq.size());
      dsq.insert(dsq.end(), vdsq.begin(), vdsq.end());
      dsq.push_back(255);
      msa_rows->name.push_back(h.name + "/" + std::to_string(d.sqfrom) + "-" + std::to_string(d.sqto));
      msa_rows->acc.push_back(h.has_acc ? h.acc : std::string());
      msa_rows->desc.push_back("[subseq from] " + (h.has_desc && !h.desc.empty() ? h.desc : h.name));
    }
  }
  const size_t n = lengths.size();
  if (n == 0) { set_error("No included domains found"); return P7X_EINVAL; }
  p7x_msa *msa = nullptr;
  const int rc = p7x_msa_from_traces(M, n, st.data(), tk.data(), ti.data(), tpp.data(), toff.data(), origin.data(), dsq.data(), offsets.data(),
                                     lengths.data(), abc_type, nullptr, flags, nullptr, &msa);
  if (rc != P7X_OK) return rc;
  msa->name = std::move(msa_rows->name); msa->acc = std::move(msa_rows->acc); msa->desc = std::move(msa_rows->desc);
  msa->msa_name = th->qname;
  *out = msa;
  return P7X_OK;
}

// esl_msafile_stockholm.c stockholm_write, 200 columns per block
int64_t p7x_msa_write_stockholm(size_t n, int64_t alen, const char *const *names, const char *const *accs, const char *const *descs,
                                const char *const *aseqs, const char *const *pps, const char *ss_cons, const char *pp_cons, const char *rf,
                                char *buf, size_t cap)
{
  if ((n && (!names || !aseqs)) || alen < 0) { set_error("p7x_msa_write_stockholm: bad arguments"); return -1; }
  constexpr int64_t cpl = 200;
  std::string o;
  auto pad = [](const char *s, int w) { std::string r(s ? s : ""); if ((int) r.size() < w) r.append((size_t) (w - (int) r.size()), ' '); return r; };
  // every row and every annotation line that is given must have exactly alen characters (the blocks copy alen out of each)
  auto bad_len = [&](const char *s, const char *what) {
    if (!s || !s[0] || std::strlen(s) == (size_t) alen) return false;
    set_error(std::string("p7x_msa_write_stockholm: ") + what + " does not have " + std::to_string(alen) + " characters");
    return true;
  };
  if (bad_len(ss_cons, "SS_cons") || bad_len(pp_cons, "PP_cons") || bad_len(rf, "RF")) return -1;
  for (size_t i = 0; i < n; ++i) {
    if (!aseqs[i] || std::strlen(aseqs[i]) != (size_t) alen) { set_error("p7x_msa_write_stockholm: row " + std::to_string(i) + " does not have " + std::to_string(alen) + " characters"); return -1; }
    if (pps && bad_len(pps[i], "a PP line")) return -1;
  }
  int maxname = 0, maxgc = 0, maxgr = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!names[i]) { set_error("p7x_msa_write_stockholm: a sequence has no name"); return -1; }
    maxname = std::max(maxname, (int) std::strlen(names[i]));
    if (pps && pps[i] && pps[i][0]) maxgr = 2;
  }
  if (ss_cons && ss_cons[0]) maxgc = 7;
  if (pp_cons && pp_cons[0]) maxgc = 7;
  if (rf && rf[0]) maxgc = std::max(maxgc, 2);
  int margin = maxname + 1;
  if (maxgc > 0 && maxgc + 6 > margin) margin = maxgc + 6;
  if (maxgr > 0 && maxname + maxgr + 7 > margin) margin = maxname + maxgr + 7;
  o += "# STOCKHOLM 1.0\n\n";
  bool gs = false;
  for (size_t i = 0; i < n; ++i) {
    if (accs && accs[i] && accs[i][0]) { o += "#=GS " + pad(names[i], maxname) + " AC " + accs[i] + "\n"; gs = true; }
    if (descs && descs[i] && descs[i][0]) { o += "#=GS " + pad(names[i], maxname) + " DE " + descs[i] + "\n"; gs = true; }
  }
  if (gs) o += "\n";
  for (int64_t pos = 0; pos < alen; pos += cpl) {
    if (pos > 0) o += "\n";
    const size_t w = (size_t) std::min(cpl, alen - pos);
    auto seg = [&](const char *s) { return std::string(s + pos, w); };
    for (size_t i = 0; i < n; ++i) {
      o += pad(names[i], margin - 1) + " " + seg(aseqs[i]) + "\n";
      if (pps && pps[i] && pps[i][0]) o += "#=GR " + pad(names[i], maxname) + " " + pad("PP", margin - maxname - 7) + " " + seg(pps[i]) + "\n";
    }
    if (ss_cons && ss_cons[0]) o += "#=GC " + pad("SS_cons", margin - 6) + " " + seg(ss_cons) + "\n";
    if (pp_cons && pp_cons[0]) o += "#=GC " + pad("PP_cons", margin - 6) + " " + seg(pp_cons) + "\n";
    if (rf && rf[0]) o += "#=GC " + pad("RF", margin - 6) + " " + seg(rf) + "\n";
  }
  o += "//\n";
  if (buf && cap >= o.size()) std::memcpy(buf, o.data(), o.size());
  return (int64_t) o.size();
}

} // extern "C"
