// p7x_msabuild.cpp -- Builder.build_msa: a protein alignment as a query (hmmbuild).
//
// Host code.  Restated from the published procedure of HMMER 3's builder: fragments marked, position-based relative
// weights (Henikoff & Henikoff 1994), consensus columns by weighted occupancy, weighted counts of the rows as paths
// through the consensus columns, Dirichlet priors (Sjolander et al. 1996: the nine-component mixture for amino match
// emissions), entropy weighting to a target mean relative entropy, the boundary conventions of a Plan 7 model.
// The passes that grow with the depth of the alignment run on the device (p7x_msabuild.hip); their host twins are
// here (debug option "host_build" = 1), over the same integers: see p7x_msabuild.hpp.
#include "p7x_msabuild.hpp"
#include "p7x_host.hpp"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>

namespace p7x {

// ---------------------------------------------------------------- priors (data)
static const double kTransPrior[7] = { 0.7939, 0.0278, 0.0135, 0.1551, 0.1331, 0.9002, 0.5630 };
static const int kMixN = 9;
static const double kMixQ[kMixN] = { 0.178091, 0.056591, 0.0960191, 0.0781233, 0.0834977, 0.0904123, 0.114468, 0.0682132, 0.234585 };
static const double kMixAlpha[kMixN][20] = {
  { 0.270671, 0.039848, 0.017576, 0.016415, 0.014268, 0.131916, 0.012391, 0.022599, 0.020358, 0.030727, 0.015315, 0.048298, 0.053803, 0.020662, 0.023612, 0.216147, 0.147226, 0.065438, 0.003758, 0.009621 },
  { 0.021465, 0.010300, 0.011741, 0.010883, 0.385651, 0.016416, 0.076196, 0.035329, 0.013921, 0.093517, 0.022034, 0.028593, 0.013086, 0.023011, 0.018866, 0.029156, 0.018153, 0.036100, 0.071770, 0.419641 },
  { 0.561459, 0.045448, 0.438366, 0.764167, 0.087364, 0.259114, 0.214940, 0.145928, 0.762204, 0.247320, 0.118662, 0.441564, 0.174822, 0.530840, 0.465529, 0.583402, 0.445586, 0.227050, 0.029510, 0.121090 },
  { 0.070143, 0.011140, 0.019479, 0.094657, 0.013162, 0.048038, 0.077000, 0.032939, 0.576639, 0.072293, 0.028240, 0.080372, 0.037661, 0.185037, 0.506783, 0.073732, 0.071587, 0.042532, 0.011254, 0.028723 },
  { 0.041103, 0.014794, 0.005610, 0.010216, 0.153602, 0.007797, 0.007175, 0.299635, 0.010849, 0.999446, 0.210189, 0.006127, 0.013021, 0.019798, 0.014509, 0.012049, 0.035799, 0.180085, 0.012744, 0.026466 },
  { 0.115607, 0.037381, 0.012414, 0.018179, 0.051778, 0.017255, 0.004911, 0.796882, 0.017074, 0.285858, 0.075811, 0.014548, 0.015092, 0.011382, 0.012696, 0.027535, 0.088333, 0.944340, 0.004373, 0.016741 },
  { 0.093461, 0.004737, 0.387252, 0.347841, 0.010822, 0.105877, 0.049776, 0.014963, 0.094276, 0.027761, 0.010040, 0.187869, 0.050018, 0.110039, 0.038668, 0.119471, 0.065802, 0.025430, 0.003215, 0.018742 },
  { 0.452171, 0.114613, 0.062460, 0.115702, 0.284246, 0.140204, 0.100358, 0.550230, 0.143995, 0.700649, 0.276580, 0.118569, 0.097470, 0.126673, 0.143634, 0.278983, 0.358482, 0.661750, 0.061533, 0.199373 },
  { 0.005193, 0.004039, 0.006722, 0.006121, 0.003468, 0.016931, 0.003647, 0.002184, 0.005019, 0.005990, 0.001473, 0.004158, 0.009055, 0.003630, 0.006583, 0.003172, 0.003690, 0.002967, 0.002772, 0.002686 },
};

// The insert emissions of every model hmmbuild writes: the mean of its insert prior, which sees no counts (they are not
// the null model's frequencies), before it adds the inserted residues, which this builder leaves out.  Read off
// the insert rows of the LuxC and RREFam fixtures, -ln p as printed (five decimals).
static const double kInsertNegLog[20] = { 2.68618, 4.42225, 2.77519, 2.73123, 3.46354, 2.40513, 3.72494, 3.29354, 2.67741, 2.69355,
                                          4.24690, 2.90347, 2.73739, 3.18146, 2.89801, 2.37887, 2.77519, 2.98518, 4.58477, 3.61503 };

// lgamma without the global sign of the C function (every argument here is positive)
static double lng(double x) { int sign = 0; return lgamma_r(x, &sign); }

struct MixPrior {
  double sum[kMixN], lnorm[kMixN];          // |alpha_q|; ln m_q + lnG|alpha_q| - sum_a lnG(alpha_qa)
  MixPrior()
  {
    for (int q = 0; q < kMixN; ++q) {
      double s = 0.0, l = 0.0;
      for (int a = 0; a < 20; ++a) { s += kMixAlpha[q][a]; l += lng(kMixAlpha[q][a]); }
      sum[q] = s; lnorm[q] = std::log(kMixQ[q]) + lng(s) - l;
    }
  }
};

// the posterior mean emission distribution of one vector of counts
static void emission_posterior(const double *c, int prior, double *p)
{
  static const MixPrior mp;
  double tot = 0.0;
  for (int a = 0; a < 20; ++a) tot += c[a];
  if (prior == 1) { for (int a = 0; a < 20; ++a) p[a] = (c[a] + 1.0) / (tot + 20.0); return; }
  double lp[kMixN], best = -INFINITY;
  for (int q = 0; q < kMixN; ++q) {
    double l = mp.lnorm[q] - lng(tot + mp.sum[q]);
    for (int a = 0; a < 20; ++a) l += lng(c[a] + kMixAlpha[q][a]);
    lp[q] = l; best = std::max(best, l);
  }
  double z = 0.0;
  for (int q = 0; q < kMixN; ++q) { lp[q] = std::exp(lp[q] - best); z += lp[q]; }
  for (int a = 0; a < 20; ++a) p[a] = 0.0;
  for (int q = 0; q < kMixN; ++q) {
    const double pq = lp[q] / z, den = tot + mp.sum[q];
    for (int a = 0; a < 20; ++a) p[a] += pq * (c[a] + kMixAlpha[q][a]) / den;
  }
}

// mean match relative entropy (bits) of the model parameterised from the counts times <scale>
static double scaled_relent(const std::vector<double> &em, int M, double scale, const double *bg, int prior)
{
  double tot = 0.0;
  for (int k = 1; k <= M; ++k) {
    double c[20], p[20], h = 0.0;
    for (int a = 0; a < 20; ++a) c[a] = em[(size_t) k * 20 + a] * scale;
    emission_posterior(c, prior, p);
    for (int a = 0; a < 20; ++a) if (p[a] > 0.0) h += p[a] * std::log2(p[a] / bg[a]);
    tot += h;
  }
  return tot / (double) M;
}

// ---------------------------------------------------------------- the host twins of the kernels
// Each walks a range of rows into sums of its own; the ranges run on up to 16 threads and their sums are added: integers,
// so the result is the same for any number of threads (and the kernels').
template <class F> static void over_row_ranges(int64_t N, F f)
{
  const int64_t hw = (int64_t) std::thread::hardware_concurrency();
  const int T = (int) std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, hw > 0 ? hw : 1), N / 512));
  if (T == 1) { f(0, (int64_t) 0, N); return; }
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) th.emplace_back(f, t, N * t / T, N * (t + 1) / T);
  for (auto &x : th) x.join();
}
template <class V> static void add_into(V &dst, const V &src) { for (size_t i = 0; i < dst.size(); ++i) dst[i] += src[i]; }

static void host_count(p7x_msacounts &c, bool weighted)
{
  std::vector<std::vector<uint64_t>> part(16);
  over_row_ranges(c.N, [&](int t, int64_t r0, int64_t r1) {
    std::vector<uint64_t> &cnt = part[t];
    cnt.assign((size_t) c.Lp * kMsaSlots, 0);
    for (int64_t i = r0; i < r1; ++i) {
      const uint8_t *row = c.ax.data() + (size_t) i * c.Lp;
      const uint64_t w = weighted ? c.wq[i] : 1;
      for (int col = 0; col < c.L; ++col) if (row[col] < kMsaCodes) cnt[(size_t) col * kMsaSlots + row[col]] += w;
    }
  });
  for (const auto &cnt : part) {
    if (cnt.empty()) continue;
    if (weighted) add_into(c.wcnt, cnt);
    else for (size_t i = 0; i < cnt.size(); ++i) c.colcnt[i] += (uint32_t) cnt[i];
  }
}
static void host_colcount(p7x_msacounts &c) { host_count(c, false); }
static void host_wcount(p7x_msacounts &c) { host_count(c, true); }
static void host_pbweight(p7x_msacounts &c)
{
  over_row_ranges(c.N, [&](int, int64_t r0, int64_t r1) {
    for (int64_t i = r0; i < r1; ++i) {
      const uint8_t *row = c.ax.data() + (size_t) i * c.Lp;
      uint64_t s = 0; int32_t len = 0;
      for (int col = 0; col < c.L; ++col) {
        if (!c.wmask[col]) continue;
        const unsigned a = row[col];
        if (msa_is_canonical(a)) { s += c.termq[(size_t) col * 20 + a]; ++len; }
        else if (msa_is_residue(a)) ++len;
      }
      c.rowsum[i] = s; c.rowlen[i] = len;
    }
  });
}
static void host_transitions(p7x_msacounts &c)
{
  const int M = c.M;
  std::vector<std::vector<uint64_t>> ptr(16), ptk(16);
  over_row_ranges(c.N, [&](int th, int64_t r0, int64_t r1) {
    std::vector<uint64_t> &trq = ptr[th], &taken = ptk[th];
    trq.assign(c.trq.size(), 0); taken.assign(c.taken.size(), 0);
    for (int64_t i = r0; i < r1; ++i) {
      const uint8_t *row = c.ax.data() + (size_t) i * c.Lp;
      const uint64_t w = c.wq[i];
      const bool frag = c.frag[i] != 0;
      for (int k = 0; k <= M; ++k) {
        const MsaStep s = msa_step(row, c.map.data(), M, k, frag);
        uint64_t *t = trq.data() + (size_t) k * 8;
        if (s.slot >= 0) t[s.slot] += w;
        if (s.nins > 0) { t[1] += w; t[4] += msa_ii_low(w, s.nins); t[7] += msa_ii_high(w, s.nins); t[3] += w; }
        if (s.taken >= 0) taken[(size_t) k * kMsaSlots + s.taken] += w;
      }
    }
  });
  for (int th = 0; th < 16; ++th) if (!ptr[th].empty()) { add_into(c.trq, ptr[th]); add_into(c.taken, ptk[th]); }
}

// ---------------------------------------------------------------- what the host decides between the passes
// the padded copy of the alignment with the fragments marked; false when a cell holds no code of the alphabet
static bool mark_fragments(p7x_msacounts &c, const uint8_t *ax, double fragthresh)
{
  c.ax.resize((size_t) c.N * c.Lp);
  c.frag.assign((size_t) c.N, 0);
  std::atomic<int64_t> nfrag{ 0 };
  std::atomic<bool> bad{ false };
  over_row_ranges(c.N, [&](int, int64_t r0, int64_t r1) {
    for (int64_t i = r0; i < r1; ++i) {
      const uint8_t *src = ax + (size_t) i * c.L;
      uint8_t *dst = c.ax.data() + (size_t) i * c.Lp;
      std::memcpy(dst, src, (size_t) c.L);
      std::memset(dst + c.L, kMsaPad, (size_t) (c.Lp - c.L));
      int first = -1, last = -1;
      unsigned top = 0;
      for (int col = 0; col < c.L; ++col) {
        top |= src[col] >= kMsaCodes;
        if (msa_is_residue(src[col])) { if (first < 0) first = col; last = col; }
      }
      if (top) bad.store(true);
      if (first < 0) continue;
      if ((double) (last - first + 1) / (double) c.L < fragthresh) {
        c.frag[i] = 1; ++nfrag;
        std::memset(dst, kMsaMissing, (size_t) first);
        std::memset(dst + last + 1, kMsaMissing, (size_t) (c.L - 1 - last));
      }
    }
  });
  c.nfrag = nfrag.load();
  return !bad.load();
}

static void column_sums(const uint32_t *cnt, uint64_t *nres, uint64_t *ngap)
{
  uint64_t r = 0;
  for (int a = 0; a <= 26; ++a) if (a != kMsaK) r += cnt[a];
  *nres = r; *ngap = cnt[kMsaK];
}

// the weighting columns and the terms 1 / (r_c n_c(a)) of their residues, in fixed point
static void weighting_columns(p7x_msacounts &c, const uint8_t *rf_mask, double symfrac)
{
  c.wmask.assign((size_t) c.Lp, 0);
  c.termq.assign((size_t) c.Lp * 20, 0);
  c.nwcols = 0;
  for (int col = 0; col < c.L; ++col) {
    bool use;
    if (rf_mask) use = rf_mask[col] != 0;
    else {
      uint64_t r, g; column_sums(c.colcnt.data() + (size_t) col * kMsaSlots, &r, &g);
      use = r + g > 0 && (double) r >= symfrac * (double) (r + g);
    }
    if (use) { c.wmask[col] = 1; ++c.nwcols; }
  }
  if (c.nwcols == 0) { for (int col = 0; col < c.L; ++col) c.wmask[col] = 1; c.nwcols = c.L; }
  for (int col = 0; col < c.L; ++col) {
    if (!c.wmask[col]) continue;
    const uint32_t *cnt = c.colcnt.data() + (size_t) col * kMsaSlots;
    uint64_t r = 0;
    for (int a = 0; a < 20; ++a) r += cnt[a] > 0;
    for (int a = 0; a < 20; ++a)
      if (cnt[a]) { const uint64_t d = r * (uint64_t) cnt[a]; c.termq[(size_t) col * 20 + a] = (((uint64_t) 1 << kMsaShift) + d / 2) / d; }
  }
}

// w_i = rowsum_i / rowlen_i, scaled to sum N, in fixed point
static void finish_weights(p7x_msacounts &c)
{
  std::vector<double> w((size_t) c.N, 0.0);
  double tot = 0.0;
  for (int64_t i = 0; i < c.N; ++i) {
    if (c.rowlen[i] > 0) w[i] = std::ldexp((double) c.rowsum[i], -kMsaShift) / (double) c.rowlen[i];
    tot += w[i];
  }
  for (int64_t i = 0; i < c.N; ++i) {
    const double v = tot > 0.0 ? w[i] * (double) c.N / tot : 1.0;
    c.wq[i] = (uint64_t) std::llround(std::ldexp(v, kMsaShift));
  }
}

static int consensus_columns(p7x_msacounts &c, const uint8_t *rf_mask, double symfrac)
{
  c.map.assign(1, -1);
  for (int col = 0; col < c.L; ++col) {
    bool use;
    if (rf_mask) use = rf_mask[col] != 0;
    else {
      const uint64_t *cnt = c.wcnt.data() + (size_t) col * kMsaSlots;
      uint64_t r = 0;
      for (int a = 0; a <= 26; ++a) if (a != kMsaK) r += cnt[a];
      const uint64_t g = cnt[kMsaK];
      use = r > 0 && (double) r >= symfrac * ((double) r + (double) g);
    }
    if (use) c.map.push_back(col);
  }
  c.M = (int) c.map.size() - 1;
  c.map.push_back(c.L);
  if (c.M < 1) { set_error("the alignment has no consensus column"); return P7X_EINVAL; }
  if (c.M > p7x_max_model_length()) {
    set_error("the alignment has " + std::to_string(c.M) + " consensus columns, more than the longest model the device takes (" +
              std::to_string(p7x_max_model_length()) + ")");
    return P7X_ERANGE;
  }
  return P7X_OK;
}

static int msa_counts(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, const uint8_t *rf_mask, int weighting, double symfrac,
                      double fragthresh, int device, p7x_msacounts &c)
{
  if (abc_type != P7X_AMINO) { set_error("alignments are built into models for the amino alphabet only"); return P7X_EINVAL; }
  if (!ax || N < 1 || L < 1) { set_error("the alignment is empty"); return P7X_EINVAL; }
  if (N > kMsaMaxRows) { set_error("the alignment has " + std::to_string(N) + " rows, more than 2^20"); return P7X_ERANGE; }
  if (L > kMsaMaxCols) { set_error("the alignment has " + std::to_string(L) + " columns, more than 65,535"); return P7X_ERANGE; }
  if (!(symfrac >= 0.0 && symfrac <= 1.0) || !(fragthresh >= 0.0 && fragthresh <= 1.0)) { set_error("symfrac and fragthresh lie in [0, 1]"); return P7X_EINVAL; }
  const bool host = debug_opt(OPT_HOST_BUILD) > 0;
  c.N = N; c.L = L; c.Lp = (L + 3) / 4 * 4; c.on_device = host ? 0 : 1;
  const int rows = debug_opt(OPT_BUILD_ROWS);
  c.rows_per_block = rows > 0 ? rows : 0;
  MsaDevice *dev = nullptr;
  struct Closer { MsaDevice *&d; ~Closer() { if (d) msa_device_close(d); } } closer{ dev };
  if (!mark_fragments(c, ax, fragthresh)) { set_error("the alignment holds a code outside the alphabet"); return P7X_EINVAL; }
  int st = P7X_OK;
  if (!host && (st = msa_device_open(device, c, &dev)) != P7X_OK) return st;

  // a pass of the host twin, timed as the device's are (wall clock in place of device events)
  auto twin = [&](void (*pass)(p7x_msacounts &), int which) {
    const auto t0 = std::chrono::steady_clock::now();
    pass(c);
    c.kernel_us[which] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  };
  c.colcnt.assign((size_t) c.Lp * kMsaSlots, 0);
  if (host) twin(host_colcount, 0); else if ((st = msa_device_colcount(dev, c)) != P7X_OK) return st;

  c.wq.assign((size_t) N, (uint64_t) 1 << kMsaShift);
  c.rowsum.assign((size_t) N, 0); c.rowlen.assign((size_t) N, 0);
  if (weighting == 1) {
    weighting_columns(c, rf_mask, symfrac);
    if (host) twin(host_pbweight, 1); else if ((st = msa_device_pbweight(dev, c)) != P7X_OK) return st;
    finish_weights(c);
  }

  c.wcnt.assign((size_t) c.Lp * kMsaSlots, 0);
  if (host) twin(host_wcount, 2); else if ((st = msa_device_wcount(dev, c)) != P7X_OK) return st;

  if ((st = consensus_columns(c, rf_mask, symfrac)) != P7X_OK) return st;
  c.trq.assign((size_t) (c.M + 1) * 8, 0);
  c.taken.assign((size_t) (c.M + 1) * kMsaSlots, 0);
  if (host) twin(host_transitions, 3); else if ((st = msa_device_transitions(dev, c)) != P7X_OK) return st;

  c.emq.assign((size_t) (c.M + 1) * kMsaSlots, 0);
  for (int k = 1; k <= c.M; ++k)
    for (int a = 0; a < kMsaSlots; ++a)
      c.emq[(size_t) k * kMsaSlots + a] = c.wcnt[(size_t) c.map[k] * kMsaSlots + a] + c.taken[(size_t) k * kMsaSlots + a];
  return P7X_OK;
}

// the one conversion of the fixed-point sums: counts in double, a degenerate residue's weight spread over its residues
static void counts_as_double(const p7x_msacounts &c, std::vector<double> &em, std::vector<double> &tr)
{
  const Alphabet &abc = Alphabet::get(P7X_AMINO);
  const int M = c.M;
  em.assign((size_t) (M + 1) * 20, 0.0); tr.assign((size_t) (M + 1) * 7, 0.0);
  for (int k = 1; k <= M; ++k) {
    const uint64_t *q = c.emq.data() + (size_t) k * kMsaSlots;
    double *e = em.data() + (size_t) k * 20;
    for (int a = 0; a < 20; ++a) e[a] = std::ldexp((double) q[a], -kMsaShift);
    for (int x = 21; x <= 26; ++x) {
      if (!q[x]) continue;
      int nd = 0;
      for (int a = 0; a < 20; ++a) nd += abc.degen[x][a];
      const double share = std::ldexp((double) q[x], -kMsaShift) / (double) nd;
      for (int a = 0; a < 20; ++a) if (abc.degen[x][a]) e[a] += share;
    }
  }
  for (int k = 0; k <= M; ++k)
    for (int s = 0; s < 7; ++s) tr[(size_t) k * 7 + s] = std::ldexp((double) c.trq[(size_t) k * 8 + s], -kMsaShift);
  for (int k = 0; k <= M; ++k) tr[(size_t) k * 7 + 4] += std::ldexp((double) c.trq[(size_t) k * 8 + 7], kMsaSplit - kMsaShift);
}

} // namespace p7x

using namespace p7x;

extern "C" {

uint32_t p7x_msa_checksum(const uint8_t *ax, size_t n)
{
  uint32_t v = 0;
  for (size_t i = 0; i < n; ++i) { v += ax[i]; v += v << 10; v ^= v >> 6; }
  v += v << 3; v ^= v >> 11; v += v << 15;
  return v;
}

int p7x_msa_counts(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, const uint8_t *rf_mask, int weighting, double symfrac,
                   double fragthresh, int device, p7x_msacounts **out)
{
  if (!out) { set_error("p7x_msa_counts: bad arguments"); return P7X_EINVAL; }
  if (weighting != 0 && weighting != 1) { set_error("p7x_msa_counts: the weighting is 0 (none) or 1 (position-based)"); return P7X_EINVAL; }
  auto *c = new p7x_msacounts();
  const int st = msa_counts(abc_type, ax, N, L, rf_mask, weighting, symfrac, fragthresh, device, *c);
  if (st != P7X_OK) { delete c; return st; }
  *out = c;
  return P7X_OK;
}

void p7x_msacounts_destroy(p7x_msacounts *c) { delete c; }

int64_t p7x_msacounts_info(const p7x_msacounts *c, int which)
{
  if (!c) return -1;
  switch (which) {
  case 0: return c->N;
  case 1: return c->L;
  case 2: return c->M;
  case 3: return c->nwcols;
  case 4: return c->on_device;
  case 5: return c->nfrag;
  case 6: case 7: case 8: case 9: return (int64_t) (c->kernel_us[which - 6] * 1000.0);      // nanoseconds
  case 10: return (int64_t) (c->upload_us * 1000.0);
  default: return -1;
  }
}

int p7x_msacounts_get(const p7x_msacounts *c, int which, void *out, size_t cap_bytes)
{
  if (!c || !out) { set_error("p7x_msacounts_get: bad arguments"); return P7X_EINVAL; }
  const size_t L = (size_t) c->L, N = (size_t) c->N, M = (size_t) c->M;
  const void *src = nullptr; size_t bytes = 0;
  std::vector<double> em, tr;
  std::vector<int32_t> map1;
  switch (which) {
  case 0: src = c->colcnt.data(); bytes = L * kMsaSlots * sizeof(uint32_t); break;
  case 1: src = c->wq.data(); bytes = N * sizeof(uint64_t); break;
  case 2: src = c->wcnt.data(); bytes = L * kMsaSlots * sizeof(uint64_t); break;
  case 3: map1.assign(c->map.begin() + 1, c->map.begin() + 1 + M); src = map1.data(); bytes = M * sizeof(int32_t); break;
  case 4: src = c->emq.data(); bytes = (M + 1) * kMsaSlots * sizeof(uint64_t); break;
  case 5: src = c->trq.data(); bytes = (M + 1) * 8 * sizeof(uint64_t); break;
  case 6: counts_as_double(*c, em, tr); src = em.data(); bytes = em.size() * sizeof(double); break;
  case 7: counts_as_double(*c, em, tr); src = tr.data(); bytes = tr.size() * sizeof(double); break;
  case 8: src = c->wmask.data(); bytes = c->wmask.empty() ? 0 : L; break;
  case 9: src = c->frag.data(); bytes = N; break;
  default: set_error("p7x_msacounts_get: unknown array"); return P7X_EINVAL;
  }
  if (bytes > cap_bytes) { set_error("p7x_msacounts_get: the buffer is too small"); return P7X_EINVAL; }
  if (bytes) std::memcpy(out, src, bytes);
  return P7X_OK;
}

int p7x_msa_parameterize(const p7x_msacounts *c, const float *bg_f, int prior, int eff_mode, double eff_value, double ere, double esigma,
                         float *t, float *mat, float *ins, double *neff_out, double *t64, double *mat64)
{
  if (!c || !bg_f || !t || !mat || !ins) { set_error("p7x_msa_parameterize: bad arguments"); return P7X_EINVAL; }
  if (prior != 0 && prior != 1) { set_error("the prior is 0 (the alphabet's Dirichlets) or 1 (Laplace)"); return P7X_EINVAL; }
  if (eff_mode < 0 || eff_mode > 2 || (eff_mode == 2 && !(eff_value > 0.0))) { set_error("bad effective sequence number"); return P7X_EINVAL; }
  const int M = c->M;
  const double N = (double) c->N;
  std::vector<double> em, tr;
  counts_as_double(*c, em, tr);
  double bg[20];
  for (int a = 0; a < 20; ++a) bg[a] = (double) bg_f[a];
  double neff = N;
  if (eff_mode == 2) neff = eff_value;
  else if (eff_mode == 1) {
    if (!(ere > 0.0)) ere = 0.59;
    const double target = std::max(ere, (esigma + std::log2((double) M * ((double) M + 1.0) / 2.0)) / (double) M);
    if (scaled_relent(em, M, 1.0, bg, prior) > target) {
      int steps = 1;
      while (std::ldexp(N, -steps) >= 0.005) ++steps;
      double lo = 0.0, hi = N, mid = 0.0;
      for (int it = 0; it < steps; ++it) {
        mid = 0.5 * (lo + hi);
        if (scaled_relent(em, M, mid / N, bg, prior) > target) hi = mid; else lo = mid;
      }
      neff = mid;
    }
  }
  const double scale = neff / N;
  float insert[20];
  {
    double z = 0.0;
    for (int a = 0; a < 20; ++a) z += std::exp(-kInsertNegLog[a]);
    for (int a = 0; a < 20; ++a) insert[a] = (float) (std::exp(-kInsertNegLog[a]) / z);
  }
  for (int k = 0; k <= M; ++k) {
    float *m = mat + (size_t) k * 20, *tk = t + (size_t) k * 7;
    if (k == 0) { for (int a = 0; a < 20; ++a) m[a] = 0.0f; m[0] = 1.0f; if (mat64) { std::memset(mat64, 0, sizeof(double) * 20); mat64[0] = 1.0; } }
    else {
      double cnt[20], p[20];
      for (int a = 0; a < 20; ++a) cnt[a] = em[(size_t) k * 20 + a] * scale;
      emission_posterior(cnt, prior, p);
      for (int a = 0; a < 20; ++a) m[a] = (float) p[a];
      if (mat64) std::memcpy(mat64 + (size_t) k * 20, p, sizeof(p));
    }
    std::memcpy(ins + (size_t) k * 20, insert, sizeof(insert));
    double v[7];
    for (int s = 0; s < 7; ++s) v[s] = tr[(size_t) k * 7 + s] * scale + (prior == 1 ? 1.0 : kTransPrior[s]);
    const double zm = v[0] + v[1] + v[2], zi = v[3] + v[4], zd = v[5] + v[6];
    v[0] /= zm; v[1] /= zm; v[2] /= zm; v[3] /= zi; v[4] /= zi; v[5] /= zd; v[6] /= zd;
    if (k == M) { const double z = v[0] + v[1]; v[0] /= z; v[1] /= z; v[2] = 0.0; }
    if (k == M || k == 0) { v[5] = 1.0; v[6] = 0.0; }
    for (int s = 0; s < 7; ++s) tk[s] = (float) v[s];
    if (t64) std::memcpy(t64 + (size_t) k * 7, v, sizeof(v));
  }
  if (neff_out) *neff_out = neff;
  return P7X_OK;
}

} // extern "C"
