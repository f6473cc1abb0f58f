// p7x_hostdp.hpp -- what the two host translation units of domain definition share (private to them): the query in a
// given configuration, the DP matrix, traces, and the entry points p7x_domaindef.cpp defines for the long-target tail
// (p7x_longtarget_host.cpp).
#pragma once
#include "p7x_host.hpp"
#include <algorithm>
#include <cstring>

namespace p7x {

int vit_pick_C(int M);          // p7x_vitfwd.hip: nodes per lane of the wave-per-target kernels, a function of M alone

enum { sM = 1, sD = 2, sI = 3, sS = 4, sN = 5, sB = 6, sE = 7, sC = 8, sT = 9, sJ = 10 };   // p7T_* (p7_trace.pxd)
enum { xE_ = 0, xN_ = 1, xJ_ = 2, xB_ = 3, xC_ = 4, xS_ = 5, NX = 6 };

// ---------------------------------------------------------------- the query in a given configuration
// Long-target (nhmmer) variant of envelope rescoring, upstream rescore_isolated_domain(..., long_target = TRUE, ...)
struct LongTargetOpts {
  bool do_null2 = true;                // false: upstream passes scores_arr == NULL and the model is not re-parameterised
  const float *match_prob = nullptr;   // [M+1][K] match emission probabilities of the core model (fwd_emissions_arr)
  int max_env_extra = 20;              // an envelope is trimmed to its alignment +- this many residues
};
// While one lives, the domain-definition calls of this thread (domaindef_from_regions, domaindef_by_posterior_heuristics,
// domaindef_finish_multi) rescore their envelopes the long-target way
struct LongTargetScope { explicit LongTargetScope(const LongTargetOpts &lt); ~LongTargetScope(); };

struct Model {
  const Profile *p;
  int M;
  float xf[4][2];                 // [E,N,J,C][MOVE,LOOP] for the current mode / length
  const float *rf_over = nullptr; // [Kp][M+1] replacement match odds (long targets: composition-adjusted background)
  const LongTargetOpts *lt = nullptr;
  const float *tf(int t) const { return p->tf.data() + (size_t) t * (M + 1); }
  const float *rf(int x) const { return (rf_over ? rf_over : p->rf_.data()) + (size_t) x * (M + 1); }
  // Order of operations.  The sums whose result depends on the order of the float additions -- the D->D chains, the row
  // sums xE / xB, the null2 expectation -- run in the order of the device kernels (p7x_envelope.hip, p7x_wave.hpp): lane z
  // of a 64-lane wavefront owns the C consecutive nodes zC+1 .. zC+C, walks them in order, and the lanes are combined by
  // the wavefront's scan / reduction trees (lanes_scan_up / lanes_scan_down / lanes_sum, p7x_domaindef.cpp).  Host twin and
  // device therefore produce the same bits, and every discrete decision taken from them (optimal-accuracy traceback, the
  // stochastic tracebacks' choices) is the same decision.  Upstream's own order (four striped lanes, serial D->D sweeps)
  // is a third one; what the fixtures pin is reproduced by all of them.
  int C = 1;                                        // nodes per lane: vit_pick_C(M), the device image's choice
  float ddprod[64];                                 // product of the D->D transitions of a lane's nodes, in node order
  // upstream = true (the default; option "host_order" = 1 selects the device's order instead): those sums run as
  // impl_sse runs them -- four stripes, node k in stripe (k-1)/Q at position (k-1)%Q, serial D->D sweeps, row sums
  // stripe by stripe and then (s0+s1)+(s2+s3) -- so that every float, and with it every decision, is the reference's.
  // The host stage uses it for whatever it computes itself, in particular for the envelopes and regions the device
  // flags as too close to call (near-tie guards of p7x_envelope.hip / p7x_ensemble.hip).
  bool upstream = true;
  int Q = 0;
  std::vector<float> st;                            // [8][Q][4] transitions in the striped layout (padding: 0)
  const float *sT(int t) const { return st.data() + (size_t) t * Q * 4; }
  // [Kp][Q][4] match odds in the striped layout, of whatever rf() currently stands for (rebuilt when that changes: the
  // long-target path swaps in composition-adjusted odds per envelope)
  mutable std::vector<float> sr; mutable const float *sr_of = nullptr;
  const float *sR(int x) const
  {
    const float *base = rf(0);
    if (sr_of != base || sr.size() != (size_t) p->Kp * Q * 4) {
      sr.assign((size_t) p->Kp * Q * 4, 0.0f);
      for (int y = 0; y < p->Kp; ++y) {
        const float *r = rf(y);
        float *d = sr.data() + (size_t) y * Q * 4;
        for (int q = 0; q < Q; ++q) for (int z = 0; z < 4; ++z) { const int k = q + 1 + z * Q; if (k <= M) d[q * 4 + z] = r[k]; }
      }
      sr_of = base;
    }
    return sr.data() + (size_t) x * Q * 4;
  }
  std::vector<float> rfT;                           // [M+1][kKpad] match odds, residue-minor (null2_by_trace)
  static constexpr int kKpad = 24;
  void prepare_rfT()
  {
    rfT.assign((size_t) (M + 1) * kKpad, 0.0f);
    for (int x = 0; x < p->K && x < kKpad; ++x) { const float *r = rf(x); for (int k = 1; k <= M; ++k) rfT[(size_t) k * kKpad + x] = r[k]; }
  }
  void prepare(int order = -1)
  {
    upstream = order >= 0 ? order == 0 : debug_opt(OPT_HOST_ORDER) <= 0;
    Q = p->Q4();
    st.assign((size_t) 8 * Q * 4, 0.0f);
    for (int t = 0; t < 8; ++t) {
      const float *src = tf(t);
      const int last = (t == 4 || t == 7) ? M - 1 : M;        // M -> D and D -> D do not leave node M
      for (int q = 0; q < Q; ++q) for (int z = 0; z < 4; ++z) { const int k = q + 1 + z * Q; if (k <= last) st[((size_t) t * Q + q) * 4 + z] = src[k]; }
    }
    C = vit_pick_C(M);
    if (C <= 0) C = (M + 63) / 64;                  // beyond the device kernels' reach: the same rule, continued
    const float *tDD = tf(7);
    for (int z = 0; z < 64; ++z) {
      float pr = 1.0f;
      for (int c = 0; c < C; ++c) { const int k = z * C + c + 1; pr *= (k <= M ? tDD[k] : 0.0f); }
      ddprod[z] = pr;
    }
  }
  void configure(bool multihit, int L)
  { // p7_oprofile_ReconfigMultihit / ReconfigUnihit (+ ReconfigLength)
    const float nj = multihit ? 1.0f : 0.0f;
    xf[XE][MOVE] = multihit ? 0.5f : 1.0f;
    xf[XE][LOOP] = multihit ? 0.5f : 0.0f;
    const float pmove = (2.0f + nj) / ((float) L + 2.0f + nj), ploop = 1.0f - pmove;
    for (int s : {XN, XJ, XC}) { xf[s][MOVE] = pmove; xf[s][LOOP] = ploop; }
  }
};

// DP matrix: the special rows 0..L and, per DP row, three arrays of M+2 floats (M, I, D).  The full-matrix engines keep
// every DP row; the rows-only (parser) engines keep two rolling ones, or none.
struct Matrix {
  int M = 0, L = 0;
  std::vector<float> m, i, d, x, scratch;
  float totscale = 0.0f;
  bool own_scales = false;
  void resize(int M_, int L_, int dp_rows = -1)       // dp_rows < 0: all L+1
  {
    M = M_; L = L_;
    const size_t n = (size_t) (dp_rows < 0 ? L + 1 : dp_rows) * (M + 2);
    if (m.size() < n) { m.resize(n); i.resize(n); d.resize(n); }
    if (x.size() < (size_t) (L + 1) * NX) x.resize((size_t) (L + 1) * NX);
    if (scratch.size() < (size_t) (M + 4) + 4 * (size_t) (L + 1)) scratch.resize((size_t) (M + 4) + 4 * (size_t) (L + 1));
  }
  float *M_(int r) { return m.data() + (size_t) r * (M + 2); }
  float *I_(int r) { return i.data() + (size_t) r * (M + 2); }
  float *D_(int r) { return d.data() + (size_t) r * (M + 2); }
  const float *M_(int r) const { return m.data() + (size_t) r * (M + 2); }
  const float *I_(int r) const { return i.data() + (size_t) r * (M + 2); }
  const float *D_(int r) const { return d.data() + (size_t) r * (M + 2); }
  float &X(int r, int s) { return x[(size_t) r * NX + s]; }
  float X(int r, int s) const { return x[(size_t) r * NX + s]; }
};

// ---------------------------------------------------------------- traces
struct Trace {
  std::vector<int8_t> st; std::vector<int> k, i; std::vector<float> pp;
  int ndom = 0;
  std::vector<int> tfrom, tto, sqfrom, sqto, hmmfrom, hmmto;
  void clear() { st.clear(); k.clear(); i.clear(); pp.clear(); ndom = 0; tfrom.clear(); tto.clear(); sqfrom.clear(); sqto.clear(); hmmfrom.clear(); hmmto.clear(); }
  void append(int s, int kk, int ii, float p)
  { // p7_trace_AppendWithPP
    int iv = 0, kv = 0; float pv = 0.0f;
    switch (s) {
      case sN: case sC: case sJ:
        if (!st.empty() && st.back() == s) { iv = ii; pv = p; }
        break;
      case sD: kv = kk; break;
      case sM: case sI: iv = ii; kv = kk; pv = p; break;
      default: break;
    }
    st.push_back((int8_t) s); k.push_back(kv); i.push_back(iv); pp.push_back(pv);
  }
  void reverse()
  { // p7_trace_Reverse: N,C,J emit on transition, so their i/pp move one step when the order flips
    const int N = (int) st.size();
    for (int z = 0; z < N; ++z)
      if ((st[z] == sN || st[z] == sC || st[z] == sJ) && z + 1 < N && st[z] == st[z + 1]) {
        if (i[z] == 0 && i[z + 1] > 0) { i[z] = i[z + 1]; i[z + 1] = 0; pp[z] = pp[z + 1]; pp[z + 1] = 0.0f; }
      }
    std::reverse(st.begin(), st.end()); std::reverse(k.begin(), k.end());
    std::reverse(i.begin(), i.end()); std::reverse(pp.begin(), pp.end());
  }
  void index()
  { // p7_trace_Index
    ndom = 0; tfrom.clear(); tto.clear(); sqfrom.clear(); sqto.clear(); hmmfrom.clear(); hmmto.clear();
    for (int z = 0; z < (int) st.size(); ++z)
      switch (st[z]) {
        case sB: tfrom.push_back(z); tto.push_back(0); sqfrom.push_back(0); sqto.push_back(0); hmmfrom.push_back(0); hmmto.push_back(0); break;
        case sM:
          if (sqfrom[ndom] == 0) sqfrom[ndom] = i[z];
          if (hmmfrom[ndom] == 0) hmmfrom[ndom] = k[z];
          sqto[ndom] = i[z]; hmmto[ndom] = k[z];
          break;
        case sE: tto[ndom] = z; ndom++; break;
        default: break;
      }
  }
};

// (These types have external linkage now that two units share them: their names must be unique in namespace p7x across the
// library -- p7x_pipeline.hip has a Workspace of its own.)
struct DomainWorkspace { Matrix fwd, bck; Trace tr; std::vector<float> wm, wi; };

// ---------------------------------------------------------------- p7x_domaindef.cpp, for the long-target tail
// p7_ForwardParser / p7_BackwardParser in the device's summation order (whatever om.upstream says): the special-state
// rows only, (L+1) x [E,N,J,B,C,SCALE], on two rolling DP rows.  dsq[1..L]; fx: Forward's rows (the scale factors).
int forward_parser_lanes(const Model &om, const uint8_t *dsq, int L, std::vector<float> &fx, float *ret_sc);
int backward_parser_lanes(const Model &om, const uint8_t *dsq, int L, const std::vector<float> &fx, std::vector<float> &bx);
float bias_filter_score(const Profile &p, const uint8_t *dsq, int64_t L);       // p7_bg_FilterScore, dsq[1..L]
void reparameterize(const Profile &p, const LongTargetOpts &lt, const uint8_t *dsq, int n, int i, int j, std::vector<float> &rf);
int rescore_isolated_domain(const Profile &p, Model &om, const uint8_t *dsq, int L, int i, int j, bool null2_is_done,
                            DomainWorkspace &ws, DomainDefResult &dd);
void make_alidisplay(const Profile &p, const Trace &tr, const uint8_t *dsq, int L, Domain &dom);

} // namespace p7x
