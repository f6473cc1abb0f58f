// p7x_logdp.cpp -- hmmalign's float64 log-space host twin (TraceAligner(logspace=True)): Forward, Backward,
// posterior decoding, optimal accuracy and its traceback of one whole sequence, for the sequences on which the scaled
// float32 engines lose a path -- two strong domains of one family, where "first copy in N, second copy aligned" lies
// below the float32 range of a row scaled for "first copy aligned".  Everything is a float64 logarithm of the profile's
// float32 odds tables, the log-sum is exact (max + log1p(exp(-d)), no table), and no row is renormalised: there are no
// scale factors to leave behind and nothing overflows.  The device kernel (p7x_alignlog.hip) states the same mathematics;
// p7x_logdp.hpp holds what the two share (the tables, the log-sum, the traceback over the optimal-accuracy matrix).
#include "p7x_logdp.hpp"
#include "p7x_hostdp.hpp"
#include <cmath>

namespace p7x {

void LogTables::build(const Profile &p, int L)
{
  M = p.M; Kp = p.Kp; W = M + 2; Q = p.Q4();
  auto lg = [](float v) { return v > 0.0f ? std::log((double) v) : kLogZero; };
  t.assign((size_t) 8 * W, kLogZero);
  for (int s = 0; s < 8; ++s)
    for (int k = 1; k <= M; ++k) t[(size_t) s * W + k] = lg(p.tf[(size_t) s * (M + 1) + k]);
  e.assign((size_t) Kp * W, kLogZero);
  for (int x = 0; x < Kp; ++x)
    for (int k = 1; k <= M; ++k) e[(size_t) x * W + k] = lg(p.rf_[(size_t) x * (M + 1) + k]);
  // the sequence's own length model, unihit (p7_ReconfigUnihit + ReconfigLength): the engines' float32 constants
  const float pmove = 2.0f / ((float) L + 2.0f), ploop = 1.0f - pmove;
  move = lg(pmove); loop = lg(ploop);
}

namespace {

struct LogWorkspace { std::vector<double> pm, pi, om, oi, od, row, x; };

// D(k) = logsum(M(k-1) + md(k-1), D(k-1) + dd(k-1)), k = 2..M, and the row's E
inline double forward_close_row(const LogTables &T, const double *mc, double *dc)
{
  const int M = T.M;
  const double *md = T.tr(tMD), *dd = T.tr(tDD);
  dc[0] = dc[1] = kLogZero;
  double xE = mc[1];
  for (int k = 2; k <= M; ++k) {
    dc[k] = logsum(mc[k - 1] + md[k - 1], dc[k - 1] + dd[k - 1]);
    xE = logsum(xE, logsum(mc[k], dc[k]));
  }
  dc[M + 1] = kLogZero;
  return xE;
}

} // namespace

int align_trace_logspace(const Profile &p, const uint8_t *dsq1, int L, AlignTrace &out)
{
  out = AlignTrace{};
  if (L <= 0) return P7X_OK;
  thread_local LogWorkspace ws;
  struct Shrink { LogWorkspace &ws; ~Shrink() { if (ws.pm.capacity() * sizeof(double) * 5 > ((size_t) 256 << 20)) ws = LogWorkspace(); } } shrink{ ws };
  LogTables T;
  T.build(p, L);
  const int M = T.M, W = T.W;
  const size_t cells = (size_t) (L + 1) * W;
  ws.pm.assign(cells, kLogZero); ws.pi.assign(cells, kLogZero);
  ws.row.assign((size_t) 8 * W, kLogZero);
  ws.x.assign((size_t) (L + 1) * LX_N, kLogZero);
  double *X = ws.x.data();
  const double *bm = T.tr(tBM), *mm = T.tr(tMM), *im = T.tr(tIM), *dm = T.tr(tDM), *md = T.tr(tMD), *mi = T.tr(tMI), *ii = T.tr(tII), *dd = T.tr(tDD);

  // ---- Forward: M and I of every row stay (the posteriors are formed from them), D rolls
  double *dprev = ws.row.data(), *dcur = dprev + W;
  X[LX_FN] = 0.0; X[LX_FB] = T.move;
  for (int i = 1; i <= L; ++i) {
    const double *e = T.er(dsq1[i]);
    const double *mp = ws.pm.data() + (size_t) (i - 1) * W, *ip = ws.pi.data() + (size_t) (i - 1) * W;
    double *mc = ws.pm.data() + (size_t) i * W, *ic = ws.pi.data() + (size_t) i * W;
    const double xB = X[(size_t) (i - 1) * LX_N + LX_FB];
    for (int k = 1; k <= M; ++k) {
      mc[k] = e[k] + logsum(logsum(xB + bm[k], mp[k - 1] + mm[k]), logsum(ip[k - 1] + im[k], dprev[k - 1] + dm[k]));
      ic[k] = logsum(mp[k] + mi[k], ip[k] + ii[k]);
    }
    const double xE = forward_close_row(T, mc, dcur);
    double *x = X + (size_t) i * LX_N, *xp = x - LX_N;
    x[LX_FN] = xp[LX_FN] + T.loop;
    x[LX_FC] = logsum(xp[LX_FC] + T.loop, xE);
    x[LX_FB] = x[LX_FN] + T.move;
    std::swap(dprev, dcur);
  }
  const double tot = X[(size_t) L * LX_N + LX_FC] + T.move;
  if (!(tot > kLogZero) || std::isnan(tot)) return P7X_EINVAL;     // no path emits this sequence at all
  out.fwdsc = (float) tot;

  // ---- Backward on rolling rows; row i's posteriors replace Forward's row i as soon as both are known
  double *bmn = ws.row.data() + 2 * (size_t) W, *bin = bmn + W, *bdc = bin + W, *bmc = bdc + W, *bic = bmc + W, *em = bic + W;
  auto close_row = [&](double xE, const double *a_m, const double *a_d, double *mc, double *dc) {
    dc[M + 1] = kLogZero;
    for (int k = M; k >= 1; --k) {
      const double down = md[k] + dc[k + 1];
      dc[k] = logsum(a_d ? logsum(xE, a_d[k]) : xE, dd[k] + dc[k + 1]);
      mc[k] = logsum(a_m ? logsum(xE, a_m[k]) : xE, down);
    }
    mc[0] = mc[M + 1] = dc[0] = kLogZero;
  };
  auto decode_row = [&](int i, const double *bM, const double *bI) {
    double *fm = ws.pm.data() + (size_t) i * W, *fi = ws.pi.data() + (size_t) i * W;
    for (int k = 1; k <= M; ++k) { fm[k] = std::exp(fm[k] + bM[k] - tot); fi[k] = std::exp(fi[k] + bI[k] - tot); }
    fm[0] = fi[0] = fm[M + 1] = fi[M + 1] = 0.0;
  };
  {
    double *x = X + (size_t) L * LX_N;
    x[LX_BC] = T.move; x[LX_BN] = kLogZero;
    close_row(x[LX_BC], nullptr, nullptr, bmn, bdc);
    for (int k = 0; k <= M + 1; ++k) bin[k] = kLogZero;
    decode_row(L, bmn, bin);
  }
  std::vector<double> &am_v = ws.od;           // borrowed until optimal accuracy lays its matrix out
  am_v.assign((size_t) 2 * W, kLogZero);
  double *a_m = am_v.data(), *a_d = a_m + W;
  for (int i = L - 1; i >= 0; --i) {
    const double *e = T.er(dsq1[i + 1]);
    double xB = kLogZero;
    for (int k = 1; k <= M; ++k) { em[k] = e[k] + bmn[k]; xB = logsum(xB, bm[k] + em[k]); }
    em[M + 1] = kLogZero;
    double *x = X + (size_t) i * LX_N, *xn = x + LX_N;
    x[LX_BN] = logsum(xB + T.move, xn[LX_BN] + T.loop);
    if (i == 0) break;
    x[LX_BC] = xn[LX_BC] + T.loop;
    for (int k = 1; k <= M; ++k) {
      a_m[k] = logsum(mm[k + 1] + em[k + 1], mi[k] + bin[k]);
      a_d[k] = dm[k + 1] + em[k + 1];
      bic[k] = logsum(im[k + 1] + em[k + 1], ii[k] + bin[k]);
    }
    close_row(x[LX_BC], a_m, a_d, bmc, bdc);
    decode_row(i, bmc, bic);
    std::swap(bmn, bmc); std::swap(bin, bic);
  }
  // posteriors of the emitting special states: residue i from N / C
  std::vector<double> ppN((size_t) L + 1, 0.0), ppC((size_t) L + 1, 0.0);
  for (int i = 1; i <= L; ++i) {
    const double *x = X + (size_t) i * LX_N, *xp = x - LX_N;
    ppN[(size_t) i] = std::exp(xp[LX_FN] + T.loop + x[LX_BN] - tot);
    ppC[(size_t) i] = std::exp(xp[LX_FC] + T.loop + x[LX_BC] - tot);
  }
  { double *m0 = ws.pm.data(), *i0 = ws.pi.data(); for (int k = 0; k <= M + 1; ++k) m0[k] = i0[k] = 0.0; }

  // ---- optimal accuracy in float64 on the float64 posteriors (delta = 0 where the transition exists, -inf elsewhere)
  ws.om.assign(cells, kLogZero); ws.oi.assign(cells, kLogZero); ws.od.assign(cells, kLogZero);
  std::vector<double> oN((size_t) L + 1, 0.0), oC((size_t) L + 1, kLogZero), oE((size_t) L + 1, kLogZero);
  OaGates G;
  G.build(p);
  for (int i = 1; i <= L; ++i) {
    const double *mp = ws.om.data() + (size_t) (i - 1) * W, *ip = ws.oi.data() + (size_t) (i - 1) * W, *dp = ws.od.data() + (size_t) (i - 1) * W;
    const double *pm = ws.pm.data() + (size_t) i * W, *pi = ws.pi.data() + (size_t) i * W;
    double *mc = ws.om.data() + (size_t) i * W, *ic = ws.oi.data() + (size_t) i * W, *dc = ws.od.data() + (size_t) i * W;
    const double xB = oN[(size_t) i - 1];
    double xE = kLogZero;
    for (int k = 1; k <= M; ++k) {
      const uint8_t g = G.g[(size_t) k];
      double sv = oa_gate(g, tBM, xB);
      sv = std::fmax(sv, oa_gate(g, tMM, mp[k - 1]));
      sv = std::fmax(sv, oa_gate(g, tIM, ip[k - 1]));
      sv = std::fmax(sv, oa_gate(g, tDM, dp[k - 1]));
      mc[k] = sv + pm[k];
      ic[k] = std::fmax(oa_gate(g, tMI, mp[k]), oa_gate(g, tII, ip[k])) + pi[k];
      if (k > 1) { const uint8_t gp = G.g[(size_t) k - 1]; dc[k] = std::fmax(oa_gate(gp, tMD, mc[k - 1]), oa_gate(gp, tDD, dc[k - 1])); }
      xE = std::fmax(xE, std::fmax(mc[k], dc[k]));
    }
    oE[(size_t) i] = xE;
    oC[(size_t) i] = std::fmax(oC[(size_t) i - 1] + ppC[(size_t) i], xE);
    oN[(size_t) i] = oN[(size_t) i - 1] + ppN[(size_t) i];
  }
  out.oasc = (float) oC[(size_t) L];

  // ---- traceback (the precedence of oa_trace, p7x_domaindef.cpp)
  OaView v;
  v.M = M; v.W = W; v.Q = T.Q; v.L = L;
  v.om = ws.om.data(); v.oi = ws.oi.data(); v.od = ws.od.data(); v.pm = ws.pm.data(); v.pi = ws.pi.data();
  v.oN = oN.data(); v.oC = oC.data(); v.oE = oE.data(); v.ppN = ppN.data(); v.ppC = ppC.data(); v.g = G.g.data();
  Trace tr;
  OaNoGuard ng;
  if (!oa_logspace_trace(v, ng, [&](int s, int k, int i, double pp) { tr.append(s, k, i, (float) pp); })) return P7X_EINVAL;
  tr.reverse();
  out.st = std::move(tr.st); out.k = std::move(tr.k); out.i = std::move(tr.i); out.pp = std::move(tr.pp);
  return P7X_OK;
}

} // namespace p7x
