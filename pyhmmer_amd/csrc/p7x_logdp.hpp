// p7x_logdp.hpp -- what hmmalign's float64 log-space host twin (p7x_logdp.cpp) and its device kernel (p7x_alignlog.hip)
// share: the logarithms of the profile's float32 odds tables, the exact log-sum, the gates of the optimal-accuracy
// recursion and its traceback.  The traceback is one function for both: they differ in how they read the matrices (View)
// and in what they do with a close call (Guard).
#pragma once
#include "p7x_internal.hpp"
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define P7X_HD __host__ __device__
#else
#define P7X_HD
#endif

namespace p7x {

constexpr double kLogZero = -__builtin_inf();

// log(exp(a) + exp(b)), exactly rounded parts and no table: max + log1p(exp(-d)); log 0 = -inf on either side
P7X_HD inline double logsum(double a, double b)
{
  const double hi = a > b ? a : b, lo = a > b ? b : a;
  if (!(lo > kLogZero)) return hi;
  return hi + log1p(exp(lo - hi));
}

// special-state values kept per row, in logs: Forward's N B C, Backward's N C
enum { LX_FN = 0, LX_FB, LX_FC, LX_BN, LX_BC, LX_N = 8 };

// float64 logs of the un-striped tables: t[s][k] (the eight transitions, p7x_internal.hpp's order) and e[x][k], rows of
// W = M + 2 with -inf at 0 and M + 1; move / loop of the unihit length model of a sequence of L residues
struct LogTables {
  int M = 0, Kp = 0, W = 0, Q = 0;
  std::vector<double> t, e;
  double move = 0.0, loop = 0.0;
  void build(const Profile &p, int L);
  const double *tr(int s) const { return t.data() + (size_t) s * W; }
  const double *er(int x) const { return e.data() + (size_t) x * W; }
};

// Which of a node's eight transitions exist (probability > 0): bit s of g[k]
struct OaGates {
  std::vector<uint8_t> g;
  void build(const Profile &p)
  {
    g.assign((size_t) p.M + 2, 0);
    for (int s = 0; s < 8; ++s)
      for (int k = 1; k <= p.M; ++k) if (p.tf[(size_t) s * (p.M + 1) + k] > 0.0f) g[(size_t) k] |= (uint8_t) (1u << s);
  }
};
P7X_HD inline double oa_gate(unsigned g, int s, double v) { return (g >> s) & 1u ? v : kLogZero; }

// p7T_* state codes of a trace step
enum { LT_M = 1, LT_D = 2, LT_I = 3, LT_S = 4, LT_N = 5, LT_B = 6, LT_E = 7, LT_C = 8, LT_T = 9 };

// The host's view of the matrices: rows of W doubles, specials per row
struct OaView {
  int M = 0, W = 0, Q = 0, L = 0;
  const double *om = nullptr, *oi = nullptr, *od = nullptr, *pm = nullptr, *pi = nullptr;
  const double *oN = nullptr, *oC = nullptr, *oE = nullptr, *ppN = nullptr, *ppC = nullptr;
  const uint8_t *g = nullptr;
  double oM(int i, int k) const { return om[(size_t) i * W + k]; }
  double oI(int i, int k) const { return oi[(size_t) i * W + k]; }
  double oD(int i, int k) const { return od[(size_t) i * W + k]; }
  double pM(int i, int k) const { return pm[(size_t) i * W + k]; }
  double pI(int i, int k) const { return pi[(size_t) i * W + k]; }
  double xN(int i) const { return oN[i]; }
  double xC(int i) const { return oC[i]; }
  double xE(int i) const { return oE[i]; }
  double pN(int i) const { return ppN[i]; }
  double pC(int i) const { return ppC[i]; }
  unsigned gates(int k) const { return g[k]; }
  // E <- M / D of row i in upstream's striped visiting order (vector q outer, its four lanes inner, M before D): a later
  // match cell takes over on a tie, a delete cell only when it is larger
  template <class Guard> void pick_E(int i, int *k, int *s, Guard &) const
  {
    double mx = kLogZero; int smax = -1, kmax = 0;
    for (int q = 0; q < Q; ++q) {
      for (int z = 0; z < 4; ++z) { const int kk = z * Q + q + 1; if (kk <= M && oM(i, kk) >= mx) { mx = oM(i, kk); smax = LT_M; kmax = kk; } }
      for (int z = 0; z < 4; ++z) { const int kk = z * Q + q + 1; if (kk <= M && oD(i, kk) >  mx) { mx = oD(i, kk); smax = LT_D; kmax = kk; } }
    }
    *k = kmax; *s = smax;
  }
};

struct OaNoGuard {
  P7X_HD void tie(double, double) {}
  P7X_HD void digit(double) {}
};

// p7_OATrace over the float64 matrices, with oa_trace()'s precedence (p7x_domaindef.cpp): M <- M, I, D, B (the first
// maximum); D <- M unless D is larger; I <- M unless I is larger; C <- C only when larger than E; B <- N (unihit: J is
// closed).  emit(state, k, i, posterior) receives the steps in traceback order, Trace::append's rules still to apply.
// false: the matrix does not hold a path (cannot happen with a finite Forward score).
template <class View, class Guard, class Emit>
P7X_HD inline bool oa_logspace_trace(const View &v, Guard &guard, Emit emit)
{
  int i = v.L, k = 0, s0 = LT_C;
  emit((int) LT_T, k, i, 0.0);
  emit((int) LT_C, k, i, 0.0);
  for (long step = 0, cap = 2L * ((long) v.L + v.M) + 16; s0 != LT_S; ++step) {
    if (step > cap) return false;
    int s1 = -1;
    switch (s0) {
      case LT_M: {
        if (i < 1 || k < 1) return false;
        const unsigned g = v.gates(k);
        // the first maximum of (M, I, D, B) and the runner-up, without an indexed array (the device keeps no private segment)
        double bv = oa_gate(g, tMM, v.oM(i - 1, k - 1)), second = kLogZero;
        int bs = LT_M;
        auto consider = [&](double pv, int st) {
          if (pv > bv) { second = second > bv ? second : bv; bv = pv; bs = st; }
          else second = second > pv ? second : pv;
        };
        consider(oa_gate(g, tIM, v.oI(i - 1, k - 1)), LT_I);
        consider(oa_gate(g, tDM, v.oD(i - 1, k - 1)), LT_D);
        consider(oa_gate(g, tBM, v.xN(i - 1)), LT_B);
        guard.tie(bv, second);
        s1 = bs; k--; i--;
        break;
      }
      case LT_D: {
        if (k < 2) return false;
        const unsigned g = v.gates(k - 1);
        const double p0 = oa_gate(g, tMD, v.oM(i, k - 1)), p1 = oa_gate(g, tDD, v.oD(i, k - 1));
        guard.tie(p0, p1);
        s1 = (p0 >= p1) ? LT_M : LT_D; k--;
        break;
      }
      case LT_I: {
        if (i < 1) return false;
        const unsigned g = v.gates(k);
        const double p0 = oa_gate(g, tMI, v.oM(i - 1, k)), p1 = oa_gate(g, tII, v.oI(i - 1, k));
        guard.tie(p0, p1);
        s1 = (p0 >= p1) ? LT_M : LT_I; i--;
        break;
      }
      case LT_N: s1 = (i == 0) ? LT_S : LT_N; break;
      case LT_C: {
        if (i < 1) return false;
        const double p0 = v.xC(i - 1) + v.pC(i), p1 = v.xE(i);
        guard.tie(p0, p1);
        s1 = (p0 > p1) ? LT_C : LT_E;
        break;
      }
      case LT_E: v.pick_E(i, &k, &s1, guard); break;
      case LT_B: s1 = LT_N; break;
      default: return false;
    }
    if (s1 == -1) return false;
    double pp = 0.0;
    if (s1 == LT_M) pp = v.pM(i, k);
    else if (s1 == LT_I) pp = v.pI(i, k);
    else if (s1 == LT_N && s0 == LT_N) pp = v.pN(i);
    else if (s1 == LT_C && s0 == LT_C) pp = v.pC(i);
    if (s1 == LT_M || s1 == LT_I || ((s1 == LT_N || s1 == LT_C) && s1 == s0 && i > 0)) guard.digit(pp);
    emit(s1, k, i, pp);
    if ((s1 == LT_N || s1 == LT_C) && s1 == s0) i--;
    s0 = s1;
  }
  return true;
}

} // namespace p7x
