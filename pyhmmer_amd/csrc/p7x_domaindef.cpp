// p7x_domaindef.cpp -- host-side domain definition for the targets that survive the Forward filter.
//
// Restates upstream p7_domaindef.c:p7_domaindef_ByPosteriorHeuristics (reference
// include/libhmmer/p7_domaindef.pxd:23-72) and the routines it drives:
//   impl_sse/decoding.c   p7_DomainDecoding, p7_Decoding
//   impl_sse/fwdback.c    p7_Forward, p7_Backward (full matrices, on envelopes only)
//   impl_sse/null2.c      p7_Null2_ByExpectation, p7_Null2_ByTrace
//   impl_sse/optacc.c     p7_OptimalAccuracy, p7_OATrace
//   impl_sse/stotrace.c   p7_StochasticTrace          (Easel "fast" LCG, re-seeded per region)
//   p7_spensemble.c       p7_spensemble_Add/_Cluster  (Easel single-linkage clustering)
//   p7_trace.c            p7_trace_Index;  p7_alidisplay.c p7_alidisplay_Create
// Matrices are un-striped (node k at index k).  Where upstream's results depend on the order in which
// the striped SSE code visits cells (tie-breaks in the OA traceback, cumulative sums in the stochastic
// traceback) that visiting order is reproduced.  Runs only for ~1e-5 of random targets plus true homologs.
#include "p7x_hostdp.hpp"
#include "p7x_choice.hpp"
#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace p7x {

// optional host profile (option "host_profile"): accumulated nanoseconds per phase, printed by host_prof_dump()
#define g_prof_on (debug_opt(OPT_HOST_PROFILE) > 0)
static std::atomic<long long> g_prof_ns[12];
static const char *g_prof_name[12] = { "domain_decoding", "region_forward", "stochastic_traces", "null2_by_trace", "cluster",
                                        "env_forward", "env_backward", "env_decoding", "optimal_accuracy", "oa_trace+display",
                                        "null2_expect", "other" };
struct ProfScope {
  int id; std::chrono::steady_clock::time_point t0;
  explicit ProfScope(int i) : id(i) { if (g_prof_on) t0 = std::chrono::steady_clock::now(); }
  ~ProfScope() { if (g_prof_on) g_prof_ns[id] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
};
void host_prof_dump()
{
  if (!g_prof_on) return;
  for (int i = 0; i < 12; ++i) { std::fprintf(stderr, "[p7x host prof] %-18s %9.3f ms\n", g_prof_name[i], g_prof_ns[i].load() / 1e6); g_prof_ns[i] = 0; }
}

namespace {

// hot loops are compiled twice (AVX2 and baseline x86-64) and dispatched at load time
#if defined(__HIP_DEVICE_COMPILE__)
#define P7X_MULTIVERSION
#else
#define P7X_MULTIVERSION __attribute__((target_clones("avx2", "default")))
#endif

// ---------------------------------------------------------------- Easel "fast" RNG (esl_randomness_CreateFast)
struct FastRng {
  uint32_t seed = 42, x = 0;
  static uint32_t mix3(uint32_t a, uint32_t b, uint32_t c)
  {
    a -= b; a -= c; a ^= (c >> 13);  b -= c; b -= a; b ^= (a << 8);   c -= a; c -= b; c ^= (b >> 13);
    a -= b; a -= c; a ^= (c >> 12);  b -= c; b -= a; b ^= (a << 16);  c -= a; c -= b; c ^= (b >> 5);
    a -= b; a -= c; a ^= (c >> 3);   b -= c; b -= a; b ^= (a << 10);  c -= a; c -= b; c ^= (b >> 15);
    return c;
  }
  // esl_randomness_Init for the LCG type: the seed is dispersed with Jenkins' mix3, never zero
  void init(uint32_t s) { seed = s; x = mix3(s, 87654321u, 12345678u); if (x == 0) x = 42; }
  uint32_t next_u32() { x = lcg_next(x); return x; }
  double next() { return (double) next_u32() / 4294967296.0; }
};

// esl_vec_FSum (Kahan).  Same arithmetic as kahan_fsum(); this translation unit is compiled without fast-math and
// without contraction, so the compensation survives without the volatile round trips through memory.
static inline float fsum(const float *v, int n)
{
  float sum = 0.0f, c = 0.0f;
  for (int i = 0; i < n; ++i) { const float y = v[i] - c; const float t = sum + y; c = (t - sum) - y; sum = t; }
  return sum;
}
void fnorm(float *v, int n)
{
  const float s = fsum(v, n);
  if (s != 0.0f) for (int i = 0; i < n; ++i) v[i] /= s;
  else           for (int i = 0; i < n; ++i) v[i] = 1. / (float) n;
}
// ---------------------------------------------------------------- the wavefront's combining trees, lane by lane
// Host restatement of p7x_wave.hpp (affine_scan_up / affine_scan_down / wave_sum_f32): the same operations on the same
// operands in the same order, so that a sum formed here and on the device is the same float.  A DPP step whose source
// lane lies outside the 16-lane row (or whose row is masked) leaves the identity (a = 0, p = 1) in place of the operand.
static inline void lanes_scan_up(float *sa, float *sp)
{ // inclusive scan of the affine maps x -> a_l + p_l x over lanes 0..l: Kogge-Stone inside the rows, then row_bcast:15 / :31
  float a[64], q[64];
  for (int s = 1; s <= 8; s <<= 1) {
    for (int l = 0; l < 64; ++l) {
      const bool src = (l & 15) >= s;
      const float pa = src ? sa[l - s] : 0.0f, pp = src ? sp[l - s] : 1.0f;
      a[l] = sa[l] + pa * sp[l]; q[l] = sp[l] * pp;
    }
    for (int l = 0; l < 64; ++l) { sa[l] = a[l]; sp[l] = q[l]; }
  }
  for (int row = 1; row < 4; row += 2) {            // rows 1 and 3 take the last lane of the row before them
    const float pa = sa[16 * row - 1], pp = sp[16 * row - 1];
    for (int l = 16 * row; l < 16 * row + 16; ++l) { sa[l] = sa[l] + pa * sp[l]; sp[l] = sp[l] * pp; }
  }
  {                                                 // rows 2 and 3 take lane 31
    const float pa = sa[31], pp = sp[31];
    for (int l = 32; l < 64; ++l) { sa[l] = sa[l] + pa * sp[l]; sp[l] = sp[l] * pp; }
  }
}
static inline void lanes_scan_down(float *sa, float *sp)
{ // the same over lanes l..63
  float a[64], q[64];
  for (int s = 1; s <= 8; s <<= 1) {
    for (int l = 0; l < 64; ++l) {
      const bool src = (l & 15) + s <= 15;
      const float pa = src ? sa[l + s] : 0.0f, pp = src ? sp[l + s] : 1.0f;
      a[l] = sa[l] + pa * sp[l]; q[l] = sp[l] * pp;
    }
    for (int l = 0; l < 64; ++l) { sa[l] = a[l]; sp[l] = q[l]; }
  }
  {
    const float a48 = sa[48], p48 = sp[48], a16 = sa[16], p16 = sp[16];
    for (int l = 0; l < 64; ++l) {
      const int row = l >> 4;
      const float pa = (row == 2) ? a48 : ((row == 0) ? a16 : 0.0f), pp = (row == 2) ? p48 : ((row == 0) ? p16 : 1.0f);
      sa[l] = sa[l] + pa * sp[l]; sp[l] = sp[l] * pp;
    }
  }
  {
    const float a32 = sa[32], p32 = sp[32];
    for (int l = 0; l < 64; ++l) {
      const float pa = (l < 32) ? a32 : 0.0f, pp = (l < 32) ? p32 : 1.0f;
      sa[l] = sa[l] + pa * sp[l]; sp[l] = sp[l] * pp;
    }
  }
}
static inline float lanes_sum(float *v)
{ // wave_sum_f32: the value lane 63 ends up with
  float t[64];
  for (int s = 1; s <= 8; s <<= 1) {
    for (int l = 0; l < 64; ++l) t[l] = v[l] + (((l & 15) >= s) ? v[l - s] : 0.0f);
    for (int l = 0; l < 64; ++l) v[l] = t[l];
  }
  for (int row = 1; row < 4; row += 2) { const float b = v[16 * row - 1]; for (int l = 16 * row; l < 16 * row + 16; ++l) v[l] = v[l] + b; }
  { const float b = v[31]; for (int l = 32; l < 64; ++l) v[l] = v[l] + b; }
  return v[63];
}

// ---------------------------------------------------------------- p7_Forward / p7_Backward
// One body per direction and summation order.  Each is written once for both answers to "where does row r live":
//   FULL   every DP row stays in the Matrix (row r at r): p7_Forward / p7_Backward, for decoding and the tracebacks;
//   !FULL  only the special-state rows, the scale factors and the score come out: p7_ForwardParser / p7_BackwardParser.
//          The lanes bodies then roll over two Matrix rows (row r at r & 1); the upstream bodies compute on their striped
//          rows anyway and simply do not copy them out.
// The bodies are inlined into plain cloned entry points below (target_clones does not go on templates).
#define P7X_INLINE static inline __attribute__((always_inline))
template <bool FULL> static inline int row_at(int r) { return FULL ? r : (r & 1); }

// dsq is 1-indexed over the envelope: residues dsq[1..L].
// D(i,k) = M(i,k-1) tMD(k-1) + D(i,k-1) tDD(k-1), k = 1..M, given the finished M row; returns xE = sum_k M(i,k) + D(i,k).
// ForwardRow<C, U>::row (p7x_waverows.hpp) operation for operation: every lane runs its own chain from a zero carry, the
// lanes' affine maps are composed by the scan, the carry enters a lane's nodes through successive products, and the row
// sum takes a lane's match cells, then its delete cells, then the reduction tree.
static float dchain_forward(const Model &om, const float *__restrict mc, float *__restrict dc)
{
  const int M = om.M, C = om.C;
  const float *__restrict tMD = om.tf(4), *__restrict tDD = om.tf(7);
  float sa[64], sp[64], es[64];
  for (int z = 0; z < 64; ++z) {
    const int k0 = z * C + 1;
    float A = 0.0f, e = 0.0f;
    const int k1 = std::min(M, k0 + C - 1);
    for (int k = k0; k <= k1; ++k) { e = e + mc[k]; dc[k] = A; A = mc[k] * tMD[k] + A * tDD[k]; }
    if (k0 + C - 1 > M) A = 0.0f;                   // a padding node closes the chain (its transitions are zero)
    sa[z] = A; sp[z] = om.ddprod[z]; es[z] = e;
  }
  lanes_scan_up(sa, sp);
  for (int z = 0; z < 64; ++z) {
    const int k0 = z * C + 1, k1 = std::min(M, k0 + C - 1);
    float w = z ? sa[z - 1] : 0.0f, e = es[z];
    for (int k = k0; k <= k1; ++k) { dc[k] = dc[k] + w; e = e + dc[k]; w = w * tDD[k]; }
    es[z] = e;
  }
  return lanes_sum(es);
}

template <bool FULL>
P7X_INLINE int forward_lanes(const Model &om, const uint8_t *dsq, int L, Matrix &ox, float *ret_sc)
{
  const int M = om.M;
  ox.resize(M, L, FULL ? -1 : 2);
  const float *__restrict bm = om.tf(0), *__restrict tMM = om.tf(1), *__restrict tIM = om.tf(2), *__restrict tDM = om.tf(3),
              *__restrict tMI = om.tf(5), *__restrict tII = om.tf(6);
  float *m0 = ox.M_(0), *i0 = ox.I_(0), *d0 = ox.D_(0);
  for (int k = 0; k <= M + 1; ++k) m0[k] = i0[k] = d0[k] = 0.0f;
  float xE = 0.f, xN = 1.f, xJ = 0.f, xB = om.xf[XN][MOVE], xC = 0.f;
  ox.X(0, xE_) = xE; ox.X(0, xN_) = xN; ox.X(0, xJ_) = xJ; ox.X(0, xB_) = xB; ox.X(0, xC_) = xC; ox.X(0, xS_) = 1.0f;
  ox.totscale = 0.0f; ox.own_scales = true;
  for (int r = 1; r <= L; ++r) {
    const float *__restrict rf = om.rf(dsq[r]);
    const int rp = row_at<FULL>(r - 1), rc = row_at<FULL>(r);
    const float *__restrict mp = ox.M_(rp), *__restrict ip = ox.I_(rp), *__restrict dp = ox.D_(rp);
    float *__restrict mc = ox.M_(rc), *__restrict ic = ox.I_(rc), *__restrict dc = ox.D_(rc);
    mc[0] = ic[0] = dc[0] = 0.0f;
    for (int k = 1; k <= M; ++k) {
      float sv = xB * bm[k];
      sv = sv + mp[k - 1] * tMM[k];
      sv = sv + ip[k - 1] * tIM[k];
      sv = sv + dp[k - 1] * tDM[k];
      mc[k] = sv * rf[k];
      ic[k] = mp[k] * tMI[k] + ip[k] * tII[k];
    }
    xE = dchain_forward(om, mc, dc);
    mc[M + 1] = ic[M + 1] = dc[M + 1] = 0.0f;
    xN = xN * om.xf[XN][LOOP];
    xC = (xC * om.xf[XC][LOOP]) + (xE * om.xf[XE][MOVE]);
    xJ = (xJ * om.xf[XJ][LOOP]) + (xE * om.xf[XE][LOOP]);
    xB = (xJ * om.xf[XJ][MOVE]) + (xN * om.xf[XN][MOVE]);
    if (xE > 1.0e4) {
      xN = xN / xE; xC = xC / xE; xJ = xJ / xE; xB = xB / xE;
      const float inv = 1.0 / xE;
      for (int q = 1; q <= M; ++q) { mc[q] *= inv; dc[q] *= inv; ic[q] *= inv; }
      ox.X(r, xS_) = xE;
      ox.totscale += std::log((double) xE);
      xE = 1.0;
    } else ox.X(r, xS_) = 1.0f;
    ox.X(r, xE_) = xE; ox.X(r, xN_) = xN; ox.X(r, xJ_) = xJ; ox.X(r, xB_) = xB; ox.X(r, xC_) = xC;
  }
  if (std::isnan(xC) || (L > 0 && xC == 0.0f) || std::isinf(xC)) { if (ret_sc) *ret_sc = INFINITY; return P7X_ERANGE; }
  if (ret_sc) *ret_sc = ox.totscale + std::log((double) (xC * om.xf[XC][MOVE]));
  return P7X_OK;
}

// D(i,k) = base(k) + D(i,k+1) tDD(k), k = M..1 (D(i,M+1) = 0); on entry dc[k] = base(k).  The envelope kernel's d_chain:
// every lane folds its nodes from the last to the first, the scan composes the lanes from 63 downwards, and each lane
// then recomputes its chain from the carry it was handed.
static void dchain_backward(const Model &om, float *__restrict dc)
{
  const int M = om.M, C = om.C;
  const float *__restrict tDD = om.tf(7);
  float sa[64], sp[64];
  for (int z = 0; z < 64; ++z) {
    const int k0 = z * C + 1, k1 = std::min(M, k0 + C - 1);
    float A = 0.0f;
    for (int k = k1; k >= k0; --k) A = dc[k] + A * tDD[k];
    sa[z] = A; sp[z] = om.ddprod[z];
  }
  lanes_scan_down(sa, sp);
  for (int z = 0; z < 64; ++z) {
    const int k0 = z * C + 1, k1 = std::min(M, k0 + C - 1);
    float w = (z < 63) ? sa[z + 1] : 0.0f;
    for (int k = k1; k >= k0; --k) { dc[k] = dc[k] + w * tDD[k]; w = dc[k]; }
  }
}
// sum_k v(k) w(k) as the kernels form it: a lane's nodes in order, then the reduction tree
static float lanes_dot(const Model &om, const float *__restrict v, const float *__restrict w)
{
  const int M = om.M, C = om.C;
  float es[64];
  for (int z = 0; z < 64; ++z) {
    const int k0 = z * C + 1, k1 = std::min(M, k0 + C - 1);
    float e = 0.0f;
    for (int k = k0; k <= k1; ++k) e = e + v[k] * w[k];
    es[z] = e;
  }
  return lanes_sum(es);
}

// fx: Forward's special rows (its scale factors are Backward's until a row sum outgrows them: own_scales)
template <bool FULL>
P7X_INLINE int backward_lanes(const Model &om, const uint8_t *dsq, int L, const float *fx, Matrix &bck, float *ret_sc)
{
  const int M = om.M;
  bck.resize(M, L, FULL ? -1 : 2);
  const float *__restrict bm = om.tf(0), *__restrict tMM = om.tf(1), *__restrict tIM = om.tf(2), *__restrict tDM = om.tf(3),
              *__restrict tMD = om.tf(4), *__restrict tMI = om.tf(5), *__restrict tII = om.tf(6);
  bck.own_scales = false;
  float xJ = 0.f, xB = 0.f, xN = 0.f;
  float xC = om.xf[XC][MOVE];
  float xE = xC * om.xf[XE][MOVE];
  float *__restrict me = bck.scratch.data();          // [M+3] work row (no allocation inside the multiversioned body)
  for (int k = 0; k <= M + 2; ++k) me[k] = 0.0f;
  {
    const int rc = row_at<FULL>(L);
    float *__restrict mc = bck.M_(rc), *__restrict ic = bck.I_(rc), *__restrict dc = bck.D_(rc);
    mc[M + 1] = ic[M + 1] = dc[M + 1] = 0.0f;
    for (int k = 1; k <= M; ++k) { dc[k] = xE; ic[k] = 0.0f; }
    dchain_backward(om, dc);
    for (int k = 1; k <= M; ++k) mc[k] = xE + dc[k + 1] * tMD[k];
    mc[0] = ic[0] = dc[0] = 0.0f;
    float sc = fx[(size_t) L * NX + xS_];
    if (sc > 1.0f) {
      xE = xE / sc; xN = xN / sc; xC = xC / sc; xJ = xJ / sc; xB = xB / sc;
      const float inv = 1.0 / sc;
      for (int k = 1; k <= M; ++k) { mc[k] *= inv; dc[k] *= inv; ic[k] *= inv; }
    }
    bck.X(L, xS_) = sc;
    bck.totscale = std::log((double) sc);
    bck.X(L, xE_) = xE; bck.X(L, xN_) = xN; bck.X(L, xJ_) = xJ; bck.X(L, xB_) = xB; bck.X(L, xC_) = xC;
  }
  for (int r = L - 1; r >= 1; --r) {
    const float *__restrict rf = om.rf(dsq[r + 1]);
    const int rn = row_at<FULL>(r + 1), rc = row_at<FULL>(r);
    const float *__restrict mn = bck.M_(rn), *__restrict in = bck.I_(rn);
    float *__restrict mc = bck.M_(rc), *__restrict ic = bck.I_(rc), *__restrict dc = bck.D_(rc);
    for (int k = 1; k <= M; ++k) me[k] = mn[k] * rf[k];                      // M(i+1,k) e(x_{i+1},k)
    me[M + 1] = 0.0f;
    xB = lanes_dot(om, me, bm);
    xC = xC * om.xf[XC][LOOP];
    xJ = (xB * om.xf[XJ][MOVE]) + (xJ * om.xf[XJ][LOOP]);
    xN = (xB * om.xf[XN][MOVE]) + (xN * om.xf[XN][LOOP]);
    xE = (xC * om.xf[XE][MOVE]) + (xJ * om.xf[XE][LOOP]);
    mc[M + 1] = ic[M + 1] = dc[M + 1] = 0.0f;
    // entering-transitions of node k+1 are stored at index k+1; node M+1 does not exist (me[M+1] = 0)
    for (int k = 1; k < M; ++k) {
      const float mek = me[k + 1];
      ic[k] = in[k] * tII[k] + mek * tIM[k + 1];
      dc[k] = mek * tDM[k + 1] + xE;
      mc[k] = (in[k] * tMI[k] + mek * tMM[k + 1]) + xE;
    }
    ic[M] = in[M] * tII[M]; dc[M] = xE; mc[M] = in[M] * tMI[M] + xE;
    dchain_backward(om, dc);
    for (int k = 1; k <= M; ++k) mc[k] += dc[k + 1] * tMD[k];
    mc[0] = ic[0] = dc[0] = 0.0f;
    if (xB > 1.0e16) bck.own_scales = true;
    float sc = bck.own_scales ? ((xB > 1.0e4) ? xB : 1.0f) : fx[(size_t) r * NX + xS_];
    bck.X(r, xS_) = sc;
    if (sc > 1.0f) {
      xE /= sc; xN /= sc; xJ /= sc; xB /= sc; xC /= sc;
      const float inv = 1.0 / sc;
      for (int k = 1; k <= M; ++k) { mc[k] *= inv; dc[k] *= inv; ic[k] *= inv; }
      bck.totscale += std::log((double) sc);
    }
    bck.X(r, xE_) = xE; bck.X(r, xN_) = xN; bck.X(r, xJ_) = xJ; bck.X(r, xB_) = xB; bck.X(r, xC_) = xC;
  }
  {
    const float *__restrict rf = om.rf(dsq[1]);
    const float *__restrict mn = bck.M_(row_at<FULL>(1));
    for (int k = 1; k <= M; ++k) me[k] = mn[k] * rf[k];
    xB = lanes_dot(om, me, bm);
    xN = (xB * om.xf[XN][MOVE]) + (xN * om.xf[XN][LOOP]);
    bck.X(0, xB_) = xB; bck.X(0, xC_) = 0.0f; bck.X(0, xJ_) = 0.0f; bck.X(0, xN_) = xN; bck.X(0, xE_) = 0.0f; bck.X(0, xS_) = 1.0f;
    if (FULL) { float *mc = bck.M_(0), *ic = bck.I_(0), *dc = bck.D_(0); for (int k = 0; k <= M + 1; ++k) mc[k] = ic[k] = dc[k] = 0.0f; }
  }
  if (std::isnan(xN) || (L > 0 && xN == 0.0f) || std::isinf(xN)) { if (ret_sc) *ret_sc = INFINITY; return P7X_ERANGE; }
  if (ret_sc) *ret_sc = bck.totscale + std::log((double) xN);
  return P7X_OK;
}

// ---------------------------------------------------------------- ... in upstream's order
// impl_sse/fwdback.c forward_engine / backward_engine restated on four-float vectors: vector q of a row holds nodes q+1,
// q+1+Q, q+1+2Q, q+1+3Q (padding nodes carry zero transitions and emissions, as p7_oprofile_Convert pads them).  Every
// multiplication and addition of the vector code is performed on the same operands in the same order: node k lives in
// stripe z = (k-1) / Q of vector q = (k-1) % Q; xE is four per-stripe sums over q (match cells first, delete cells after
// the delete chain) folded as (s0 + s1) + (s2 + s3); the D->D chain is one serial sweep per stripe and then up to three
// carry sweeps from stripe to stripe (always three when M < 100, else until no cell grows).  FULL is upstream's do_full:
// the rows go to the un-striped Matrix afterwards.
typedef float V4 __attribute__((vector_size(16), aligned(4)));      // four stripes side by side (the compiler's own vector type: one SIMD operation per vector operation)
static inline V4 v4_set(float a) { return V4{ a, a, a, a }; }
static inline V4 v4_add(const V4 &a, const V4 &b) { return a + b; }
static inline V4 v4_mul(const V4 &a, const V4 &b) { return a * b; }
static inline V4 v4_shr(const V4 &a) { const V4 z = { 0.0f, 0.0f, 0.0f, 0.0f }; return __builtin_shufflevector(a, z, 4, 0, 1, 2); }   // esl_sse_rightshift_ps(a, 0)
static inline V4 v4_shl(const V4 &a) { const V4 z = { 0.0f, 0.0f, 0.0f, 0.0f }; return __builtin_shufflevector(a, z, 1, 2, 3, 4); }   // esl_sse_leftshift_ps(a, 0)
static inline float v4_hsum(const V4 &a) { return (a[0] + a[1]) + (a[2] + a[3]); }            // esl_sse_hsum_ps
struct StripedRow { std::vector<V4> m, d, i; void resize(int Q) { m.resize((size_t) Q); d.resize((size_t) Q); i.resize((size_t) Q); } };
static inline void unstripe(const StripedRow &r, int Q, int M, float *mc, float *ic, float *dc)
{
  for (int q = 0; q < Q; ++q)
    for (int z = 0; z < 4; ++z) { const int k = q + 1 + z * Q; if (k <= M) { mc[k] = r.m[q][z]; ic[k] = r.i[q][z]; dc[k] = r.d[q][z]; } }
  mc[0] = ic[0] = dc[0] = 0.0f; mc[M + 1] = ic[M + 1] = dc[M + 1] = 0.0f;
}

struct StripedScratch { StripedRow a, b; };     // per thread, owned by the callers of the entry points (no thread_local inside a cloned function)
template <bool FULL>
P7X_INLINE int forward_upstream(const Model &om, const uint8_t *dsq, int L, Matrix &ox, float *ret_sc, StripedScratch &ss)
{
  const int M = om.M, Q = om.Q;
  ox.resize(M, L, FULL ? -1 : 0);
  const V4 *tBM = reinterpret_cast<const V4 *>(om.sT(0)), *tMM = reinterpret_cast<const V4 *>(om.sT(1)), *tIM = reinterpret_cast<const V4 *>(om.sT(2)),
           *tDM = reinterpret_cast<const V4 *>(om.sT(3)), *tMD = reinterpret_cast<const V4 *>(om.sT(4)), *tMI = reinterpret_cast<const V4 *>(om.sT(5)),
           *tII = reinterpret_cast<const V4 *>(om.sT(6)), *tDD = reinterpret_cast<const V4 *>(om.sT(7));
  StripedRow &row = ss.a;
  row.resize(Q);
  const V4 zero = v4_set(0.0f);
  for (int q = 0; q < Q; ++q) row.m[q] = row.d[q] = row.i[q] = zero;
  if (FULL) { float *m0 = ox.M_(0), *i0 = ox.I_(0), *d0 = ox.D_(0); for (int k = 0; k <= M + 1; ++k) m0[k] = i0[k] = d0[k] = 0.0f; }
  float xE = 0.f, xN = 1.f, xJ = 0.f, xB = om.xf[XN][MOVE], xC = 0.f;
  ox.X(0, xE_) = xE; ox.X(0, xN_) = xN; ox.X(0, xJ_) = xJ; ox.X(0, xB_) = xB; ox.X(0, xC_) = xC; ox.X(0, xS_) = 1.0f;
  ox.totscale = 0.0f; ox.own_scales = true;
  for (int r = 1; r <= L; ++r) {
    const V4 *rv = reinterpret_cast<const V4 *>(om.sR(dsq[r]));
    V4 dcv = zero, xEv = zero;
    const V4 xBv = v4_set(xB);
    V4 mpv = v4_shr(row.m[Q - 1]), dpv = v4_shr(row.d[Q - 1]), ipv = v4_shr(row.i[Q - 1]);
    for (int q = 0; q < Q; ++q) {
      V4 sv = v4_mul(xBv, tBM[q]);
      sv = v4_add(sv, v4_mul(mpv, tMM[q]));
      sv = v4_add(sv, v4_mul(ipv, tIM[q]));
      sv = v4_add(sv, v4_mul(dpv, tDM[q]));
      sv = v4_mul(sv, rv[(size_t) q]);
      xEv = v4_add(xEv, sv);
      mpv = row.m[q]; dpv = row.d[q]; ipv = row.i[q];
      row.m[q] = sv;
      row.d[q] = dcv;
      dcv = v4_mul(sv, tMD[q]);
      sv = v4_mul(mpv, tMI[q]);
      row.i[q] = v4_add(sv, v4_mul(ipv, tII[q]));
    }
    dcv = v4_shr(dcv);
    row.d[0] = zero;
    for (int q = 0; q < Q; ++q) { row.d[q] = v4_add(dcv, row.d[q]); dcv = v4_mul(row.d[q], tDD[q]); }
    if (M < 100) {
      for (int j = 1; j < 4; ++j) {
        dcv = v4_shr(dcv);
        for (int q = 0; q < Q; ++q) { row.d[q] = v4_add(dcv, row.d[q]); dcv = v4_mul(dcv, tDD[q]); }
      }
    } else {
      for (int j = 1; j < 4; ++j) {
        bool grew = false;
        dcv = v4_shr(dcv);
        for (int q = 0; q < Q; ++q) {
          const V4 sv = v4_add(dcv, row.d[q]);
          for (int z = 0; z < 4; ++z) grew |= sv[z] > row.d[q][z];
          row.d[q] = sv;
          dcv = v4_mul(dcv, tDD[q]);
        }
        if (!grew) break;
      }
    }
    for (int q = 0; q < Q; ++q) xEv = v4_add(row.d[q], xEv);
    xE = v4_hsum(xEv);
    xN = xN * om.xf[XN][LOOP];
    xC = (xC * om.xf[XC][LOOP]) + (xE * om.xf[XE][MOVE]);
    xJ = (xJ * om.xf[XJ][LOOP]) + (xE * om.xf[XE][LOOP]);
    xB = (xJ * om.xf[XJ][MOVE]) + (xN * om.xf[XN][MOVE]);
    if (xE > 1.0e4) {
      xN = xN / xE; xC = xC / xE; xJ = xJ / xE; xB = xB / xE;
      const V4 inv = v4_set((float) (1.0 / xE));
      for (int q = 0; q < Q; ++q) { row.m[q] = v4_mul(row.m[q], inv); row.d[q] = v4_mul(row.d[q], inv); row.i[q] = v4_mul(row.i[q], inv); }
      ox.X(r, xS_) = xE;
      ox.totscale += std::log((double) xE);
      xE = 1.0;
    } else ox.X(r, xS_) = 1.0f;
    ox.X(r, xE_) = xE; ox.X(r, xN_) = xN; ox.X(r, xJ_) = xJ; ox.X(r, xB_) = xB; ox.X(r, xC_) = xC;
    if (FULL) unstripe(row, Q, M, ox.M_(r), ox.I_(r), ox.D_(r));
  }
  if (std::isnan(xC) || (L > 0 && xC == 0.0f) || std::isinf(xC)) { if (ret_sc) *ret_sc = INFINITY; return P7X_ERANGE; }
  if (ret_sc) *ret_sc = ox.totscale + std::log((double) (xC * om.xf[XC][MOVE]));
  return P7X_OK;
}

template <bool FULL>
P7X_INLINE int backward_upstream(const Model &om, const uint8_t *dsq, int L, const float *fx, Matrix &bck, float *ret_sc, StripedScratch &ss)
{
  const int M = om.M, Q = om.Q;
  bck.resize(M, L, FULL ? -1 : 0);
  const V4 *tBM = reinterpret_cast<const V4 *>(om.sT(0)), *tMM = reinterpret_cast<const V4 *>(om.sT(1)), *tIM = reinterpret_cast<const V4 *>(om.sT(2)),
           *tDM = reinterpret_cast<const V4 *>(om.sT(3)), *tMD = reinterpret_cast<const V4 *>(om.sT(4)), *tMI = reinterpret_cast<const V4 *>(om.sT(5)),
           *tII = reinterpret_cast<const V4 *>(om.sT(6)), *tDD = reinterpret_cast<const V4 *>(om.sT(7));
  StripedRow &rowa = ss.a, &rowb = ss.b;
  rowa.resize(Q); rowb.resize(Q);
  StripedRow *cur = &rowa, *nxt = &rowb;          // row i being built, row i + 1
  const V4 zero = v4_set(0.0f);
  bck.own_scales = false;
  float xJ = 0.f, xB = 0.f, xN = 0.f;
  float xC = om.xf[XC][MOVE];
  float xE = xC * om.xf[XE][MOVE];
  // the D -> D paths of a row: one sweep down every stripe from what the stripe after it holds so far, then three sweeps that
  // hand the remainder from stripe to stripe; then the M -> D paths.  first: the operand the first sweep starts from.
  auto close_row = [&](StripedRow &r, const V4 &first, const V4 &xEv, bool add_e) {
    V4 dpv = v4_shl(first), dcv = zero;
    for (int q = Q - 1; q >= 0; --q) {
      dcv = v4_mul(dpv, tDD[q]);
      if (add_e) { r.d[q] = v4_add(r.d[q], v4_add(dcv, xEv)); r.m[q] = v4_add(r.m[q], xEv); }
      else       r.d[q] = v4_add(r.d[q], dcv);
      dpv = r.d[q];
    }
    for (int j = 1; j < 4; ++j) {
      dcv = v4_shl(dcv);
      for (int q = Q - 1; q >= 0; --q) { dcv = v4_mul(dcv, tDD[q]); r.d[q] = v4_add(r.d[q], dcv); }
    }
    dcv = v4_shl(r.d[0]);
    for (int q = Q - 1; q >= 0; --q) { r.m[q] = v4_add(r.m[q], v4_mul(dcv, tMD[q])); dcv = r.d[q]; }
  };
  auto rescale = [&](StripedRow &r, float sc) {
    const V4 inv = v4_set((float) (1.0 / sc));
    for (int q = 0; q < Q; ++q) { r.m[q] = v4_mul(r.m[q], inv); r.d[q] = v4_mul(r.d[q], inv); r.i[q] = v4_mul(r.i[q], inv); }
  };
  {
    const V4 xEv = v4_set(xE);
    for (int q = 0; q < Q; ++q) { cur->m[q] = cur->d[q] = xEv; cur->i[q] = zero; }
    close_row(*cur, cur->d[Q - 1], xEv, false);
    const float sc = fx[(size_t) L * NX + xS_];
    if (sc > 1.0f) { xE = xE / sc; xN = xN / sc; xC = xC / sc; xJ = xJ / sc; xB = xB / sc; rescale(*cur, sc); }
    bck.X(L, xS_) = sc;
    bck.totscale = std::log((double) sc);
    bck.X(L, xE_) = xE; bck.X(L, xN_) = xN; bck.X(L, xJ_) = xJ; bck.X(L, xB_) = xB; bck.X(L, xC_) = xC;
    if (FULL) unstripe(*cur, Q, M, bck.M_(L), bck.I_(L), bck.D_(L));
  }
  for (int r = L - 1; r >= 1; --r) {
    std::swap(cur, nxt);
    const V4 *rv = reinterpret_cast<const V4 *>(om.sR(dsq[r + 1]));
    V4 tmmv = v4_shl(tMM[0]), timv = v4_shl(tIM[0]), tdmv = v4_shl(tDM[0]);      // the transitions INTO the node after the stripe's last
    V4 mpv = v4_shl(v4_mul(nxt->m[0], rv[0]));                                   // M(i+1, k+1) e(x_{i+1}, k+1)
    V4 xBv = zero;
    for (int q = Q - 1; q >= 0; --q) {
      const V4 ipv = nxt->i[q];
      cur->i[q] = v4_add(v4_mul(ipv, tII[q]), v4_mul(mpv, timv));
      cur->d[q] = v4_mul(mpv, tdmv);
      const V4 mcv = v4_add(v4_mul(ipv, tMI[q]), v4_mul(mpv, tmmv));
      mpv = v4_mul(nxt->m[q], rv[(size_t) q]);
      cur->m[q] = mcv;
      tdmv = tDM[q]; timv = tIM[q]; tmmv = tMM[q];
      xBv = v4_add(xBv, v4_mul(mpv, tBM[q]));
    }
    xB = v4_hsum(xBv);
    xC = xC * om.xf[XC][LOOP];
    xJ = (xB * om.xf[XJ][MOVE]) + (xJ * om.xf[XJ][LOOP]);
    xN = (xB * om.xf[XN][MOVE]) + (xN * om.xf[XN][LOOP]);
    xE = (xC * om.xf[XE][MOVE]) + (xJ * om.xf[XE][LOOP]);
    const V4 xEv = v4_set(xE);
    close_row(*cur, v4_add(cur->d[0], xEv), xEv, true);
    if (xB > 1.0e16) bck.own_scales = true;
    const float sc = bck.own_scales ? ((xB > 1.0e4) ? xB : 1.0f) : fx[(size_t) r * NX + xS_];
    bck.X(r, xS_) = sc;
    if (sc > 1.0f) {
      xE /= sc; xN /= sc; xJ /= sc; xB /= sc; xC /= sc;
      rescale(*cur, sc);
      bck.totscale += std::log((double) sc);
    }
    bck.X(r, xE_) = xE; bck.X(r, xN_) = xN; bck.X(r, xJ_) = xJ; bck.X(r, xB_) = xB; bck.X(r, xC_) = xC;
    if (FULL) unstripe(*cur, Q, M, bck.M_(r), bck.I_(r), bck.D_(r));
  }
  {
    const V4 *rv = reinterpret_cast<const V4 *>(om.sR(dsq[1]));
    V4 xBv = zero;
    for (int q = Q - 1; q >= 0; --q) xBv = v4_add(xBv, v4_mul(v4_mul(cur->m[q], rv[(size_t) q]), tBM[q]));
    xB = v4_hsum(xBv);
    xN = (xB * om.xf[XN][MOVE]) + (xN * om.xf[XN][LOOP]);
    bck.X(0, xB_) = xB; bck.X(0, xC_) = 0.0f; bck.X(0, xJ_) = 0.0f; bck.X(0, xN_) = xN; bck.X(0, xE_) = 0.0f; bck.X(0, xS_) = 1.0f;
    if (FULL) { float *mc = bck.M_(0), *ic = bck.I_(0), *dc = bck.D_(0); for (int k = 0; k <= M + 1; ++k) mc[k] = ic[k] = dc[k] = 0.0f; }
  }
  if (std::isnan(xN) || (L > 0 && xN == 0.0f) || std::isinf(xN)) { if (ret_sc) *ret_sc = INFINITY; return P7X_ERANGE; }
  if (ret_sc) *ret_sc = bck.totscale + std::log((double) xN);
  return P7X_OK;
}

// the cloned entry points: (direction, order) x (full matrix, rows only)
P7X_MULTIVERSION int forward_full_lanes(const Model &om, const uint8_t *dsq, int L, Matrix &ox, float *sc) { return forward_lanes<true>(om, dsq, L, ox, sc); }
P7X_MULTIVERSION int forward_rows_lanes(const Model &om, const uint8_t *dsq, int L, Matrix &ox, float *sc) { return forward_lanes<false>(om, dsq, L, ox, sc); }
P7X_MULTIVERSION int backward_full_lanes(const Model &om, const uint8_t *dsq, int L, const float *fx, Matrix &bck, float *sc) { return backward_lanes<true>(om, dsq, L, fx, bck, sc); }
P7X_MULTIVERSION int backward_rows_lanes(const Model &om, const uint8_t *dsq, int L, const float *fx, Matrix &bck, float *sc) { return backward_lanes<false>(om, dsq, L, fx, bck, sc); }
P7X_MULTIVERSION int forward_full_upstream(const Model &om, const uint8_t *dsq, int L, Matrix &ox, float *sc, StripedScratch &ss) { return forward_upstream<true>(om, dsq, L, ox, sc, ss); }
P7X_MULTIVERSION int forward_rows_upstream(const Model &om, const uint8_t *dsq, int L, Matrix &ox, float *sc, StripedScratch &ss) { return forward_upstream<false>(om, dsq, L, ox, sc, ss); }
P7X_MULTIVERSION int backward_full_upstream(const Model &om, const uint8_t *dsq, int L, const float *fx, Matrix &bck, float *sc, StripedScratch &ss) { return backward_upstream<true>(om, dsq, L, fx, bck, sc, ss); }
P7X_MULTIVERSION int backward_rows_upstream(const Model &om, const uint8_t *dsq, int L, const float *fx, Matrix &bck, float *sc, StripedScratch &ss) { return backward_upstream<false>(om, dsq, L, fx, bck, sc, ss); }

static StripedScratch &striped_scratch() { thread_local StripedScratch *ss = new StripedScratch(); return *ss; }     // (leaked with its thread: a few KB)
static inline int forward_full(const Model &om, const uint8_t *dsq, int L, Matrix &ox, float *ret_sc)
{ return om.upstream ? forward_full_upstream(om, dsq, L, ox, ret_sc, striped_scratch()) : forward_full_lanes(om, dsq, L, ox, ret_sc); }
static inline int backward_full(const Model &om, const uint8_t *dsq, int L, const Matrix &fwd, Matrix &bck, float *ret_sc)
{ return om.upstream ? backward_full_upstream(om, dsq, L, fwd.x.data(), bck, ret_sc, striped_scratch()) : backward_full_lanes(om, dsq, L, fwd.x.data(), bck, ret_sc); }


// ---------------------------------------------------------------- p7_Decoding: posteriors into <bck> (in place)
// NOTE: only the M and I posteriors are formed.  bck.D_ keeps Backward's delete values afterwards (upstream zeroes them): a
// future reader of the delete "posteriors" must not take them from here.
P7X_MULTIVERSION int decoding(const Model &om, const Matrix &fwd, Matrix &bck)
{
  const int M = om.M, L = fwd.L;
  float scaleproduct = 1.0 / bck.X(0, xN_);
  // row 0 is zeroed *after* reading xN(0); upstream writes into a third matrix, we overwrite <bck> row by row,
  // which is safe because row i of the posterior only needs row i of both matrices and specials of row i-1 (fwd).
  float *bN = bck.scratch.data() + (M + 4), *bJ = bN + (L + 1), *bC = bJ + (L + 1), *bS = bC + (L + 1);
  for (int r = 0; r <= L; ++r) { bN[r] = bck.X(r, xN_); bJ[r] = bck.X(r, xJ_); bC[r] = bck.X(r, xC_); bS[r] = bck.X(r, xS_); }
  {
    float *mc = bck.M_(0), *ic = bck.I_(0), *dc = bck.D_(0);
    for (int k = 0; k <= M + 1; ++k) mc[k] = ic[k] = dc[k] = 0.0f;
    bck.X(0, xE_) = bck.X(0, xN_) = bck.X(0, xJ_) = bck.X(0, xC_) = bck.X(0, xB_) = 0.0f;
  }
  for (int r = 1; r <= L; ++r) {
    const float totr = scaleproduct * fwd.X(r, xS_);
    const float *__restrict fm = fwd.M_(r), *__restrict fi = fwd.I_(r);
    float *__restrict mc = bck.M_(r), *__restrict ic = bck.I_(r), *__restrict dc = bck.D_(r);
    (void) dc;                 // upstream zeroes the delete posteriors; nothing downstream reads them (optimal accuracy, null2 and the
                               // trace take M and I), so the row is left as Backward wrote it and a store stream is saved
    for (int k = 1; k <= M; ++k) {
      mc[k] = (fm[k] * mc[k]) * totr;
      ic[k] = (fi[k] * ic[k]) * totr;
    }
    bck.X(r, xE_) = 0.0f;
    bck.X(r, xN_) = fwd.X(r - 1, xN_) * bN[r] * om.xf[XN][LOOP] * scaleproduct;
    bck.X(r, xJ_) = fwd.X(r - 1, xJ_) * bJ[r] * om.xf[XJ][LOOP] * scaleproduct;
    bck.X(r, xB_) = 0.0f;
    bck.X(r, xC_) = fwd.X(r - 1, xC_) * bC[r] * om.xf[XC][LOOP] * scaleproduct;
    if (bck.own_scales) scaleproduct *= fwd.X(r, xS_) / bS[r];
  }
  return std::isinf(scaleproduct) ? P7X_ERANGE : P7X_OK;
}

// esl_abc_FAvgScVec + gap-like symbols
void finish_null2(const Profile &p, float *null2)
{
  const Alphabet &abc = Alphabet::get(p.abc_type);
  for (int x = p.K + 1; x <= p.Kp - 3; ++x) {
    float result = 0.0f; int n = 0;
    for (int y = 0; y < p.K; ++y) if (abc.degen[x][y]) { result += null2[y]; ++n; }
    null2[x] = result / (float) n;
  }
  null2[p.K] = 1.0f; null2[p.Kp - 2] = 1.0f; null2[p.Kp - 1] = 1.0f;
}

// ---------------------------------------------------------------- p7_Null2_ByExpectation (pp = posterior matrix)
P7X_MULTIVERSION void null2_by_expectation(const Model &om, Matrix &pp, float *null2)
{
  const int M = om.M, Ld = pp.L;
  float *m0 = pp.M_(0), *i0 = pp.I_(0);
  std::memcpy(m0, pp.M_(1), sizeof(float) * (M + 2));
  std::memcpy(i0, pp.I_(1), sizeof(float) * (M + 2));
  float eN = pp.X(1, xN_), eC = pp.X(1, xC_), eJ = pp.X(1, xJ_);
  for (int r = 2; r <= Ld; ++r) {
    const float *mr = pp.M_(r), *ir = pp.I_(r);
    for (int k = 1; k <= M; ++k) { m0[k] = mr[k] + m0[k]; i0[k] = ir[k] + i0[k]; }
    eN += pp.X(r, xN_); eC += pp.X(r, xC_); eJ += pp.X(r, xJ_);
  }
  const float norm = 1.0 / (float) Ld;
  for (int k = 1; k <= M; ++k) { m0[k] *= norm; i0[k] *= norm; }
  eN *= norm; eC *= norm; eJ *= norm;
  const float xfactor = eN + eC + eJ;
  const int C = om.C;
  if (om.upstream) {                                    // impl_sse/null2.c: four stripes, a stripe's nodes in order (match term, insert term), then hsum
    const int Q = om.Q;
    for (int x = 0; x < om.p->K; ++x) {
      const float *rf = om.rf(x);
      float sv[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
      for (int q = 0; q < Q; ++q)
        for (int z = 0; z < 4; ++z) { const int k = q + 1 + z * Q; if (k <= M) { sv[z] = sv[z] + m0[k] * rf[k]; sv[z] = sv[z] + i0[k]; } }
      null2[x] = ((sv[0] + sv[1]) + (sv[2] + sv[3])) + xfactor;
    }
    finish_null2(*om.p, null2);
    return;
  }
  for (int x = 0; x < om.p->K; ++x) {
    const float *rf = om.rf(x);
    float es[64];                                       // the envelope kernel's order: a lane's nodes, match then insert, then the tree
    for (int z = 0; z < 64; ++z) {
      const int k0 = z * C + 1, k1 = std::min(M, k0 + C - 1);
      float e = 0.0f;
      for (int k = k0; k <= k1; ++k) { e = e + m0[k] * rf[k]; e = e + i0[k]; }
      es[z] = e;
    }
    null2[x] = lanes_sum(es) + xfactor;
  }
  finish_null2(*om.p, null2);
}

// ---------------------------------------------------------------- p7_OptimalAccuracy + p7_OATrace
inline float gate(float t, float v) { return t > 0.0f ? v : 0.0f; }   // upstream: and(cmpgt(t,0), v)
inline float vmax(float a, float b) { return a > b ? a : b; }

P7X_MULTIVERSION void optimal_accuracy(const Model &om, const Matrix &pp, Matrix &ox, float *ret_e)
{
  const int M = om.M, L = pp.L;
  ox.resize(M, L);
  const float *bm = om.tf(0), *tMM = om.tf(1), *tIM = om.tf(2), *tDM = om.tf(3), *tMD = om.tf(4), *tMI = om.tf(5), *tII = om.tf(6), *tDD = om.tf(7);
  {
    float *mc = ox.M_(0), *ic = ox.I_(0), *dc = ox.D_(0);
    for (int k = 0; k <= M + 1; ++k) mc[k] = ic[k] = dc[k] = -INFINITY;
  }
  ox.X(0, xE_) = -INFINITY; ox.X(0, xN_) = 0.f; ox.X(0, xJ_) = -INFINITY; ox.X(0, xB_) = 0.f; ox.X(0, xC_) = -INFINITY;
  for (int r = 1; r <= L; ++r) {
    const float *__restrict mp = ox.M_(r - 1), *__restrict ip = ox.I_(r - 1), *__restrict dp = ox.D_(r - 1);
    const float *__restrict pm = pp.M_(r), *__restrict pi = pp.I_(r);
    float *__restrict mc = ox.M_(r), *__restrict ic = ox.I_(r), *__restrict dc = ox.D_(r);
    const float xB = ox.X(r - 1, xB_);
    mc[0] = ic[0] = dc[0] = -INFINITY;
    for (int k = 1; k <= M; ++k) {
      float sv = gate(bm[k], xB);
      sv = vmax(sv, gate(tMM[k], mp[k - 1]));
      sv = vmax(sv, gate(tIM[k], ip[k - 1]));
      sv = vmax(sv, gate(tDM[k], dp[k - 1]));
      mc[k] = sv + pm[k];
      float iv = gate(tMI[k], mp[k]);
      iv = vmax(iv, gate(tII[k], ip[k]));
      ic[k] = iv + pi[k];
    }
    // D(i,k) = max( gate(tMD(k-1), M(i,k-1)), gate(tDD(k-1), D(i,k-1)) ), D(i,1) = -inf.  Maxima are exact: any order of
    // evaluation (the device's gated max-scan included) gives these values.
    dc[1] = -INFINITY;
    for (int k = 2; k <= M; ++k) dc[k] = vmax(gate(tMD[k - 1], mc[k - 1]), (tDD[k - 1] > 0.0f) ? dc[k - 1] : 0.0f);
    float xEmax = -INFINITY;
    {
      float a8[8]; for (int z = 0; z < 8; ++z) a8[z] = -INFINITY;
      int k = 1;
      for (; k + 7 <= M; k += 8) for (int z = 0; z < 8; ++z) a8[z] = vmax(a8[z], vmax(mc[k + z], dc[k + z]));
      for (; k <= M; ++k) a8[0] = vmax(a8[0], vmax(mc[k], dc[k]));
      for (int z = 0; z < 8; ++z) xEmax = vmax(xEmax, a8[z]);
    }
    mc[M + 1] = ic[M + 1] = dc[M + 1] = -INFINITY;
    ox.X(r, xE_) = xEmax;
    float t1, t2;
    t1 = (om.xf[XJ][LOOP] == 0.0f) ? 0.0f : ox.X(r - 1, xJ_) + pp.X(r, xJ_);
    t2 = (om.xf[XE][LOOP] == 0.0f) ? 0.0f : ox.X(r, xE_);
    ox.X(r, xJ_) = std::fmax(t1, t2);
    t1 = (om.xf[XC][LOOP] == 0.0f) ? 0.0f : ox.X(r - 1, xC_) + pp.X(r, xC_);
    t2 = (om.xf[XE][MOVE] == 0.0f) ? 0.0f : ox.X(r, xE_);
    ox.X(r, xC_) = std::fmax(t1, t2);
    ox.X(r, xN_) = (om.xf[XN][LOOP] == 0.0f) ? 0.0f : ox.X(r - 1, xN_) + pp.X(r, xN_);
    t1 = (om.xf[XN][MOVE] == 0.0f) ? 0.0f : ox.X(r, xN_);
    t2 = (om.xf[XJ][MOVE] == 0.0f) ? 0.0f : ox.X(r, xJ_);
    ox.X(r, xB_) = std::fmax(t1, t2);
  }
  *ret_e = ox.X(L, xC_);
}

int oa_trace(const Model &om, const Matrix &pp, const Matrix &ox, Trace &tr)
{
  const int M = om.M, Q = om.p->Q4();
  const float *bm = om.tf(0), *tMM = om.tf(1), *tIM = om.tf(2), *tDM = om.tf(3), *tMD = om.tf(4), *tMI = om.tf(5), *tII = om.tf(6), *tDD = om.tf(7);
  int i = ox.L, k = 0;
  tr.clear();
  tr.append(sT, k, i, 0.0f);
  tr.append(sC, k, i, 0.0f);
  int s0 = sC;
  auto postprob = [&](int scur, int sprv, int kk, int ii) -> float {
    switch (scur) {
      case sM: return pp.M_(ii)[kk];
      case sI: return pp.I_(ii)[kk];
      case sN: if (sprv == scur) return pp.X(ii, xN_); return 0.0f;
      case sC: if (sprv == scur) return pp.X(ii, xC_); return 0.0f;
      case sJ: if (sprv == scur) return pp.X(ii, xJ_); return 0.0f;
      default: return 0.0f;
    }
  };
  while (s0 != sS) {
    int s1 = -1;
    switch (s0) {
      case sM: {
        float path[4];
        path[0] = (tMM[k] == 0.0f) ? -INFINITY : ox.M_(i - 1)[k - 1];
        path[1] = (tIM[k] == 0.0f) ? -INFINITY : ox.I_(i - 1)[k - 1];
        path[2] = (tDM[k] == 0.0f) ? -INFINITY : ox.D_(i - 1)[k - 1];
        path[3] = (bm[k]  == 0.0f) ? -INFINITY : ox.X(i - 1, xB_);
        static const int state[4] = { sM, sI, sD, sB };
        int best = 0;
        for (int a = 1; a < 4; ++a) if (path[a] > path[best]) best = a;     // esl_vec_FArgMax: first maximum
        s1 = state[best]; k--; i--;
        break;
      }
      case sD: {
        const float p0 = (tMD[k - 1] == 0.0f) ? -INFINITY : ox.M_(i)[k - 1];
        const float p1 = (tDD[k - 1] == 0.0f) ? -INFINITY : ox.D_(i)[k - 1];
        s1 = (p0 >= p1) ? sM : sD; k--;
        break;
      }
      case sI: {
        const float p0 = (tMI[k] == 0.0f) ? -INFINITY : ox.M_(i - 1)[k];
        const float p1 = (tII[k] == 0.0f) ? -INFINITY : ox.I_(i - 1)[k];
        s1 = (p0 >= p1) ? sM : sI; i--;
        break;
      }
      case sN: s1 = (i == 0) ? sS : sN; break;
      case sC: {
        const float t1 = (om.xf[XC][LOOP] == 0.0f) ? 0.0f : 1.0f, t2 = (om.xf[XE][MOVE] == 0.0f) ? 0.0f : 1.0f;
        const float p0 = t1 * (ox.X(i - 1, xC_) + pp.X(i, xC_)), p1 = t2 * ox.X(i, xE_);
        s1 = (p0 > p1) ? sC : sE;
        break;
      }
      case sJ: {
        const float t1 = (om.xf[XJ][LOOP] == 0.0f) ? 0.0f : 1.0f, t2 = (om.xf[XE][LOOP] == 0.0f) ? 0.0f : 1.0f;
        const float p0 = t1 * (ox.X(i - 1, xJ_) + pp.X(i, xJ_)), p1 = t2 * ox.X(i, xE_);
        s1 = (p0 > p1) ? sJ : sE;
        break;
      }
      case sE: {   // striped visiting order: q outer, lanes inner; M beats D on ties (>= vs >)
        float mx = -INFINITY; int smax = -1, kmax = 0;
        const float *mr = ox.M_(i), *dr = ox.D_(i);
        for (int q = 0; q < Q; ++q) {
          for (int z = 0; z < 4; ++z) { const int kk = z * Q + q + 1; if (kk <= M && mr[kk] >= mx) { mx = mr[kk]; smax = sM; kmax = kk; } }
          for (int z = 0; z < 4; ++z) { const int kk = z * Q + q + 1; if (kk <= M && dr[kk] >  mx) { mx = dr[kk]; smax = sD; kmax = kk; } }
        }
        k = kmax; s1 = smax;
        break;
      }
      case sB: {
        const float t1 = (om.xf[XN][MOVE] == 0.0f) ? 0.0f : 1.0f, t2 = (om.xf[XJ][MOVE] == 0.0f) ? 0.0f : 1.0f;
        s1 = (t1 * ox.X(i, xN_) > t2 * ox.X(i, xJ_)) ? sN : sJ;
        break;
      }
      default: return P7X_EINVAL;
    }
    if (s1 == -1) return P7X_EINVAL;
    tr.append(s1, k, i, postprob(s1, s0, k, i));
    if ((s1 == sN || s1 == sJ || s1 == sC) && s1 == s0) i--;
    s0 = s1;
  }
  tr.reverse();
  return P7X_OK;
}

// ---------------------------------------------------------------- p7_StochasticTrace
// The choices are made through p7x_choice.hpp (integer thresholds against the generator's 32-bit state -- the reference's
// floating-point test restated exactly, see there): the same functions the device fills its choice records with.
int stochastic_trace(FastRng &rng, const Model &om, const Matrix &fx, int L, Trace &tr)
{
  const int M = om.M, Q = om.p->Q4();
  const float *bm = om.tf(0), *tMM = om.tf(1), *tIM = om.tf(2), *tDM = om.tf(3), *tMD = om.tf(4), *tMI = om.tf(5), *tII = om.tf(6), *tDD = om.tf(7);
  int i = L, k = 0;
  tr.clear();
  tr.append(sT, k, i, 0.0f);
  tr.append(sC, k, i, 0.0f);
  int s0 = sC;
  auto pair = [&](float a, float b) -> int {
    uint32_t T, bits;
    choice_pair(a, b, &T, &bits);
    return choice_pick_pair(T, bits, rng.next_u32());
  };
  while (s0 != sS) {
    int s1 = -1;
    switch (s0) {
      case sM: {
        if (i < 1 || k < 1) return P7X_EINVAL;
        uint32_t c4[4];
        choice_cell_m(fx.X(i - 1, xB_) * bm[k], fx.M_(i - 1)[k - 1] * tMM[k], fx.I_(i - 1)[k - 1] * tIM[k], fx.D_(i - 1)[k - 1] * tDM[k], c4);
        static const int state[4] = { sB, sM, sI, sD };
        s1 = state[choice_pick_m(c4, rng.next_u32())]; k--; i--;
        break;
      }
      case sD: {
        if (i < 1 || k < 1) return P7X_EINVAL;
        s1 = pair(fx.M_(i)[k - 1] * tMD[k - 1], fx.D_(i)[k - 1] * tDD[k - 1]) == 0 ? sM : sD; k--;
        break;
      }
      case sI: {
        if (i < 1 || k < 1) return P7X_EINVAL;
        s1 = pair(fx.M_(i - 1)[k] * tMI[k], fx.I_(i - 1)[k] * tII[k]) == 0 ? sM : sI; i--;
        break;
      }
      case sN: s1 = (i == 0) ? sS : sN; break;
      case sC: {
        if (i < 1) return P7X_EINVAL;
        s1 = pair(fx.X(i - 1, xC_) * om.xf[XC][LOOP], fx.X(i, xE_) * om.xf[XE][MOVE] * fx.X(i, xS_)) == 0 ? sC : sE;
        break;
      }
      case sJ: {
        if (i < 1) return P7X_EINVAL;
        s1 = pair(fx.X(i - 1, xJ_) * om.xf[XJ][LOOP], fx.X(i, xE_) * om.xf[XE][LOOP] * fx.X(i, xS_)) == 0 ? sJ : sE;
        break;
      }
      case sE: {
        double sum = 0.0;
        const double roll = rng.next();
        const float norm = (float) (1.0 / fx.X(i, xE_));
        const float *mr = fx.M_(i), *dr = fx.D_(i);
        bool done = false;
        for (int pass = 0; pass < 2 && !done; ++pass) {
          for (int q = 0; q < Q && !done; ++q) {
            for (int z = 0; z < 4 && !done; ++z) { const int kk = z * Q + q + 1; sum += (kk <= M ? mr[kk] * norm : 0.0f); if (roll < sum) { k = kk; s1 = sM; done = true; } }
            for (int z = 0; z < 4 && !done; ++z) { const int kk = z * Q + q + 1; sum += (kk <= M ? dr[kk] * norm : 0.0f); if (roll < sum) { k = kk; s1 = sD; done = true; } }
          }
          if (!done && sum < 0.99) return P7X_EINVAL;
        }
        if (!done) return P7X_EINVAL;
        break;
      }
      case sB: {
        s1 = pair(fx.X(i, xN_) * om.xf[XN][MOVE], fx.X(i, xJ_) * om.xf[XJ][MOVE]) == 0 ? sN : sJ;
        break;
      }
      default: return P7X_EINVAL;
    }
    if (s1 == -1) return P7X_EINVAL;
    tr.append(s1, k, i, 0.0f);
    if ((s1 == sN || s1 == sJ || s1 == sC) && s1 == s0) i--;
    s0 = s1;
  }
  tr.reverse();
  return P7X_OK;
}

// ---------------------------------------------------------------- p7_Null2_ByTrace
P7X_MULTIVERSION void null2_by_trace(const Model &om, const Trace &tr, int zstart, int zend, float *wm, float *wi, float *null2)
{ // wm / wi: [M+2] scratch.  The sums run in upstream's striped order (4 lanes, q ascending) for every residue at once:
  // residue-minor odds make the inner loop a plain vector update, and nodes the trace never visited contribute
  // exact zeros, so they are skipped.
  const int M = om.M, Q = om.p->Q4(), K = om.p->K;
  constexpr int KP = Model::kKpad;
  (void) wi;          // the insert slots stay zero (see below): adding them is adding 0.0f, which is exact, so they are left out
  for (int k = 0; k <= M + 1; ++k) wm[k] = 0.0f;
  float eN = 0.0f, eC = 0.0f, eJ = 0.0f;
  int Ld = 0;
  for (int z = zstart; z <= zend; ++z) {
    if (tr.i[z] == 0) continue;
    Ld++;
    // upstream computes a match/insert selector here and then never uses it: the usage count of an insert
    // emission lands in the MATCH slot of node k as well (the insert slot stays zero)
    if (tr.k[z] > 0) wm[tr.k[z]] += 1.0f;
    else switch (tr.st[z]) { case sN: eN += 1.0f; break; case sC: eC += 1.0f; break; case sJ: eJ += 1.0f; break; default: break; }
  }
  const float norm = 1.0 / (float) Ld;
  for (int k = 1; k <= M; ++k) wm[k] *= norm;
  eN *= norm; eC *= norm; eJ *= norm;
  const float xfactor = eN + eC + eJ;
  float acc[4][KP];
  for (int z = 0; z < 4; ++z) for (int x = 0; x < KP; ++x) acc[z][x] = 0.0f;
  const float *__restrict rfT = om.rfT.data();
  for (int q = 0; q < Q; ++q)
    for (int z = 0; z < 4; ++z) {
      const int k = q + 1 + z * Q;
      if (k > M) continue;
      const float w = wm[k];
      if (w == 0.0f) continue;
      const float *__restrict r = rfT + (size_t) k * KP;
      float *__restrict a = acc[z];
      for (int x = 0; x < KP; ++x) a[x] = a[x] + w * r[x];
    }
  for (int x = 0; x < K; ++x) null2[x] = ((acc[0][x] + acc[1][x]) + (acc[2][x] + acc[3][x])) + xfactor;
  finish_null2(*om.p, null2);
}

// ---------------------------------------------------------------- p7_spensemble
struct SpCoord { int idx, i, j, k, m; float prob; };

bool sp_link(const SpCoord &h1, const SpCoord &h2, float min_overlap, bool of_smaller, int max_diagdiff)
{
  int nov = std::min(h1.j, h2.j) - std::max(h1.i, h2.i) + 1;
  int n = of_smaller ? std::min(h1.j - h1.i + 1, h2.j - h2.i + 1) : std::max(h1.j - h1.i + 1, h2.j - h2.i + 1);
  if ((float) nov / (float) n < min_overlap) return false;
  nov = std::min(h1.m, h2.m) - std::max(h1.k, h2.k);
  n = of_smaller ? std::min(h1.m - h1.k + 1, h2.m - h2.k + 1) : std::max(h1.m - h1.k + 1, h2.m - h2.k + 1);
  if ((float) nov / (float) n < min_overlap) return false;
  int d1 = h1.i - h1.k, d2 = h2.i - h2.k; if (std::abs(d1 - d2) <= max_diagdiff) return true;
  d1 = h1.j - h1.m; d2 = h2.j - h2.m;     if (std::abs(d1 - d2) <= max_diagdiff) return true;
  return false;
}

// esl_cluster_SingleLinkage: same traversal order as Easel, so cluster numbers agree
void single_linkage(const std::vector<SpCoord> &sp, float min_overlap, bool of_smaller, int max_diagdiff,
                    std::vector<int> &assign, int &nc)
{
  const int n = (int) sp.size();
  std::vector<int> a(n), b(n);
  assign.assign(n, 0);
  for (int v = 0; v < n; ++v) a[v] = n - v - 1;
  int na = n; nc = 0;
  while (na > 0) {
    int v = a[na - 1]; na--;
    b[0] = v; int nb = 1;
    while (nb > 0) {
      v = b[nb - 1]; nb--;
      assign[v] = nc;
      for (int i = na - 1; i >= 0; --i)
        if (sp_link(sp[v], sp[a[i]], min_overlap, of_smaller, max_diagdiff)) { b[nb++] = a[i]; a[i] = a[na - 1]; na--; }
    }
    nc++;
  }
}

void sp_cluster(const std::vector<SpCoord> &sp, int nsamples, float min_overlap, bool of_smaller, int max_diagdiff,
                float min_posterior, float min_endpointp, std::vector<SpCoord> &sigc)
{
  std::vector<int> assign; int nc = 0;
  single_linkage(sp, min_overlap, of_smaller, max_diagdiff, assign, nc);
  const int n = (int) sp.size();
  sigc.clear();
  std::vector<int> epc;
  for (int c = 0; c < nc; ++c) {
    int idx_of_last = -1, ninc = 0;
    for (int h = 0; h < n; ++h) if (assign[h] == c) { if (sp[h].idx != idx_of_last) ninc++; idx_of_last = sp[h].idx; }
    if ((float) ninc / (float) nsamples < min_posterior) continue;
    int imin = 0, imax = 0, jmin = 0, jmax = 0, kmin = 0, kmax = 0, mmin = 0, mmax = 0;
    for (int h = 0; h < n; ++h) if (assign[h] == c) {
      if (imin == 0) { imin = imax = sp[h].i; jmin = jmax = sp[h].j; kmin = kmax = sp[h].k; mmin = mmax = sp[h].m; }
      else {
        imin = std::min(imin, sp[h].i); imax = std::max(imax, sp[h].i);
        jmin = std::min(jmin, sp[h].j); jmax = std::max(jmax, sp[h].j);
        kmin = std::min(kmin, sp[h].k); kmax = std::max(kmax, sp[h].k);
        mmin = std::min(mmin, sp[h].m); mmax = std::max(mmax, sp[h].m);
      }
    }
    const int epc_threshold = (int) std::ceil((float) ninc * min_endpointp);
    auto argmax = [&](int w) { int b = 0; for (int q = 1; q < w; ++q) if (epc[q] > epc[b]) b = q; return b; };
    int best_i = 0, best_j = 0, best_k = 0, best_m = 0;
    epc.assign(imax - imin + 1, 0);
    for (int h = 0; h < n; ++h) if (assign[h] == c) epc[sp[h].i - imin]++;
    for (int i = imin; i <= imax; ++i) if (epc[i - imin] >= epc_threshold) { best_i = i; break; }
    if (best_i == 0) best_i = argmax(imax - imin + 1) + imin;
    epc.assign(kmax - kmin + 1, 0);
    for (int h = 0; h < n; ++h) if (assign[h] == c) epc[sp[h].k - kmin]++;
    for (int k = kmin; k <= kmax; ++k) if (epc[k - kmin] >= epc_threshold) { best_k = k; break; }
    if (best_k == 0) best_k = argmax(kmax - kmin + 1) + kmin;
    epc.assign(jmax - jmin + 1, 0);
    for (int h = 0; h < n; ++h) if (assign[h] == c) epc[sp[h].j - jmin]++;
    for (int j = jmax; j >= jmin; --j) if (epc[j - jmin] >= epc_threshold) { best_j = j; break; }
    if (best_j == 0) best_j = argmax(jmax - jmin + 1) + jmin;
    epc.assign(mmax - mmin + 1, 0);
    for (int h = 0; h < n; ++h) if (assign[h] == c) epc[sp[h].m - mmin]++;
    for (int m = mmax; m >= mmin; --m) if (epc[m - mmin] >= epc_threshold) { best_m = m; break; }
    if (best_m == 0) best_m = argmax(mmax - mmin + 1) + mmin;
    if (best_i > best_j || best_k > best_m) continue;
    sigc.push_back(SpCoord{ c, best_i, best_j, best_k, best_m, (float) ninc / (float) nsamples });
  }
  std::stable_sort(sigc.begin(), sigc.end(), [](const SpCoord &a, const SpCoord &b) { return a.i < b.i; });
}

} // anonymous namespace

// ---------------------------------------------------------------- p7_alidisplay_Create (domain 0 of an OA trace)
void make_alidisplay(const Profile &p, const Trace &tr, const uint8_t *dsq, int L, Domain &dom)
{
  const Alphabet &abc = Alphabet::get(p.abc_type);
  const int N = (int) tr.st.size();
  int z1 = 0, z2;
  for (z1 = 0; z1 < N; ++z1) if (tr.st[z1] == sB) break;
  z1++;                                           // first state after B
  for (z2 = z1 + 1; z2 < N; ++z2) if (tr.st[z2] == sE) break;
  z2--;                                           // last state before E
  dom.N = z2 - z1 + 1;
  dom.hmmfrom = tr.k[z1]; dom.hmmto = tr.k[z2]; dom.M = p.M;
  dom.sqfrom = tr.i[z1]; dom.sqto = tr.i[z2]; dom.L = L;
  dom.model.assign(dom.N, ' '); dom.mline.assign(dom.N, ' '); dom.aseq.assign(dom.N, ' '); dom.ppline.assign(dom.N, ' ');
  const bool has_rf = p.rf.size() > 1 && p.rf[0] != 0, has_mm = p.mm.size() > 1 && p.mm[0] != 0, has_cs = p.cs.size() > 1 && p.cs[0] != 0;
  if (has_rf) dom.rfline.assign(dom.N, ' ');
  if (has_mm) dom.mmline.assign(dom.N, ' ');
  if (has_cs) dom.csline.assign(dom.N, ' ');
  // residue code of a consensus character (strchr over the alphabet's symbols, upper-cased): tabulated per call instead
  // of searched per aligned column -- most of this function's time was the search
  signed char code_of[256];
  std::memset(code_of, -1, sizeof code_of);
  for (int x = (int) std::strlen(abc.sym) - 1; x >= 0; --x) code_of[(unsigned char) abc.sym[x]] = (signed char) x;     // first occurrence wins, as strchr
  auto digitize = [&](char c) -> int { return code_of[(unsigned char) std::toupper((unsigned char) c)]; };
  for (int z = z1; z <= z2; ++z) {
    const int k = tr.k[z], i = tr.i[z], s = tr.st[z], o = z - z1;
    const char cons = (k >= 1 && (int) p.consensus.size() > k) ? p.consensus[k] : 'x';
    if (has_rf) dom.rfline[o] = (s == sI) ? '.' : p.rf[k];
    if (has_mm) dom.mmline[o] = (s == sI) ? '.' : p.mm[k];
    if (has_cs) dom.csline[o] = (s == sI) ? '.' : p.cs[k];
    switch (s) {
      case sM: {
        const int x = dsq[i];
        dom.model[o] = cons;
        if (x == digitize(cons)) dom.mline[o] = cons;
        else if (p.rf_[(size_t) x * (p.M + 1) + k] > 1.0f) dom.mline[o] = '+';
        else dom.mline[o] = ' ';
        dom.aseq[o] = (char) std::toupper((unsigned char) abc.sym[x]);
        break;
      }
      case sI: dom.model[o] = '.'; dom.mline[o] = ' '; dom.aseq[o] = (char) std::tolower((unsigned char) abc.sym[dsq[i]]); break;
      case sD: dom.model[o] = cons; dom.mline[o] = ' '; dom.aseq[o] = '-'; break;
      default: break;
    }
    if (s == sD) dom.ppline[o] = '.';
    else { const float pv = tr.pp[z]; dom.ppline[o] = (pv + 0.05 >= 1.0) ? '*' : (char) ((int) ((pv + 0.05) * 10.0) + '0'); }
  }
}

// ---------------------------------------------------------------- rescore_isolated_domain
// upstream reparameterize_model + p7_oprofile_UpdateFwdEmissionScores: the background becomes
//   bg'[x] = (1 - s) * composition(dsq[i..j])[x] + s * bg->f[x],   s = 25 / min(100, max(50, n)),  n = window length
// (0.25 for every window of 100 residues or more), and the match odds rf'[x][k] = match_prob[k][x] / bg'[x], degenerate
// codes by expectation under bg'.  Pinned by bmyD1/bmyD2.tbl and the RF00001 answers (all windows there are > 100 nt; the
// short-window branch of s is restated from upstream and not pinned by any fixture).
void reparameterize(const Profile &p, const LongTargetOpts &lt, const uint8_t *dsq, int n, int i, int j, std::vector<float> &rf)
{
  const int M = p.M, K = p.K, Kp = p.Kp;
  const Alphabet &abc = Alphabet::get(p.abc_type);
  const float bg_smooth = 25.0f / (float) std::min(100, std::max(50, n));
  float cnt[MAXK];
  for (int x = 0; x < K; ++x) cnt[x] = 0.0f;
  for (int pos = i; pos <= j; ++pos) {           // esl_sq_CountResidues: degenerate residues count fractionally
    const int x = dsq[pos];
    if (x < K) cnt[x] += 1.0f;
    else if (x > K && x <= Kp - 3) {
      int nd = 0; for (int y = 0; y < K; ++y) nd += abc.degen[x][y] ? 1 : 0;
      for (int y = 0; y < K; ++y) if (abc.degen[x][y]) cnt[y] += 1.0f / (float) nd;
    }
  }
  float tot = 0.0f; for (int x = 0; x < K; ++x) tot += cnt[x];
  float bgn[MAXK];
  for (int x = 0; x < K; ++x) bgn[x] = (1.0f - bg_smooth) * (tot > 0 ? cnt[x] / tot : p.bgf[x]) + bg_smooth * p.bgf[x];
  rf.assign((size_t) Kp * (M + 1), 0.0f);
  for (int k = 1; k <= M; ++k) {
    float sc[MAXKP];
    for (int x = 0; x < K; ++x) sc[x] = logf(lt.match_prob[(size_t) k * K + x] / bgn[x]);
    sc[K] = sc[Kp - 2] = sc[Kp - 1] = -INFINITY;
    for (int x = K + 1; x <= Kp - 3; ++x) {      // esl_abc_FExpectScVec with the new background
      float num = 0.f, den = 0.f;
      for (int y = 0; y < K; ++y) if (abc.degen[x][y]) { num += sc[y] * bgn[y]; den += bgn[y]; }
      sc[x] = num / den;
    }
    for (int x = 0; x < Kp; ++x) rf[(size_t) x * (M + 1) + k] = expf(sc[x]);
  }
}

int rescore_isolated_domain(const Profile &p, Model &om, const uint8_t *dsq, int L, int i, int j, bool null2_is_done,
                            DomainWorkspace &ws, DomainDefResult &dd)
{
  const LongTargetOpts *lt = om.lt;
  int Ld = j - i + 1;
  float envsc = 0.0f, oasc = 0.0f;
  float save_xf[4][2];
  thread_local std::vector<float> rf_lt;
  if (lt) std::memcpy(save_xf, om.xf, sizeof(save_xf));
  struct Restore { Model &om; const LongTargetOpts *lt; float (*xf)[2];
                   ~Restore() { if (lt) { om.rf_over = nullptr; std::memcpy(om.xf, xf, sizeof(float) * 8); } } } restore{ om, lt, save_xf };
  // Long targets (upstream rescore_isolated_domain with long_target = TRUE): the envelope is scored unihit under a length
  // model of its OWN length (p7_oprofile_ReconfigRestLength(om, j-i+1); the pipeline re-expresses the score for max_length
  // afterwards) and, with null2 on, against emissions re-derived for a background mixed with the envelope's composition.
  auto lt_setup = [&]() {
    om.configure(false, Ld);
    if (lt->do_null2) { reparameterize(p, *lt, dsq, L, i, j, rf_lt); om.rf_over = rf_lt.data(); om.sr_of = nullptr; }     // (same buffer, new odds: the striped copy is stale)
  };
  auto align = [&]() -> int {
    { ProfScope ps(5); forward_full(om, dsq + i - 1, Ld, ws.fwd, &envsc); }
    { ProfScope ps(6); backward_full(om, dsq + i - 1, Ld, ws.fwd, ws.bck, nullptr); }
    { ProfScope ps(7); if (decoding(om, ws.fwd, ws.bck) == P7X_ERANGE) return P7X_ENORESULT; }   // repetitive garbage; the envelope is dropped
    { ProfScope ps(8); optimal_accuracy(om, ws.bck, ws.fwd, &oasc); }                              // <fwd> now holds the OA matrix
    ProfScope ps9(9);
    if (oa_trace(om, ws.bck, ws.fwd, ws.tr) != P7X_OK) return P7X_EINVAL;
    for (size_t z = 0; z < ws.tr.st.size(); ++z) if (ws.tr.i[z] > 0) ws.tr.i[z] += i - 1;
    return P7X_OK;
  };
  if (lt) lt_setup();
  int st = align();
  if (st != P7X_OK) return st;
  Domain dom;
  make_alidisplay(p, ws.tr, dsq, L, dom);
  if (lt && (i < dom.sqfrom - lt->max_env_extra || j > dom.sqto + lt->max_env_extra)) {
    // long targets often give envelopes far wider than the alignment (a repetitive stretch of the model collecting
    // weak matches): trim the envelope to the alignment +- max_env_extra and do it again
    i = std::max<int>(i, (int) dom.sqfrom - lt->max_env_extra);
    j = std::min<int>(j, (int) dom.sqto + lt->max_env_extra);
    Ld = j - i + 1;
    lt_setup();
    if ((st = align()) != P7X_OK) return st;
    dom = Domain();
    make_alidisplay(p, ws.tr, dsq, L, dom);
  }
  float domcorrection = 0.0f;
  if (lt) {
    if (lt->do_null2) {
      // the bias of a long-target envelope is the score it loses against the composition-adjusted background; the
      // envelope score itself is the unmodified model's (Forward again with the original emissions)
      float orig = 0.0f;
      om.rf_over = nullptr;
      forward_full(om, dsq + i - 1, Ld, ws.fwd, &orig);
      domcorrection = std::max(0.0f, orig - envsc);
      envsc = orig;
    }
  } else {
    if (!null2_is_done) {
      float null2[MAXKP];
      ProfScope psn(10);
      null2_by_expectation(om, ws.bck, null2);
      float ln2[MAXKP];                                   // one logarithm per residue code, not per residue
      for (int x = 0; x < p.Kp; ++x) ln2[x] = logf(null2[x]);
      for (int pos = i; pos <= j; ++pos) dd.n2sc[pos] = ln2[dsq[pos]];
    }
    for (int pos = i; pos <= j; ++pos) domcorrection += dd.n2sc[pos];
  }
  dom.domcorrection = domcorrection;
  dom.ienv = i; dom.jenv = j; dom.envsc = envsc; dom.oasc = oasc;
  dom.iali = dom.sqfrom; dom.jali = dom.sqto;
  dd.dcl.push_back(std::move(dom));
  return P7X_OK;
}


// ---------------------------------------------------------------- p7_domaindef_ByPosteriorHeuristics
// Step 1: posterior decoding of the special states (p7_DomainDecoding) and the region scan.
int domaindef_regions(const Profile &p, int L, const float *fx, const float *bx, DomainDefResult &dd, std::vector<Region> &regs)
{
  const float rt1 = 0.25f, rt2 = 0.10f, rt3 = 0.20f;                         // p7_domaindef.pxd:39-41
  Model om{ &p, p.M, {} };
  dd.dcl.clear(); dd.n2sc.assign(L + 1, 0.0f); dd.multi.clear();
  dd.nregions = dd.nclustered = dd.noverlaps = dd.nenvelopes = 0;
  regs.clear();
  om.configure(true, L);
  thread_local std::vector<float> btot, etot, mocc;
  btot.resize(L + 1); etot.resize(L + 1); mocc.resize(L + 1);
  {
    float scaleproduct = 1.0 / bx[0 * NX + xN_];
    btot[0] = etot[0] = mocc[0] = 0.0f;
    for (int i = 1; i <= L; ++i) {
      btot[i] = btot[i - 1] + (fx[(i - 1) * NX + xB_] * bx[(i - 1) * NX + xB_]) * fx[(i - 1) * NX + xS_] * scaleproduct;
      etot[i] = etot[i - 1] + (fx[i * NX + xE_] * bx[i * NX + xE_]) * fx[i * NX + xS_] * scaleproduct;
      float njcp = fx[(i - 1) * NX + xN_] * bx[i * NX + xN_] * om.xf[XN][LOOP] * scaleproduct;
      njcp += fx[(i - 1) * NX + xJ_] * bx[i * NX + xJ_] * om.xf[XJ][LOOP] * scaleproduct;
      njcp += fx[(i - 1) * NX + xC_] * bx[i * NX + xC_] * om.xf[XC][LOOP] * scaleproduct;
      mocc[i] = 1. - njcp;
    }
    if (std::isinf(scaleproduct)) return P7X_ERANGE;
  }
  dd.nexpected = btot[L];
  int i = -1; bool triggered = false;
  for (int j = 1; j <= L; ++j) {
    if (!triggered) {
      if (mocc[j] - (btot[j] - btot[j - 1]) < rt2) i = j;
      else if (i == -1) i = j;
      if (mocc[j] >= rt1) triggered = true;
    } else if (mocc[j] - (etot[j] - etot[j - 1]) < rt2) {
      dd.nregions++;
      float mx = -1.0f;                                                      // is_multidomain_region
      for (int z = i; z <= j; ++z) mx = std::max(mx, std::min(etot[z] - etot[i - 1], btot[j] - btot[z - 1]));
      regs.push_back(Region{ i, j, mx >= rt3 });
      i = -1; triggered = false;
    }
  }
  return P7X_OK;
}

static thread_local const LongTargetOpts *t_long_target = nullptr;     // LongTargetScope: set by the long-target pipeline around its calls
LongTargetScope::LongTargetScope(const LongTargetOpts &lt) { t_long_target = &lt; }
LongTargetScope::~LongTargetScope() { t_long_target = nullptr; }

// Step 2 for a multi-domain region: region_trace_ensemble (sampled tracebacks from a multihit Forward matrix of the
// region, single-linkage clustering of their domain coordinates), then every surviving envelope is rescored.

int domaindef_multi_region(const Profile &p, const uint8_t *dsq, int L, int i, int j, uint32_t seed, bool do_reseeding,
                           MultiRegionState &state, DomainDefResult &dd, std::vector<Domain> &out,
                           std::vector<EnvelopeRequest> *defer2, int item, const EnsembleResult *ens)
{
  const int nsamples = 200;                                                  // p7_domaindef.pxd:43-48
  const float min_overlap = 0.8f, min_posterior = 0.25f, min_endpointp = 0.02f;
  const bool of_smaller = true; const int max_diagdiff = 4;
  thread_local DomainWorkspace ws;
  Model om{ &p, p.M, {} };
  om.lt = t_long_target;
  om.prepare();
  const int Lr = j - i + 1;
  std::vector<SpCoord> sp;
  dd.nclustered++;
  if (ens && ens->status >= 0 && (ens->status & 64) && ens->status < 128) dd.nens_redone++;
  if (ens && ens->status == 0 && do_reseeding && !om.lt) {
    dd.nens_device++;
    // the ensemble was sampled on the device (p7x_ensemble.hip): end points and null2 sums are in; a sample's domains come
    // in traceback order and go into the list first domain first, as p7_trace_Index numbers them
    sp.reserve((size_t) ens->ndom);
    for (int a = 0; a < ens->ndom; ) {
      int b = a;
      while (b < ens->ndom && ens->dom[(size_t) b * 5] == ens->dom[(size_t) a * 5]) ++b;
      for (int d = b - 1; d >= a; --d) {
        const int32_t *o = ens->dom + (size_t) d * 5;
        sp.push_back(SpCoord{ o[0], o[1] + i - 1, o[2] + i - 1, o[3], o[4], 0.0f });
      }
      a = b;
    }
    for (int pos = 1; pos <= Lr; ++pos) dd.n2sc[i + pos - 1] = logf(ens->n2[pos] / (float) nsamples);
  } else {
    om.prepare_rfT();
    ws.wm.resize(p.M + 2); ws.wi.resize(p.M + 2);
    FastRng rng; rng.seed = state.rng_seed; rng.x = state.rng_x;
    if (!state.started) { rng.init(seed); state.started = true; }
    om.configure(true, L);
    { ProfScope ps(1); forward_full(om, dsq + i - 1, j - i + 1, ws.fwd, nullptr); }
    for (int pos = i; pos <= j; ++pos) dd.n2sc[pos] = 0.0f;
    if (do_reseeding) rng.init(seed);
    float null2[MAXKP];
    for (int t = 0; t < nsamples; ++t) {
      { ProfScope ps(2); if (stochastic_trace(rng, om, ws.fwd, Lr, ws.tr) != P7X_OK) return P7X_EINVAL; }
      ws.tr.index();
      if (ens && ens->raw_out && ens->raw_out->want_traces) {      // test seam: the path itself
        EnsembleRaw &raw = *ens->raw_out;
        raw.off.push_back((int32_t) raw.st.size());
        raw.st.insert(raw.st.end(), ws.tr.st.begin(), ws.tr.st.end());
        raw.k.insert(raw.k.end(), ws.tr.k.begin(), ws.tr.k.end());
        raw.i.insert(raw.i.end(), ws.tr.i.begin(), ws.tr.i.end());
      }
      int pos = 1;
      for (int d = 0; d < ws.tr.ndom; ++d) {
        sp.push_back(SpCoord{ t, ws.tr.sqfrom[d] + i - 1, ws.tr.sqto[d] + i - 1, ws.tr.hmmfrom[d], ws.tr.hmmto[d], 0.0f });
        { ProfScope ps(3); null2_by_trace(om, ws.tr, ws.tr.tfrom[d], ws.tr.tto[d], ws.wm.data(), ws.wi.data(), null2); }
        for (; pos <= ws.tr.sqfrom[d]; ++pos) dd.n2sc[i + pos - 1] += 1.0f;   // sic: the first domain residue counts as "outside"
        for (; pos <= ws.tr.sqto[d]; ++pos) dd.n2sc[i + pos - 1] += null2[dsq[i + pos - 1]];
      }
      for (; pos <= Lr; ++pos) dd.n2sc[i + pos - 1] += 1.0f;
    }
    state.rng_seed = rng.seed; state.rng_x = rng.x;
    if (ens && ens->raw_out) {            // test seam: the ensemble as sampled, before the logarithm and the clustering
      ens->raw_out->dom.clear();
      for (const SpCoord &c : sp) { ens->raw_out->dom.push_back(c.idx); ens->raw_out->dom.push_back(c.i - i + 1); ens->raw_out->dom.push_back(c.j - i + 1); ens->raw_out->dom.push_back(c.k); ens->raw_out->dom.push_back(c.m); }
      ens->raw_out->n2.assign((size_t) Lr + 1, 0.0f);
      for (int pos = 1; pos <= Lr; ++pos) ens->raw_out->n2[(size_t) pos] = dd.n2sc[i + pos - 1];
    }
    for (int pos = i; pos <= j; ++pos) dd.n2sc[pos] = logf(dd.n2sc[pos] / (float) nsamples);
  }
  std::vector<SpCoord> sigc;
  { ProfScope ps(4); sp_cluster(sp, nsamples, min_overlap, of_smaller, max_diagdiff, min_posterior, min_endpointp, sigc); }
  // remove envelopes dominated (>= 80% overlap of the smaller) by a more probable one
  const int nc0 = (int) sigc.size();
  std::vector<char> dominated(nc0, 0);
  for (int d = 0; d < nc0; ++d)
    for (int d2 = d + 1; d2 < nc0; ++d2) {
      const int nov = std::min(sigc[d].j, sigc[d2].j) - std::max(sigc[d].i, sigc[d2].i) + 1;
      if (nov == 0) break;
      const int n = std::min(sigc[d].j - sigc[d].i + 1, sigc[d2].j - sigc[d2].i + 1);
      if ((float) nov / (float) n >= 0.8f) { if (sigc[d].prob > sigc[d2].prob) dominated[d2] = 1; else dominated[d] = 1; }
    }
  om.configure(false, L);
  if (defer2 && !om.lt) {                  // the device rescores the clustered envelopes; overlaps are counted when its answers are in
    out.clear();
    for (int d = 0; d < nc0; ++d) {
      if (dominated[d]) continue;
      dd.nenvelopes++;
      Domain ph; ph.ienv = sigc[d].i; ph.jenv = sigc[d].j; ph.deferred2 = (int) defer2->size();
      defer2->push_back(EnvelopeRequest{ item, (int32_t) sigc[d].i, (int32_t) sigc[d].j });
      out.push_back(std::move(ph));
    }
    return P7X_OK;
  }
  int last_j2 = 0;
  std::vector<Domain> keep;
  keep.swap(dd.dcl);                       // rescore_isolated_domain() appends to dd.dcl: collect this region's domains apart
  for (int d = 0; d < nc0; ++d) {
    if (dominated[d]) continue;
    const int i2 = sigc[d].i, j2 = sigc[d].j;
    if (i2 <= last_j2) dd.noverlaps++;
    dd.nenvelopes++;
    if (rescore_isolated_domain(p, om, dsq, L, i2, j2, true, ws, dd) == P7X_OK) last_j2 = j2;
  }
  out = std::move(dd.dcl);
  dd.dcl.swap(keep);
  return P7X_OK;
}

static int dispatch_regions(const Profile &p, const uint8_t *dsq, int L, const Region *regs, int nregs, uint32_t seed,
                            bool do_reseeding, DomainDefResult &dd, std::vector<EnvelopeRequest> *defer, int item);

int domaindef_by_posterior_heuristics(const Profile &p, const uint8_t *dsq, int L, const float *fx, const float *bx,
                                      uint32_t seed, bool do_reseeding, DomainDefResult &dd,
                                      std::vector<EnvelopeRequest> *defer, int item)
{
  thread_local std::vector<Region> regs;
  const int st = domaindef_regions(p, L, fx, bx, dd, regs);
  if (st != P7X_OK) return st;
  return dispatch_regions(p, dsq, L, regs.data(), (int) regs.size(), seed, do_reseeding, dd, defer, item);
}

int domaindef_from_regions(const Profile &p, const uint8_t *dsq, int L, float nexpected, const Region *regs, int nregs,
                           uint32_t seed, bool do_reseeding, DomainDefResult &dd, std::vector<EnvelopeRequest> *defer, int item)
{
  dd.dcl.clear(); dd.n2sc.assign(L + 1, 0.0f); dd.multi.clear();
  dd.nclustered = dd.noverlaps = dd.nenvelopes = 0;
  dd.nregions = nregs; dd.nexpected = nexpected;
  return dispatch_regions(p, dsq, L, regs, nregs, seed, do_reseeding, dd, defer, item);
}

static int dispatch_regions(const Profile &p, const uint8_t *dsq, int L, const Region *regs, int nregs, uint32_t seed,
                            bool do_reseeding, DomainDefResult &dd, std::vector<EnvelopeRequest> *defer, int item)
{
  Model om{ &p, p.M, {} };
  om.lt = t_long_target;
  thread_local DomainWorkspace ws;
  bool prepared = false;
  MultiRegionState state;
  for (int ri = 0; ri < nregs; ++ri) {
    const Region &r = regs[ri];
    if (r.multi) {
      if (defer) {                    // resolved later by domaindef_multi_region(): leave a marker in domain order
        Domain ph; ph.ienv = r.i; ph.jenv = r.j; ph.deferred = -2; ph.multi_slot = (int) dd.multi.size();
        dd.multi.emplace_back();
        dd.dcl.push_back(std::move(ph));
        continue;
      }
      std::vector<Domain> doms;
      const int st2 = domaindef_multi_region(p, dsq, L, r.i, r.j, seed, do_reseeding, state, dd, doms);
      if (st2 != P7X_OK) return st2;
      for (Domain &d : doms) dd.dcl.push_back(std::move(d));
    } else {
      dd.nenvelopes++;
      if (defer) {                   // rescored on the device; domaindef_finish_deferred() fills the placeholder
        Domain ph; ph.ienv = r.i; ph.jenv = r.j; ph.deferred = (int) defer->size();
        defer->push_back(EnvelopeRequest{ item, r.i, r.j });
        dd.dcl.push_back(std::move(ph));
      } else {
        if (!prepared) { om.prepare(); om.configure(false, L); prepared = true; }
        rescore_isolated_domain(p, om, dsq, L, r.i, r.j, false, ws, dd);
      }
    }
  }
  return P7X_OK;
}

// The multi-domain regions left behind by the deferring call above, in order.
int domaindef_finish_multi(const Profile &p, const uint8_t *dsq, int L, uint32_t seed, bool do_reseeding, DomainDefResult &dd,
                           std::vector<EnvelopeRequest> *defer2, int item, const EnsembleResult *const *ens)
{
  MultiRegionState state;
  int nth = 0;
  for (Domain &d : dd.dcl) {
    if (d.deferred != -2) continue;
    const int st = domaindef_multi_region(p, dsq, L, (int) d.ienv, (int) d.jenv, seed, do_reseeding, state, dd, dd.multi[(size_t) d.multi_slot],
                                          defer2, item, ens ? ens[nth] : nullptr);
    ++nth;
    if (st != P7X_OK) return st;
  }
  return P7X_OK;
}

uint32_t fast_rng_state(uint32_t seed) { FastRng r; r.init(seed); return r.x; }

// ---------------------------------------------------------------- the parsers: special-state rows only
// The rows-only engines write into a Matrix whose special rows are the caller's vector (lent for the call).
struct RowsOf {
  Matrix mx; std::vector<float> &v;
  explicit RowsOf(std::vector<float> &rows) : v(rows) { mx.x.swap(v); }
  ~RowsOf() { v.swap(mx.x); v.resize((size_t) (mx.L + 1) * NX); }
};

int forward_parser_lanes(const Model &om, const uint8_t *dsq, int L, std::vector<float> &fx, float *ret_sc)
{
  RowsOf f(fx);
  return forward_rows_lanes(om, dsq, L, f.mx, ret_sc);
}

// (a 2,400-residue window of a 1,200-node model would stream 70 MB of full matrices through the host caches for rows the
// region scan never reads)
int backward_parser_lanes(const Model &om, const uint8_t *dsq, int L, const std::vector<float> &fx, std::vector<float> &bx)
{
  RowsOf b(bx);
  return backward_rows_lanes(om, dsq, L, fx.data(), b.mx, nullptr);
}

// p7_ForwardParser / p7_BackwardParser special-state rows in upstream's summation order, for the region-scan guard
// (p7x_tophits.cpp).  Memory: the rows themselves and O(M) of striped DP rows, whatever L x M is.
int parser_rows_upstream(const Profile &p, const uint8_t *dsq, int L, std::vector<float> &fx, std::vector<float> &bx)
{
  Model om{ &p, p.M, {} };
  om.prepare(0);
  om.configure(true, L);
  RowsOf f(fx), b(bx);
  const int st = forward_rows_upstream(om, dsq, L, f.mx, nullptr, striped_scratch());
  if (st != P7X_OK) return st;
  return backward_rows_upstream(om, dsq, L, f.mx.x.data(), b.mx, nullptr, striped_scratch());
}

// The F3 tie-breaker (the guard in p7x_tophits.cpp): the Forward parser score in upstream's summation order.  The device
// kernels and the lanes engines use other (faster) association orders, a few ulps apart -- which only matters for a target
// whose P-value sits on the F3 threshold.  dsq1[1..L]; multihit, length model of L as the pipeline configures the parser.
int host_forward_parser_exact(const Profile &p, const uint8_t *dsq1, int L, float *sc)
{
  Model om{ &p, p.M, {} };
  om.prepare(0);
  om.configure(true, L);
  Matrix ox;
  return forward_rows_upstream(om, dsq1, L, ox, sc, striped_scratch());
}

// p7_bg_FilterScore: Forward score of the two-state composition HMM (esl_hmm_Forward), float arithmetic as upstream
float bias_filter_score(const Profile &p, const uint8_t *dsq, int64_t L)
{
  if (L < 1) return null1_score((int) L);         // no residue 1 to start from: dsq[1] is the sentinel (bias_kernel does the same)
  const Alphabet &abc = Alphabet::get(p.abc_type);
  float eo[MAXKP][2];
  for (int x = 0; x < p.Kp; ++x) { eo[x][0] = 1.0f; eo[x][1] = 1.0f; }
  for (int x = 0; x < p.K; ++x) { eo[x][0] = p.bgf[x] / p.bgf[x]; eo[x][1] = p.compo[x] / p.bgf[x]; }
  for (int x = p.K + 1; x <= p.Kp - 3; ++x)
    for (int s = 0; s < 2; ++s) {
      float e = 0.0f, den = 0.0f;
      for (int y = 0; y < p.K; ++y) if (abc.degen[x][y]) { e += (s == 0 ? p.bgf[y] : p.compo[y]); den += p.bgf[y]; }
      eo[x][s] = den > 0.0f ? e / den : 0.0f;
    }
  const float p1 = (float) L / (float) (L + 1);
  const float L1 = (float) ((double) (float) p.M / 8.0);
  const float t00 = p1, t01 = 1.0f - p1, t10 = 1.0f / (L1 + 1.0f), t11 = L1 / (L1 + 1.0f);
  float dp0 = eo[dsq[1]][0] * 0.999f, dp1 = eo[dsq[1]][1] * 0.001f;
  float mx = std::max(0.0f, std::max(dp0, dp1));
  dp0 /= mx; dp1 /= mx;
  float logsc = 0.0f;
  logsc += (float) std::log((double) mx);
  for (int64_t i = 2; i <= L; ++i) {
    const int x = dsq[i];
    float n0 = 0.0f; n0 += dp0 * t00; n0 += dp1 * t10; n0 *= eo[x][0];
    float n1 = 0.0f; n1 += dp0 * t01; n1 += dp1 * t11; n1 *= eo[x][1];
    mx = std::max(0.0f, std::max(n0, n1));
    dp0 = n0 / mx; dp1 = n1 / mx;
    logsc += (float) std::log((double) mx);
  }
  float last = 0.0f; last += dp0 * 1.0f; last += dp1 * 1.0f;
  logsc += (float) std::log((double) last);
  return logsc + (float) L * logf(p1) + logf((float) (1. - (double) p1));
}
// the null score the F3 guard compares a Forward score against
float host_filter_null_score(const Profile &p, const uint8_t *dsq1, int L, bool do_bias) { return do_bias ? bias_filter_score(p, dsq1, L) : null1_score(L); }

// hmmalign's per-sequence step (upstream p7_tracealign_computeTraces): the profile unihit local with the sequence's own
// length model, the whole sequence as the envelope, Forward -> Backward -> Decoding -> OptimalAccuracy -> OATrace -- the
// steps of rescore_isolated_domain() without null2, in upstream's summation order unless <order> says otherwise (0
// upstream, 1 the device's, -1 the "host_order" seam).  dsq1[1..L]; the trace comes out in forward order.  P7X_ERANGE:
// p7_Decoding overflowed.
int align_trace_upstream(const Profile &p, const uint8_t *dsq1, int L, AlignTrace &out, int order, bool stop_on_own_scales)
{
  out = AlignTrace{};
  if (L <= 0) return P7X_OK;                    // an empty sequence: an empty trace
  // two full matrices of (L + 1) x (M + 2) cells: a worker keeps them for its next sequence, but not beyond 128 MiB (a
  // long model against a long sequence would otherwise leave gigabytes behind in every worker of the pool)
  thread_local DomainWorkspace ws;
  struct Shrink { DomainWorkspace &ws; ~Shrink() { if (ws.fwd.m.capacity() * sizeof(float) * 6 > ((size_t) 128 << 20)) ws = DomainWorkspace(); } } shrink{ ws };
  Model om{ &p, p.M, {} };
  om.prepare(order);
  om.configure(false, L);
  int st = forward_full(om, dsq1, L, ws.fwd, &out.fwdsc);
  if (st != P7X_OK) return st;
  if ((st = backward_full(om, dsq1, L, ws.fwd, ws.bck, nullptr)) != P7X_OK) return st;
  if (stop_on_own_scales && ws.bck.own_scales) return P7X_ERANGE;
  if (decoding(om, ws.fwd, ws.bck) == P7X_ERANGE) return P7X_ERANGE;
  optimal_accuracy(om, ws.bck, ws.fwd, &out.oasc);
  if (oa_trace(om, ws.bck, ws.fwd, ws.tr) != P7X_OK) return P7X_EINVAL;
  out.st = ws.tr.st; out.k = ws.tr.k; out.i = ws.tr.i; out.pp = ws.tr.pp;
  return P7X_OK;
}

// The event that sends a sequence to hmmalign's log-space path, without the alignment: Forward's and Backward's special rows
// in upstream's order on two rolling DP rows, as the parsers run them, but unihit with the sequence's own length model.
bool align_leaves_forward_scales(const Profile &p, const uint8_t *dsq1, int L)
{
  if (L <= 0) return false;
  Model om{ &p, p.M, {} };
  om.prepare(0);
  om.configure(false, L);
  thread_local std::vector<float> fx, bx;
  RowsOf f(fx), b(bx);
  if (forward_rows_upstream(om, dsq1, L, f.mx, nullptr, striped_scratch()) != P7X_OK) return true;
  if (backward_rows_upstream(om, dsq1, L, f.mx.x.data(), b.mx, nullptr, striped_scratch()) != P7X_OK) return true;
  return b.mx.own_scales;
}

// A device trace (traceback order, EnvelopeResult's packing: state | k << 8) in forward order, as p7_trace_Reverse leaves it
void align_trace_from_device(const uint32_t *ta, const int32_t *ti, const float *tp, int n, AlignTrace &out)
{
  Trace tr;
  for (int z = 0; z < n; ++z) tr.append((int) (ta[z] & 0xffu), (int) ((ta[z] >> 8) & 0xffffu), ti[z], tp[z]);
  tr.reverse();
  out.st = std::move(tr.st); out.k = std::move(tr.k); out.i = std::move(tr.i); out.pp = std::move(tr.pp);
}

// Second half of rescore_isolated_domain() for envelopes rescored by the device kernel: trace -> alignment
// display, null2 odds -> per-residue corrections.  req_index[n] is the position in <res> of local request n
// (Domain::deferred of the placeholders of this target).
int domaindef_finish_deferred(const Profile &p, const uint8_t *dsq, int L, const std::vector<EnvelopeResult> &res,
                              const std::vector<int> &req_index, DomainDefResult &dd,
                              const std::vector<EnvelopeResult> *res2, const std::vector<int> *req_index2)
{
  thread_local DomainWorkspace ws;
  std::vector<Domain> kept;
  kept.reserve(dd.dcl.size());
  // the device's answer for envelope i..j -> a Domain; null2_done: the region's ensemble already set dd.n2sc on i..j
  Model om_exact{ &p, p.M, {} };
  bool om_exact_ready = false;
  auto from_result = [&](const EnvelopeResult &r, int i, int j, bool null2_done, Domain &dom) -> bool {
    if (r.status & 2) return false;                  // p7_Decoding range error: the envelope is dropped
    if (r.status & 0xff & ~(3 | 64)) return false;   // traceback failure: upstream's rescore returns without a domain
    if (r.status & 64) {
      // a near-tie on the device's optimal-accuracy trace (p7x_envelope.hip, cfg.oa_guard): this envelope again with
      // the host twin, which performs the reference's operations in the reference's order
      if (!om_exact_ready) { om_exact.prepare(); om_exact.configure(false, L); om_exact_ready = true; }      // upstream's order (unless the test seam "host_order" asks for the device's)
      DomainDefResult one;
      one.n2sc.swap(dd.n2sc);
      const int st = rescore_isolated_domain(p, om_exact, dsq, L, i, j, null2_done, ws, one);
      dd.n2sc.swap(one.n2sc);
      dd.nneartie++;
      for (int b = 0; b < 8; ++b) if (r.status & (1 << (8 + b))) dd.neartie_why[b]++;
      if (st != P7X_OK || one.dcl.empty()) return false;
      dom = std::move(one.dcl[0]);
      return true;
    }
    Trace &tr = ws.tr;
    tr.clear();
    for (int z = 0; z < r.ntrace; ++z) tr.append((int) (r.ta[z] & 0xffu), (int) ((r.ta[z] >> 8) & 0xffffu), r.ti[z], r.tp[z]);
    tr.reverse();
    for (size_t z = 0; z < tr.st.size(); ++z) if (tr.i[z] > 0) tr.i[z] += i - 1;
    make_alidisplay(p, tr, dsq, L, dom);
    if (!null2_done) {
      float null2[MAXKP];
      for (int x = 0; x < p.K; ++x) null2[x] = r.null2[x];
      finish_null2(p, null2);
      float ln2[MAXKP];                                   // one logarithm per residue code, not per residue
      for (int x = 0; x < p.Kp; ++x) ln2[x] = logf(null2[x]);
      for (int pos = i; pos <= j; ++pos) dd.n2sc[pos] = ln2[dsq[pos]];
    }
    float domcorrection = 0.0f;
    for (int pos = i; pos <= j; ++pos) domcorrection += dd.n2sc[pos];
    dom.domcorrection = domcorrection;
    dom.ienv = i; dom.jenv = j; dom.envsc = r.envsc; dom.oasc = r.oasc;
    dom.iali = dom.sqfrom; dom.jali = dom.sqto;
    return true;
  };
  for (Domain &d : dd.dcl) {
    if (d.deferred == -2) {
      int last_j2 = 0;
      for (Domain &m : dd.multi[(size_t) d.multi_slot]) {
        if (m.deferred2 < 0 || !res2 || !req_index2) { kept.push_back(std::move(m)); continue; }
        const int i2 = (int) m.ienv, j2 = (int) m.jenv;
        if (i2 <= last_j2) dd.noverlaps++;
        Domain dom;
        if (from_result((*res2)[(size_t) (*req_index2)[(size_t) m.deferred2]], i2, j2, true, dom)) { last_j2 = j2; kept.push_back(std::move(dom)); }
      }
      continue;
    }
    if (d.deferred < 0) { kept.push_back(std::move(d)); continue; }
    Domain dom;
    if (from_result(res[(size_t) req_index[(size_t) d.deferred]], (int) d.ienv, (int) d.jenv, false, dom)) kept.push_back(std::move(dom));
  }
  dd.dcl = std::move(kept);
  return P7X_OK;
}

} // namespace p7x

// Test seam: one choice point through the integer thresholds of p7x_choice.hpp and through esl_rnd_FChoose as the
// reference writes it (floating-point test against roll = x / 2^32); x is the generator's state AFTER the draw.
extern "C" int p7x_debug_choice(const float *p, int n, uint32_t x, int *via_thresholds, int *via_fchoose)
{
  using namespace p7x;
  if (!p || n < 2 || n > 4 || !via_thresholds || !via_fchoose) return P7X_EINVAL;
  float a[4], b[4];
  for (int i = 0; i < n; ++i) a[i] = b[i] = p[i];
  uint32_t T[3] = { 0, 0, 0 }, fb = 0;
  choice_thresholds(a, n, T, &fb);
  *via_thresholds = choice_pick(T, fb, n, x);
  fnorm(b, n);
  FastRng r; r.x = x;
  const double roll = (double) x / 4294967296.0;
  const double norm = fsum(b, n);
  double sum = 0.0;
  int pick = -1;
  for (int i = 0; i < n && pick < 0; ++i) { sum += b[i]; if (roll < sum / norm) pick = i; }
  if (pick < 0) { pick = 0; for (int i = n - 1; i >= 0; --i) if (b[i] > 0.0f) { pick = i; break; } }
  *via_fchoose = pick;
  return P7X_OK;
}

// Calibration seam of the ensemble walk's near-threshold guard (p7x_ensemble.hip): the Forward matrix of region i..j of
// dsq1[1..L] in both summation orders -- the device's lane chunks and upstream's stripes -- and, for every cell, the integer
// thresholds of the three choice points a traceback can meet there (p7x_choice.hpp).  out[0] = thresholds compared,
// out[1] = the largest |T_lanes - T_upstream| / 2^32, out[2 + b] = how many differ by more than 2^-(24 - b), b = 0..9.
extern "C" int p7x_debug_order_spread(const p7x_oprofile *om, const uint8_t *dsq1, int32_t L, int32_t i, int32_t j, int multihit, double *out12)
{
  using namespace p7x;
  if (!om || !dsq1 || !out12 || i < 1 || j < i || j > L) { set_error("p7x_debug_order_spread: bad arguments"); return P7X_EINVAL; }
  const Profile &p = om->p;
  Model a{ &p, p.M, {} }, b{ &p, p.M, {} };
  a.prepare(1); b.prepare(0);
  a.configure(multihit != 0, L); b.configure(multihit != 0, L);
  Matrix fa, fb;
  const int Lr = j - i + 1, M = p.M;
  forward_full(a, dsq1 + i - 1, Lr, fa, nullptr);
  forward_full(b, dsq1 + i - 1, Lr, fb, nullptr);
  for (int q = 0; q < 12; ++q) out12[q] = 0.0;
  auto note = [&](uint32_t ta, uint32_t tb) {
    const double d = std::fabs((double) ta - (double) tb) / 4294967296.0;
    out12[0] += 1.0;
    if (d > out12[1]) out12[1] = d;
    for (int q = 0; q < 10; ++q) if (d > std::ldexp(1.0, -(24 - q))) out12[2 + q] += 1.0;
  };
  const float *bm = a.tf(0), *tMM = a.tf(1), *tIM = a.tf(2), *tDM = a.tf(3), *tMD = a.tf(4), *tMI = a.tf(5), *tII = a.tf(6), *tDD = a.tf(7);
  for (int r = 1; r <= Lr; ++r)
    for (int k = 1; k <= M; ++k) {
      uint32_t ca[4], cb[4], ta, tb, fa_, fb_;
      choice_cell_m(fa.X(r - 1, xB_) * bm[k], fa.M_(r - 1)[k - 1] * tMM[k], fa.I_(r - 1)[k - 1] * tIM[k], fa.D_(r - 1)[k - 1] * tDM[k], ca);
      choice_cell_m(fb.X(r - 1, xB_) * bm[k], fb.M_(r - 1)[k - 1] * tMM[k], fb.I_(r - 1)[k - 1] * tIM[k], fb.D_(r - 1)[k - 1] * tDM[k], cb);
      for (int q = 0; q < 3; ++q) note(ca[q], cb[q]);
      choice_pair(fa.M_(r - 1)[k] * tMI[k], fa.I_(r - 1)[k] * tII[k], &ta, &fa_);
      choice_pair(fb.M_(r - 1)[k] * tMI[k], fb.I_(r - 1)[k] * tII[k], &tb, &fb_);
      note(ta, tb);
      if (k > 1) {
        choice_pair(fa.M_(r)[k - 1] * tMD[k - 1], fa.D_(r)[k - 1] * tDD[k - 1], &ta, &fa_);
        choice_pair(fb.M_(r)[k - 1] * tMD[k - 1], fb.D_(r)[k - 1] * tDD[k - 1], &tb, &fb_);
        note(ta, tb);
      }
    }
  return P7X_OK;
}

// Test seam: the choice records of every cell and row of region i..j of dsq1[1..L] as the host twin forms them, in the
// summation order of the "host_order" option -- the operands of stochastic_trace()'s choices, in the layout and with the
// operations of ens_forward_kernel (p7x_choice.hpp).  cells: [(Lr + 1)][M + 1] records (row 0 and node 0 stay zero),
// rows: [Lr + 1]; md (may be NULL): [(Lr + 1)][M + 1][2], the scaled Forward values M(r, k), D(r, k) the E state chooses from.
namespace p7x {
int host_choice_records(const Profile &p, const uint8_t *dsq1, int L, int i, int j, ChoiceCell *cells, ChoiceRow *rows, float *md)
{
  Model om{ &p, p.M, {} };
  om.prepare();
  om.configure(true, L);
  Matrix fx;
  const int Lr = j - i + 1, M = p.M, Mrow = M + 1;
  forward_full(om, dsq1 + i - 1, Lr, fx, nullptr);
  std::memset(cells, 0, (size_t) (Lr + 1) * Mrow * sizeof(ChoiceCell));
  std::memset(rows, 0, (size_t) (Lr + 1) * sizeof(ChoiceRow));
  if (md) std::memset(md, 0, (size_t) (Lr + 1) * Mrow * 2 * sizeof(float));
  const float *bm = om.tf(0), *tMM = om.tf(1), *tIM = om.tf(2), *tDM = om.tf(3), *tMD = om.tf(4), *tMI = om.tf(5), *tII = om.tf(6), *tDD = om.tf(7);
  { uint32_t T, b; choice_pair(fx.X(0, xN_) * om.xf[XN][MOVE], fx.X(0, xJ_) * om.xf[XJ][MOVE], &T, &b); rows[0].x[2] = T; rows[0].x[3] = b << 4; }
  for (int r = 1; r <= Lr; ++r) {
    for (int k = 1; k <= M; ++k) {
      ChoiceCell &c = cells[(size_t) r * Mrow + k];
      uint32_t bi, bd;
      choice_cell_m(fx.X(r - 1, xB_) * bm[k], fx.M_(r - 1)[k - 1] * tMM[k], fx.I_(r - 1)[k - 1] * tIM[k], fx.D_(r - 1)[k - 1] * tDM[k], c.m);
      choice_pair(fx.M_(r - 1)[k] * tMI[k], fx.I_(r - 1)[k] * tII[k], &c.id[0], &bi);
      if (k > 1) choice_pair(fx.M_(r)[k - 1] * tMD[k - 1], fx.D_(r)[k - 1] * tDD[k - 1], &c.id[1], &bd);
      else       choice_pair(0.0f, 0.0f, &c.id[1], &bd);             // no node before the first: both weights are zero
      c.id[2] = bi | (bd << 2); c.id[3] = 0;
      if (md) { md[((size_t) r * Mrow + k) * 2] = fx.M_(r)[k]; md[((size_t) r * Mrow + k) * 2 + 1] = fx.D_(r)[k]; }
    }
    ChoiceRow &w = rows[r];
    uint32_t bc, bj, bb;
    choice_pair(fx.X(r - 1, xC_) * om.xf[XC][LOOP], fx.X(r, xE_) * om.xf[XE][MOVE] * fx.X(r, xS_), &w.x[0], &bc);
    choice_pair(fx.X(r - 1, xJ_) * om.xf[XJ][LOOP], fx.X(r, xE_) * om.xf[XE][LOOP] * fx.X(r, xS_), &w.x[1], &bj);
    choice_pair(fx.X(r, xN_) * om.xf[XN][MOVE], fx.X(r, xJ_) * om.xf[XJ][MOVE], &w.x[2], &bb);
    w.x[3] = bc | (bj << 2) | (bb << 4);
    const float norm = (float) (1.0 / fx.X(r, xE_));
    std::memcpy(&w.e[0], &norm, 4);
  }
  return P7X_OK;
}
} // namespace p7x

// Test seam: the 200 sampled paths of region i..j of dsq1[1..L] as the host twin walks them (in the "host_order" option's
// summation order), with the twin's ensemble in p7x_debug_ensemble's format.  Host code, no device.
extern "C" int p7x_debug_ensemble_traces(const p7x_oprofile *om, const uint8_t *dsq1, int32_t L, int32_t i, int32_t j, uint32_t seed,
                                         int8_t *st, int32_t *k, int32_t *pos, int64_t step_cap, int32_t *off201, int64_t *nsteps,
                                         int32_t *ndom, int32_t *dom, int32_t dom_cap, float *n2)
{
  using namespace p7x;
  if (!om || !dsq1 || !st || !k || !pos || !off201 || !nsteps || !ndom || !dom || !n2 || i < 1 || j < i || j > L || step_cap < 0 || dom_cap < 0) {
    set_error("p7x_debug_ensemble_traces: bad arguments"); return P7X_EINVAL;
  }
  EnsembleRaw raw;
  raw.want_traces = true;
  EnsembleResult e; e.status = -1; e.raw_out = &raw;
  DomainDefResult dd;
  dd.n2sc.assign((size_t) L + 1, 0.0f);
  std::vector<Domain> out;
  std::vector<EnvelopeRequest> defer2;
  MultiRegionState state;
  const int status = domaindef_multi_region(om->p, dsq1, L, i, j, seed, true, state, dd, out, &defer2, 0, &e);
  if (status != P7X_OK) return status;
  if (raw.off.size() != 200) { set_error("p7x_debug_ensemble_traces: the twin did not sample 200 paths"); return P7X_EINVAL; }
  raw.off.push_back((int32_t) raw.st.size());
  *nsteps = (int64_t) raw.st.size();
  std::memcpy(off201, raw.off.data(), 201 * sizeof(int32_t));
  const size_t n = (size_t) std::min<int64_t>(*nsteps, step_cap);
  std::memcpy(st, raw.st.data(), n); std::memcpy(k, raw.k.data(), n * 4); std::memcpy(pos, raw.i.data(), n * 4);
  *ndom = (int32_t) (raw.dom.size() / 5);
  std::memcpy(dom, raw.dom.data(), std::min(raw.dom.size(), (size_t) dom_cap * 5) * 4);
  std::memcpy(n2, raw.n2.data(), (size_t) (j - i + 2) * 4);
  return P7X_OK;
}


extern "C" int p7x_forward_parser_exact(const p7x_oprofile *om, const uint8_t *dsq, int32_t L, float *sc)
{
  using namespace p7x;
  if (!om || !sc || L < 0 || (L > 0 && !dsq)) { set_error("p7x_forward_parser_exact: bad arguments"); return P7X_EINVAL; }
  return host_forward_parser_exact(om->p, dsq, L, sc);
}

// Test seam of the rows-only engines in upstream's order: the parsers' special-state rows of dsq1[1..L] (multihit, length
// model of L) as the region-scan guard gets them (parser_rows_upstream), (L+1) x [E,N,J,B,C,SCALE] floats each.
extern "C" int p7x_debug_parser_rows(const p7x_oprofile *om, const uint8_t *dsq1, int32_t L, float *fx, float *bx)
{
  using namespace p7x;
  if (!om || !dsq1 || L < 1 || !fx || !bx) { set_error("p7x_debug_parser_rows: bad arguments"); return P7X_EINVAL; }
  std::vector<float> f, b;
  const int st = parser_rows_upstream(om->p, dsq1, L, f, b);
  if (st != P7X_OK) return st;
  std::memcpy(fx, f.data(), f.size() * sizeof(float));
  std::memcpy(bx, b.data(), b.size() * sizeof(float));
  return P7X_OK;
}

// Test seam of the bias filter's host twin (tests/test_host_bias_reference.py holds it to the float64 reference)
extern "C" int p7x_debug_bias_filter_host(const p7x_oprofile *om, const uint8_t *dsq1, int32_t L, float *sc)
{
  using namespace p7x;
  if (!om || !dsq1 || L < 0 || !sc) { set_error("p7x_debug_bias_filter_host: bad arguments"); return P7X_EINVAL; }
  for (int32_t i = 1; i <= L; ++i)
    if (dsq1[i] >= om->p.Kp) { set_error("p7x_debug_bias_filter_host: residue code out of range"); return P7X_EINVAL; }
  *sc = bias_filter_score(om->p, dsq1, L);
  return P7X_OK;
}

// Test seam of p7x_alidisplay_backconvert: the display make_alidisplay renders of a trace's first domain over dsq1[1..L], as the
// one domain of a one-hit list (which owns the strings)
extern "C" int p7x_debug_tophits_from_trace(const p7x_oprofile *om, const uint8_t *dsq1, int32_t L, int32_t N, const int8_t *st,
                                            const int32_t *k, const int32_t *i, const float *pp, const char *name, p7x_tophits **out)
{
  using namespace p7x;
  if (!om || !dsq1 || L < 1 || N < 3 || !st || !k || !i || !out) { set_error("p7x_debug_tophits_from_trace: bad arguments"); return P7X_EINVAL; }
  *out = nullptr;
  const Profile &p = om->p;
  Trace tr;
  int zb = -1, ze = -1;
  for (int z = 0; z < N; ++z) {
    const bool core = st[z] == sM || st[z] == sD || st[z] == sI, emits = st[z] == sM || st[z] == sI;
    if ((core && (k[z] < 1 || k[z] > p.M)) || (emits && (i[z] < 1 || i[z] > L || dsq1[i[z]] >= p.Kp))) { set_error("p7x_debug_tophits_from_trace: trace out of range"); return P7X_EINVAL; }
    if (st[z] == sB && zb < 0) zb = z;
    if (st[z] == sE && zb >= 0 && ze < 0) ze = z;
    tr.st.push_back(st[z]); tr.k.push_back(k[z]); tr.i.push_back(i[z]); tr.pp.push_back(pp ? pp[z] : 0.0f);
  }
  if (zb < 0 || ze < zb + 2) { set_error("p7x_debug_tophits_from_trace: the trace has no domain"); return P7X_EINVAL; }
  for (int z = zb + 1; z < ze; ++z)
    if (st[z] != sM && st[z] != sD && st[z] != sI) { set_error("p7x_debug_tophits_from_trace: the trace has no domain"); return P7X_EINVAL; }
  auto th = std::make_unique<p7x_tophits>();
  p7x_pipeline_cfg_default(&th->cfg);
  th->qname = p.name; th->qacc = p.acc; th->qdesc = p.desc; th->q_has_acc = p.has_acc; th->q_has_desc = p.has_desc;
  th->M = p.M; th->abc_type = p.abc_type;
  Hit hit;
  hit.name = name ? name : "";
  hit.ndom = 1;
  hit.dcl.resize(1);
  make_alidisplay(p, tr, dsq1, L, hit.dcl[0]);
  th->hits.push_back(std::move(hit));
  *out = th.release();
  return P7X_OK;
}
