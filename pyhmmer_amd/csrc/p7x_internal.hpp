// p7x_internal.hpp -- shared declarations of libp7x (product code; never includes oracle/).
#pragma once
#include "../../include/p7x.h"
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

// functions that device code calls as well: nothing under a plain C++ compiler
#if defined(__HIPCC__)
#define P7X_HD __host__ __device__
#else
#define P7X_HD
#endif

namespace p7x {

constexpr int MAXK  = 20;
constexpr int MAXKP = 29;
constexpr double kLog2  = 0.69314718055994529;
constexpr double kLog2R = 1.44269504088896341;

// special-state / transition indices, same numbering as impl_sse/p7_oprofile.pxd:29-49
enum { XE = 0, XN = 1, XJ = 2, XC = 3 };
enum { MOVE = 0, LOOP = 1 };
enum { tBM = 0, tMM, tIM, tDM, tMD, tMI, tII, tDD, NTRANS };
// generic profile transition order (upstream p7_profile.h)
enum { gMM = 0, gIM, gDM, gBM, gMD, gDD, gMI, gII };

struct Alphabet {
  int type, K, Kp;
  const char *sym;
  unsigned char degen[MAXKP][MAXK];
  static const Alphabet &get(int type);
};

// Everything the path needs about one query, stored UN-striped: index k = 1..M is the node.
// Transition tables follow the oprofile convention (impl_sse/p7_oprofile.pxd:41-49):
//   tw/tf[tBM|tMM|tIM|tDM][k] = score of entering node k (from B / M,I,D of node k-1)
//   tw/tf[tMD|tMI|tII|tDD][k] = score of leaving node k.
struct Profile {
  int M = 0, K = 0, Kp = 0, abc_type = 0, L = 0, max_length = -1, mode = 0;
  float nj = 1.0f;
  double relent_mh = 0.0;        // M x mean match relative entropy of the core model (bits): p7_Lambda at calibration; 0 = not known
  std::string name, acc, desc, consensus, rf, mm, cs;
  bool has_acc = false, has_desc = false;
  float evparam[6], cutoff[6], compo[MAXK], bgf[MAXK];
  // generic log-odds profile (p7_ProfileConfig)
  std::vector<float> tsc;        // [(M+1)*8] generic order gMM..gII
  std::vector<float> msc;        // [Kp][M+1]
  float xsc[4][2];
  // MSV (mf_conversion)
  std::vector<uint8_t> rb;       // [Kp][M+1] biased costs, rb[x][0] unused (255)
  uint8_t tbm_b, tec_b, tjb_b, base_b, bias_b;
  float scale_b;
  // Viterbi (vf_conversion)
  std::vector<int16_t> rw;       // [Kp][M+1]
  std::vector<int16_t> tw;       // [NTRANS][M+1]
  int16_t xw[4][2];
  float scale_w; int16_t base_w, ddbound_w; float ncj_roundoff;
  // Forward/Backward (fb_conversion): odds ratios / probabilities
  std::vector<float> rf_;        // [Kp][M+1]
  std::vector<float> tf;         // [NTRANS][M+1]
  float xf[4][2];

  int Q16() const { int q = (M - 1) / 16 + 1; return q < 2 ? 2 : q; }
  int Q8()  const { int q = (M - 1) / 8  + 1; return q < 2 ? 2 : q; }
  int Q4()  const { int q = (M - 1) / 4  + 1; return q < 2 ? 2 : q; }
};

// host math shared by the pipeline (p7x_stats.cpp)
float  sse_expf(float x);                               // Easel esl_sse_expf, one lane
uint8_t unbiased_byteify(float scale_b, float sc);
int16_t wordify(float scale_w, float sc);

// ---- the length model and the score units of the integer filters, each written once (host and device code)
// multihit move probability of N / C / J for a target of L residues, 3 / (L + 3), in upstream's spelling with nj = 1
// (p7_oprofile_ReconfigRestLength, p7_ReconfigLength)
P7X_HD inline float length_pmove(float L) { return (2.0f + 1.0f) / (L + 2.0f + 1.0f); }
// its cost in the MSV filter's bytes (p7_oprofile_ReconfigMSVLength) and the Viterbi filter's words
inline uint8_t tjb_of(float scale_b, int64_t L) { return unbiased_byteify(scale_b, logf(length_pmove((float) L))); }
inline int16_t xw_move_of(float scale_w, int64_t L) { return wordify(scale_w, logf(length_pmove((float) L))); }
// xJ of the MSV filter (negative: it overflowed) -> nats, p7_MSVFilter's last lines.  The quotient is a float below 2^17 in
// magnitude: upstream's subtraction of 3.0 in double is exact and rounds once, to the float that a float subtraction gives.
P7X_HD inline float msv_score_nats(int xJ, int tjb, int base_b, float scale_b)
{
  if (xJ < 0) return __builtin_inff();
  float sc = ((float) (xJ - tjb) - (float) base_b);
  sc /= scale_b;
  sc -= 3.0;
  return sc;
}
// xC of the Viterbi filter (32767: overflow, -32768: no path) -> nats, p7_ViterbiFilter's last lines
P7X_HD inline float vit_score_nats(int xC, int xw_move, int base_w, float scale_w)
{
  if (xC >= 32767) return __builtin_inff();
  if (xC <= -32768) return -__builtin_inff();
  float sc = (float) xC + (float) xw_move - (float) base_w;
  sc /= scale_w;
  sc -= 3.0;
  return sc;
}

double gumbel_surv(double x, double mu, double lambda);
double exp_surv(double x, double mu, double lambda);
double exp_logsurv(double x, double mu, double lambda);
float  null1_score(int L);
double match_relent_sum(const float *mat, const float *bg_f, int M, int K);      // p7x_builder.cpp
void   flogsum_init();
float  flogsum(float a, float b);

void set_error(const std::string &msg);

// Test / diagnostic seam (p7x_debug_set_option, include/p7x.h): process-wide knobs that pick a kernel family for a parity test, bound
// a workspace, or switch a trace on.  -1 = not set (the library decides).  The library reads no environment variables.
enum { OPT_SMALL_BLOCK = 0, OPT_VIT_WAVE, OPT_MSV_EXACT, OPT_MSV_LONG_GROUPS, OPT_MSV_BLOCKS_PER_CU, OPT_ENV_WORKSPACE_GB, OPT_DEVICE_CLUSTERED,
       OPT_TRACE_FINISH, OPT_TRACE_LONGTARGET, OPT_TRACE_ENVELOPE, OPT_HOST_PROFILE, OPT_SSV_KERNEL, OPT_MSV_F16, OPT_ENS_LDS_KB, OPT_ENS_FAIL, OPT_MSV_TIERS, OPT_STAGE_MERGE, OPT_EARLY_PACK, OPT_HOST_ORDER, OPT_VIT_LONG_CUT, OPT_FWD_GROUPED, OPT_REGION_GUARD_PPM, OPT_MSV_K8, OPT_MSV_LANE_BLOCKS, OPT_HOST_ALIGN, OPT_ALIGN_WORKSPACE_GB, OPT_CASCADE_STREAMS, OPT_CASCADE_SPLIT, OPT_SSV_PARTS, OPT_ALIGN_LOGSPACE, OPT_VIT_WIDE, OPT_HOST_EMIT, OPT_EMIT_CAP, OPT_EMIT_LDS, OPT_HOST_BUILD, OPT_BUILD_ROWS, OPT_HOST_PAIRID, OPT_PAIRID_TILE, OPT_MSA_CODES, OPT_HOST_TRANSLATE, OPT_ORF_CHUNK, OPT_ENV_BLOCKS, OPT_SSV_SCAN_CHUNK, OPT_HOST_SHUFFLE, OPT_SHUFFLE_SLAB, OPT_COUNT };
int debug_opt(int which);

}
struct p7x_oprofile;
namespace p7x {
void attach_dev_cache(p7x_oprofile *om);

} // namespace p7x

struct p7x_oprofile { p7x::Profile p; void *dev_cache = nullptr; };
