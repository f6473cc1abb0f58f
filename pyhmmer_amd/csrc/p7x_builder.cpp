// p7x_builder.cpp -- a protein SEQUENCE as a query (phmmer): the single-sequence model and its E-value calibration.
//
// Host code, no device.  Restated from the published algorithms of HMMER 3 / Easel:
//   * the score system (p7_builder_LoadScoreSystem): BLOSUM62 turned into joint probabilities against the background
//     (esl_scorematrix_ProbifyGivenBG: lambda with sum f_a f_b exp(lambda s_ab) = 1), then into P(b | a) per query residue;
//   * the model (p7_Seqmodel / p7_SingleBuilder): one node per residue, match row = the conditional row of the residue,
//     inserts = background, gap-open / gap-extend transitions;
//   * the calibration (p7_Calibrate): the 600 random sequences every model is scored against (esl_rsq_xfIID on Easel's
//     generators) and the three fits (p7_Lambda, esl_gumbel_FitCompleteLoc, esl_gumbel_FitComplete + p7_Tau).
// The scores come from elsewhere: the device (p7x_calibrate.hip) or, in the CPU tests, the oracle.
#include "p7x_host.hpp"
#include "p7x_choice.hpp"
#include "p7x_rng.hpp"
#include <cmath>
#include <cstring>

namespace p7x {

// ---------------------------------------------------------------- BLOSUM62 (data), rows and columns in the order of kB62Order
static const char kB62Order[] = "ARNDCQEGHILKMFPSTWYV";
static const int8_t kB62[20][20] = {
  {  4, -1, -2, -2,  0, -1, -1,  0, -2, -1, -1, -1, -1, -2, -1,  1,  0, -3, -2,  0 },
  { -1,  5,  0, -2, -3,  1,  0, -2,  0, -3, -2,  2, -1, -3, -2, -1, -1, -3, -2, -3 },
  { -2,  0,  6,  1, -3,  0,  0,  0,  1, -3, -3,  0, -2, -3, -2,  1,  0, -4, -2, -3 },
  { -2, -2,  1,  6, -3,  0,  2, -1, -1, -3, -4, -1, -3, -3, -1,  0, -1, -4, -3, -3 },
  {  0, -3, -3, -3,  9, -3, -4, -3, -3, -1, -1, -3, -1, -2, -3, -1, -1, -2, -2, -1 },
  { -1,  1,  0,  0, -3,  5,  2, -2,  0, -3, -2,  1,  0, -3, -1,  0, -1, -2, -1, -2 },
  { -1,  0,  0,  2, -4,  2,  5, -2,  0, -3, -3,  1, -2, -3, -1,  0, -1, -3, -2, -2 },
  {  0, -2,  0, -1, -3, -2, -2,  6, -2, -4, -4, -2, -3, -3, -2,  0, -2, -2, -3, -3 },
  { -2,  0,  1, -1, -3,  0,  0, -2,  8, -3, -3, -1, -2, -1, -2, -1, -2, -2,  2, -3 },
  { -1, -3, -3, -3, -1, -3, -3, -4, -3,  4,  2, -3,  1,  0, -3, -2, -1, -3, -1,  3 },
  { -1, -2, -3, -4, -1, -2, -3, -4, -3,  2,  4, -2,  2,  0, -3, -2, -1, -2, -1,  1 },
  { -1,  2,  0, -1, -3,  1,  1, -2, -1, -3, -2,  5, -1, -3, -1,  0, -1, -3, -2, -2 },
  { -1, -1, -2, -3, -1,  0, -2, -3, -2,  1,  2, -1,  5,  0, -2, -1, -1, -1, -1,  1 },
  { -2, -3, -3, -3, -2, -3, -3, -3, -1,  0,  0, -3,  0,  6, -4, -2, -2,  1,  3, -1 },
  { -1, -2, -2, -1, -3, -1, -1, -2, -2, -3, -3, -1, -2, -4,  7, -1, -1, -4, -3, -2 },
  {  1, -1,  1,  0, -1,  0,  0,  0, -1, -2, -2,  0, -1, -2, -1,  4,  1, -3, -2, -2 },
  {  0, -1,  0, -1, -1, -1, -1, -2, -2, -1, -1, -1, -1, -2, -1,  1,  5, -2, -2,  0 },
  { -3, -3, -4, -4, -2, -2, -3, -2, -2, -3, -2, -3, -1,  1, -4, -3, -2, 11,  2, -3 },
  { -2, -2, -2, -3, -2, -1, -2, -3,  2, -1, -1, -2, -1,  3, -3, -2, -2,  2,  7, -1 },
  {  0, -3, -3, -3, -1, -2, -2, -3, -3,  3,  1, -2,  1, -1, -2, -2,  0, -3, -1,  4 },
};

// Joint probabilities Q[a][b] = f_a f_b exp(lambda s_ab) over the canonical residues, in the alphabet's own order.
static int probify_blosum62(const Alphabet &abc, const float *bg_f, double Q[MAXK][MAXK])
{
  int pos[MAXK];
  for (int a = 0; a < 20; ++a) {
    const char *at = std::strchr(kB62Order, abc.sym[a]);
    if (!at) { set_error("the alphabet has a residue BLOSUM62 does not score"); return P7X_EINVAL; }
    pos[a] = (int) (at - kB62Order);
  }
  double f[MAXK];
  int s[MAXK][MAXK], smax = 0;
  for (int a = 0; a < 20; ++a) {
    f[a] = (double) bg_f[a];
    for (int b = 0; b < 20; ++b) { s[a][b] = kB62[pos[a]][pos[b]]; smax = std::max(smax, s[a][b]); }
  }
  auto fdf = [&](double lam, double *fx, double *dfx) {
    double v = 0.0, d = 0.0;
    for (int a = 0; a < 20; ++a)
      for (int b = 0; b < 20; ++b) { const double e = f[a] * f[b] * std::exp(lam * (double) s[a][b]); v += e; d += e * (double) s[a][b]; }
    *fx = v - 1.0; *dfx = d;
  };
  // f(0) = 0 too: bracket the positive root from the right (f > 0), then Newton-Raphson
  double lam = 1.0 / (double) smax, fx = 0.0, dfx = 0.0;
  for (; lam < 50.0; lam *= 2.0) { fdf(lam, &fx, &dfx); if (fx > 0.0) break; }
  if (!(fx > 0.0)) { set_error("no lambda for the score matrix against this background"); return P7X_EINVAL; }
  for (int it = 0; it < 100; ++it) {
    fdf(lam, &fx, &dfx);
    const double next = lam - fx / dfx;
    const bool done = std::fabs(next - lam) <= 1e-15 * std::fabs(next) || fx == 0.0;
    lam = next;
    if (done) break;
  }
  for (int a = 0; a < 20; ++a)
    for (int b = 0; b < 20; ++b) Q[a][b] = f[a] * f[b] * std::exp(lam * (double) s[a][b]);
  return P7X_OK;
}

// p7_MeanMatchRelativeEntropy times M: the sum over the nodes of esl_vec_FRelEntropy(mat[k], bg) (bits; float sums)
double match_relent_sum(const float *mat, const float *bg_f, int M, int K)
{
  double tot = 0.0;
  for (int k = 1; k <= M; ++k) {
    const float *p = mat + (size_t) k * K;
    float kl = 0.0f;
    for (int x = 0; x < K; ++x)
      if (p[x] > 0.0f) kl += p[x] * std::log(p[x] / bg_f[x]);
    tot += (float) (1.44269504 * kl);
  }
  return tot;
}

// esl_rnd_FChoose: the first residue whose cumulative probability exceeds the deviate -- the sums in double over the
// Kahan-summed norm, the last residue of positive probability when rounding leaves every ratio below it (the same
// function the stochastic tracebacks draw with: p7x_choice.hpp)
static int fchoose(EaselRng &r, const float *p, int K)
{
  const double roll = r.next();
  float fs = 0.0f, c = 0.0f;
  for (int i = 0; i < K; ++i) { const float y = p[i] - c; const float t = fs + y; c = (t - fs) - y; fs = t; }
  const double norm = (double) fs;
  double sum = 0.0;
  int last = 0;
  for (int i = 0; i < K; ++i) {
    sum += (double) p[i];
    if (p[i] > 0.0f) last = i;
    if (roll < sum / norm) return i;
  }
  return last;
}

static const int kCalN = P7X_CAL_N;
static const int kCalL[3] = { 200, 200, 100 };       // p7_Calibrate's EmL, EvL, EfL

// One sample of L residues (esl_rsq_xfIID)
static void draw_sample(EaselRng &r, const float *bg_f, int K, int L, uint8_t *out)
{
  for (int i = 0; i < L; ++i) out[i] = (uint8_t) fchoose(r, bg_f, K);
}

// ---------------------------------------------------------------- the fits (Easel esl_gumbel.c; doubles)
static double gumbel_fit_loc(const double *x, int n, double lambda)
{
  double esum = 0.0;
  for (int i = 0; i < n; ++i) esum += std::exp(-lambda * x[i]);
  return -std::log(esum / (double) n) / lambda;
}

static void lawless416(const double *x, int n, double lambda, double *f, double *df)
{
  double esum = 0.0, xesum = 0.0, xxesum = 0.0, xsum = 0.0;
  for (int i = 0; i < n; ++i) {
    const double e = std::exp(-lambda * x[i]);
    xsum += x[i]; xesum += x[i] * e; xxesum += x[i] * x[i] * e; esum += e;
  }
  *f = (1.0 / lambda) - (xsum / (double) n) + (xesum / esum);
  *df = ((xesum / esum) * (xesum / esum)) - (xxesum / esum) - (1.0 / (lambda * lambda));
}

static int gumbel_fit_complete(const double *x, int n, double *mu, double *lambda)
{
  double sum = 0.0, sqsum = 0.0;
  for (int i = 0; i < n; ++i) { sum += x[i]; sqsum += x[i] * x[i]; }
  const double var = (sqsum - sum * sum / (double) n) / ((double) n - 1.0);
  if (!(var > 0.0)) return P7X_ENORESULT;
  double lam = 3.14159265358979323846 / std::sqrt(6.0 * var), fx = 0.0, dfx = 0.0;
  const double tol = 1e-5;
  int it = 0;
  for (; it < 100; ++it) {
    lawless416(x, n, lam, &fx, &dfx);
    if (std::fabs(fx) < tol) break;
    lam = lam - fx / dfx;
    if (lam <= 0.0) lam = 0.001;
  }
  if (it == 100) {       // Newton-Raphson failed: bracket the root and bisect
    double left = 0.0, right = 3.14159265358979323846 / std::sqrt(6.0 * var);
    lawless416(x, n, right, &fx, &dfx);
    while (fx > 0.0) { right *= 2.0; if (right > 1000.0) return P7X_ENORESULT; lawless416(x, n, right, &fx, &dfx); }
    for (it = 0; it < 100; ++it) {
      const double mid = (left + right) / 2.0;
      lawless416(x, n, mid, &fx, &dfx);
      if (std::fabs(fx) < tol) { lam = mid; break; }
      if (fx > 0.0) left = mid; else right = mid;
      lam = mid;
    }
  }
  *lambda = lam;
  *mu = gumbel_fit_loc(x, n, lam);
  return P7X_OK;
}

} // namespace p7x

using namespace p7x;

extern "C" {

int p7x_builder_single(int32_t abc_type, const uint8_t *dsq, int32_t L, const float *bg_f, const char *score_matrix,
                       double popen, double pextend, float *t, float *mat, float *ins)
{
  if (!dsq || !bg_f || !t || !mat || !ins || L < 1) { set_error("p7x_builder_single: bad arguments"); return P7X_EINVAL; }
  if (abc_type != P7X_AMINO) { set_error("single-sequence models are built for the amino alphabet only"); return P7X_EINVAL; }
  if (!score_matrix || std::strcmp(score_matrix, "BLOSUM62") != 0) { set_error("the only score matrix is BLOSUM62"); return P7X_EINVAL; }
  if (!(popen >= 0.0 && popen < 0.5) || !(pextend >= 0.0 && pextend < 1.0)) { set_error("popen must lie in [0, 0.5) and pextend in [0, 1)"); return P7X_EINVAL; }
  const Alphabet &abc = Alphabet::get(abc_type);
  const int K = abc.K;
  double Q[MAXK][MAXK];
  const int st = probify_blosum62(abc, bg_f, Q);
  if (st != P7X_OK) return st;
  // P(b | a): the joint row of the query residue over its own sum; a degenerate residue stands for the sum of the joint rows
  // of its residues (the degenerate rows of the joint matrix), normalised the same way
  for (int k = 0; k <= L; ++k) {
    float *m = mat + (size_t) k * K, *tk = t + (size_t) k * 7;
    if (k == 0) { for (int b = 0; b < K; ++b) m[b] = 0.0f; m[0] = 1.0f; }
    else {
      const int x = dsq[k - 1];
      if (x >= abc.Kp - 2 || x == K) { set_error("the query holds a gap or a missing-data symbol at residue " + std::to_string(k)); return P7X_EINVAL; }
      double row[MAXK], tot = 0.0;
      for (int b = 0; b < K; ++b) {
        double v = 0.0;
        if (x < K) v = Q[x][b];
        else for (int a = 0; a < K; ++a) if (abc.degen[x][a]) v += Q[a][b];
        row[b] = v; tot += v;
      }
      if (!(tot > 0.0)) { set_error("a query residue stands for no canonical residue"); return P7X_EINVAL; }
      for (int b = 0; b < K; ++b) m[b] = (float) (row[b] / tot);
    }
    std::memcpy(ins + (size_t) k * K, bg_f, sizeof(float) * K);
    tk[0] = (float) (1.0 - 2.0 * popen); tk[1] = (float) popen; tk[2] = (float) popen;      // MM MI MD
    tk[3] = (float) (1.0 - pextend); tk[4] = (float) pextend;                              // IM II
    tk[5] = (float) (1.0 - pextend); tk[6] = (float) pextend;                              // DM DD
  }
  float *tm = t + (size_t) L * 7;               // the last node: no M->D, D->M = 1
  tm[0] = (float) (1.0 - popen); tm[2] = 0.0f; tm[5] = 1.0f; tm[6] = 0.0f;
  return P7X_OK;
}

int p7x_calibration_stream(int32_t abc_type, const float *bg_f, uint32_t seed, int generator, uint8_t *out)
{
  if (!bg_f || !out) { set_error("p7x_calibration_stream: bad arguments"); return P7X_EINVAL; }
  if (abc_type != P7X_AMINO && abc_type != P7X_DNA && abc_type != P7X_RNA) { set_error("unknown alphabet"); return P7X_EINVAL; }
  if (generator != P7X_RNG_MERSENNE && generator != P7X_RNG_FAST) { set_error("unknown generator"); return P7X_EINVAL; }
  const int K = Alphabet::get(abc_type).K;
  EaselRng r;
  r.init(generator, seed);
  for (int stage = 0; stage < 3; ++stage)
    for (int i = 0; i < kCalN; ++i) { draw_sample(r, bg_f, K, kCalL[stage], out); out += kCalL[stage]; }
  return P7X_OK;
}

int p7x_rng_seed(int generator, uint32_t seed, uint32_t *state)
{
  if (!state) { set_error("p7x_rng_seed: bad arguments"); return P7X_EINVAL; }
  if (generator != P7X_RNG_MERSENNE && generator != P7X_RNG_FAST) { set_error("unknown generator"); return P7X_EINVAL; }
  EaselRng r;
  r.init(generator, seed);
  r.save(state);
  return P7X_OK;
}

int p7x_rng_draw(int generator, uint32_t *state, size_t n, double *out)
{
  if (!state || (n && !out)) { set_error("p7x_rng_draw: bad arguments"); return P7X_EINVAL; }
  if (generator != P7X_RNG_MERSENNE && generator != P7X_RNG_FAST) { set_error("unknown generator"); return P7X_EINVAL; }
  EaselRng r;
  r.load(generator, state);
  for (size_t i = 0; i < n; ++i) out[i] = r.next();
  r.save(state);
  return P7X_OK;
}

int p7x_calibration_redraw(int32_t abc_type, const float *bg_f, uint32_t seed, int generator, const int32_t *skipped,
                           int nskipped, uint8_t *out)
{
  if (!bg_f || !out || nskipped < 0 || (nskipped > 0 && !skipped)) { set_error("p7x_calibration_redraw: bad arguments"); return P7X_EINVAL; }
  if (abc_type != P7X_AMINO && abc_type != P7X_DNA && abc_type != P7X_RNA) { set_error("unknown alphabet"); return P7X_EINVAL; }
  if (generator != P7X_RNG_MERSENNE && generator != P7X_RNG_FAST) { set_error("unknown generator"); return P7X_EINVAL; }
  const int K = Alphabet::get(abc_type).K;
  EaselRng r;
  r.init(generator, seed);
  int draw = 0, s = 0;                           // draws made so far (kept or not); next entry of <skipped>
  uint8_t scratch[256];
  for (int stage = 0; stage < 3; ++stage)
    for (int i = 0; i < kCalN; ++draw) {
      if (s < nskipped && skipped[s] < draw) { set_error("p7x_calibration_redraw: skipped draws must be increasing"); return P7X_EINVAL; }
      if (s < nskipped && skipped[s] == draw) {
        if (stage == 2) { set_error("p7x_calibration_redraw: a Forward sample cannot overflow"); return P7X_EINVAL; }
        draw_sample(r, bg_f, K, kCalL[stage], scratch); ++s; continue;
      }
      draw_sample(r, bg_f, K, kCalL[stage], out); out += kCalL[stage]; ++i;
    }
  return P7X_OK;
}

int32_t p7x_calibration_draw_of(int32_t kept, const int32_t *skipped, int nskipped)
{
  int32_t draw = kept;
  for (int i = 0; i < nskipped; ++i) if (skipped[i] <= draw) ++draw;
  return draw;
}

int p7x_calibration_fit(const float *sc, const uint8_t *overflow, double mh, float *out_evparam)
{
  if (!sc || !out_evparam || !(mh > 0.0)) { set_error("p7x_calibration_fit: bad arguments"); return P7X_EINVAL; }
  int first = -1;
  if (overflow)
    for (int i = 0; i < 2 * kCalN && first < 0; ++i) if (overflow[i]) first = i;
  if (first >= 0) {
    set_error("calibration sample " + std::to_string(first) + " overflowed its filter: upstream draws it again, which moves every later sample");
    return P7X_ERANGE;
  }
  const double lambda = kLog2 + 1.44 / mh;         // p7_Lambda: M H = the summed match relative entropy
  double x[3][P7X_CAL_N];
  for (int stage = 0; stage < 3; ++stage) {
    const float nullsc = null1_score(kCalL[stage]);
    for (int i = 0; i < kCalN; ++i) {
      const float v = sc[stage * kCalN + i];
      if (!std::isfinite(v)) { set_error("a calibration score is not finite"); return P7X_ERANGE; }
      x[stage][i] = (double) (v - nullsc) / kLog2;
    }
  }
  const double mmu = gumbel_fit_loc(x[0], kCalN, lambda), vmu = gumbel_fit_loc(x[1], kCalN, lambda);
  double gmu = 0.0, glam = 0.0;
  const int st = gumbel_fit_complete(x[2], kCalN, &gmu, &glam);
  if (st != P7X_OK) { set_error("no Gumbel fit to the Forward scores"); return st; }
  const double tailp = 0.04;                       // p7_Tau: where the Gumbel's tail holds <tailp>, moved back to mass 1
  const double tau = (gmu - std::log(-1.0 * std::log(1.0 - tailp)) / glam) + std::log(tailp) / lambda;
  out_evparam[P7X_MMU] = (float) mmu; out_evparam[P7X_MLAMBDA] = (float) lambda;
  out_evparam[P7X_VMU] = (float) vmu; out_evparam[P7X_VLAMBDA] = (float) lambda;
  out_evparam[P7X_FTAU] = (float) tau; out_evparam[P7X_FLAMBDA] = (float) lambda;
  return P7X_OK;
}

int p7x_calibration_scores(const p7x_oprofile *om, const int32_t *xJ, const int32_t *xC, float *sc, uint8_t *overflow)
{
  if (!om || !xJ || !xC || !sc || !overflow) { set_error("p7x_calibration_scores: bad arguments"); return P7X_EINVAL; }
  const Profile &p = om->p;
  const uint8_t tjb = tjb_of(p.scale_b, kCalL[0]);
  const int16_t xwm = xw_move_of(p.scale_w, kCalL[1]);
  for (int i = 0; i < kCalN; ++i) {      // (an overflowed sample's score is +inf; p7x_calibration_fit stops at its mark)
    overflow[i] = xJ[i] < 0;
    sc[i] = msv_score_nats(xJ[i], tjb, p.base_b, p.scale_b);
    overflow[kCalN + i] = xC[i] >= 32767;
    sc[kCalN + i] = vit_score_nats(xC[i], xwm, p.base_w, p.scale_w);
  }
  return P7X_OK;
}

int p7x_debug_score_units(const p7x_oprofile *om, const int32_t *L, size_t nL, int32_t *tjb, int32_t *xw_move, const int32_t *xJ, size_t nJ, const int32_t *xC, size_t nC, float *usc, float *vfsc)
{
  if (!om || !L || !tjb || !xw_move || (nJ && (!xJ || !usc)) || (nC && (!xC || !vfsc))) { set_error("p7x_debug_score_units: bad arguments"); return P7X_EINVAL; }
  const Profile &p = om->p;
  for (size_t l = 0; l < nL; ++l) {
    tjb[l] = tjb_of(p.scale_b, L[l]); xw_move[l] = xw_move_of(p.scale_w, L[l]);
    for (size_t i = 0; i < nJ; ++i) usc[l * nJ + i] = msv_score_nats(xJ[i], tjb[l], p.base_b, p.scale_b);
    for (size_t i = 0; i < nC; ++i) vfsc[l * nC + i] = vit_score_nats(xC[i], xw_move[l], p.base_w, p.scale_w);
  }
  return P7X_OK;
}

double p7x_oprofile_match_relent(const p7x_oprofile *om) { return om ? om->p.relent_mh : 0.0; }

} // extern "C"
