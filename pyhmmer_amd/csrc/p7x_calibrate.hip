// p7x_calibrate.hip -- p7_Calibrate for a batch of query profiles: the E-value parameters of sequence queries (phmmer).
//
// Every model is scored against the same 600 random sequences (200 of 200 residues through the MSV filter, 200 of 200
// through the Viterbi filter, 200 of 100 through the Forward parser: p7x_builder.cpp draws them), which are generated once
// per device and stay resident.  One wavefront scores one (model, sample) with the wave-per-target layout of
// p7x_vitfwd.hip -- lane z owns nodes zC+1 .. zC+C, tables [c*64 + lane] from the profile's device image -- but with
// everything a calibration fixes folded in: the targets have one length per stage, so the length models are three constants
// computed on the host (no length tables, no work lists, no slot arrays), a block's four wavefronts are four consecutive
// samples, and only the emission rows of the canonical residues are staged in LDS (a random sequence holds nothing else).
// blockIdx.y is the model; the models of a launch share their tier of nodes per lane (P7X_NODE_TIERS).  The three stages
// are three launches per tier on one stream; the host waits once, for the copy of the raw results, and does the fits.
// Integer results are those of vit_kernel / msv_wave_kernel bit for bit (same operations in the same order); the Forward
// score is fwd_kernel's (same summation order).
#include "p7x_wave.hpp"
#include "p7x_launch.hpp"
#include "p7x_host.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>

namespace p7x {

constexpr int kCalN = P7X_CAL_N;
constexpr int kCalLmsv = 200, kCalLvit = 200, kCalLfwd = 100;
constexpr int kCalOffVit = kCalN * kCalLmsv, kCalOffFwd = kCalOffVit + kCalN * kCalLvit;
static_assert(kCalOffFwd + kCalN * kCalLfwd == P7X_CAL_RESIDUES, "the stream's layout");
static_assert(kCalN % (kWsBlock / 64) == 0, "a block's wavefronts are samples of one stage");

struct CalArgs {
  int M, C, K;                      // K: emission rows staged (the canonical residues)
  const void *msv_emis;             // int16 [.][Mpad] bias - cost
  const void *vit_trans, *vit_emis; // uint4 [Mpad]; int16 [.][Mpad]
  const void *fwd_trans, *fwd_emis; // float4 [2 Mpad]; float [.][Mpad]
  int base_b, bias_b, tec_b, tjbm;  // MSV; tjbm = tjb(L = 200) + tbm
  int xwm, base_w, xw_e, ddbound;   // Viterbi; xwm = the N/C/J move score of L = 200
  float xf_e_move, xf_e_loop;       // Forward
  int32_t *out;                     // [3][kCalN]: xJ (-1 overflow), xC (32767 overflow), Forward score (float bits)
};

// the residues of a block's sample: its wavefront's number inside the stage, and where the sample starts
__device__ __forceinline__ int cal_sample() { return rfl((int) (blockIdx.x * (kWsBlock / 64) + (threadIdx.x >> 6))); }

// ======================================================================================= MSV
// Row body: the twin of msv_wave_kernel's kBlk == 1 path (p7x_vitfwd.hip).  A fix there belongs here too;
// tests/test_gpu_calibrate.py::test_raw_scores_against_the_oracle_and_the_cascade_kernels ties the two bit for bit.
template <int C>
__global__ void __launch_bounds__(kWsBlock) cal_msv_kernel(const ArgRef ref, const uint8_t *__restrict__ stream)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int Mpad = 64 * C;
  constexpr bool EG = C > 32;         // M > 2048: the table is read where it lies (L2)
  const CalArgs a = load_args<CalArgs>(ref);
  const short *em = EG ? reinterpret_cast<const short *>(a.msv_emis) : reinterpret_cast<const short *>(smem);
  if constexpr (!EG) {
    const uint4 *ge = reinterpret_cast<const uint4 *>(a.msv_emis);
    uint4 *le = reinterpret_cast<uint4 *>(smem);
    for (int i = threadIdx.x; i < a.K * Mpad / 8; i += kWsBlock) le[i] = ge[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int s = cal_sample();
  const uint8_t *sq = stream + (size_t) s * kCalLmsv;
  constexpr int L = kCalLmsv;
  int mm[C];
#pragma unroll unroll_c(C)
  for (int c = 0; c < C; ++c) mm[c] = 0;
  int xJ = 0, xEmax = 0;
  int xB = max(a.base_b - a.tjbm, 0);
  for (int i0 = 0; i0 < L; i0 += 64) {
    const int nrow = min(64, L - i0);
    const uint32_t resid = (lane < nrow) ? sq[i0 + lane] : 0;
    for (int r = 0; r < nrow; ++r) {
      const int x = __builtin_amdgcn_readlane((int) resid, r);
      const short *er = em + x * Mpad + lane;
      int mp = dpp_shr1(mm[C - 1], 0);
      int rowmax = kNegPad;
#pragma unroll unroll_c(C)
      for (int c = 0; c < C; ++c) {
        const int sv = max(mp, xB) + (int) er[c * 64];
        mp = mm[c];
        mm[c] = sv;
        rowmax = max(rowmax, sv);
      }
      const int xE = wave_max_i32(rowmax);
      xEmax = max(xEmax, xE);
      xJ = max(xJ, xE - a.tec_b);
      xB = max(max(a.base_b, xJ) - a.tjbm, 0);
    }
  }
  if (lane == 0) a.out[s] = (xEmax >= 255 - a.bias_b) ? -1 : xJ;
}

// ======================================================================================= Viterbi filter
// Row body: the twin of vit_kernel (p7x_vitfwd.hip) without its long-target branch; tied to it bit for bit by the same test.
template <int C>
__global__ void __launch_bounds__(kWsBlock) cal_vit_kernel(const ArgRef ref, const uint8_t *__restrict__ stream)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int Mpad = 64 * C;
  constexpr bool EG = C > 32;         // M > 2048: only the transitions are staged
  constexpr bool TG = C > 128;        // M > 8192: the transitions are read through L2 as well (as vit_kernel)
  static_assert(!TG || EG, "transitions through L2 only where the emissions are");
  const CalArgs a = load_args<CalArgs>(ref);
  const uint4 *tr = TG ? reinterpret_cast<const uint4 *>(a.vit_trans) : reinterpret_cast<const uint4 *>(smem);      // [Mpad]
  const short *em = EG ? reinterpret_cast<const short *>(a.vit_emis) : reinterpret_cast<const short *>(smem + (size_t) Mpad * 16);
  {
    if constexpr (!TG) {
      const uint4 *gt = reinterpret_cast<const uint4 *>(a.vit_trans);
      uint4 *lt = reinterpret_cast<uint4 *>(smem);
      for (int i = threadIdx.x; i < Mpad; i += kWsBlock) lt[i] = gt[i];
    }
    if constexpr (!EG) {
      const uint4 *ge = reinterpret_cast<const uint4 *>(a.vit_emis);
      uint4 *le = reinterpret_cast<uint4 *>(smem + (size_t) Mpad * 16);
      for (int i = threadIdx.x; i < a.K * Mpad / 8; i += kWsBlock) le[i] = ge[i];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const short NEG = (short) -32768;
  const int s = cal_sample();
  const uint8_t *sq = stream + kCalOffVit + (size_t) s * kCalLvit;
  constexpr int L = kCalLvit;
  const int xwm = a.xwm;

  short mm[C], im[C], dm[C], tdd[C];
#pragma unroll unroll_c(C)
  for (int c = 0; c < C; ++c) { mm[c] = im[c] = dm[c] = NEG; tdd[c] = NEG; }
  int xN = a.base_w, xB = xN + xwm, xJ = -32768, xC = -32768;
  bool overflow = false;
  for (int i0 = 0; i0 < L && !overflow; i0 += 64) {
    const int nrow = min(64, L - i0);
    const uint32_t resid = (lane < nrow) ? sq[i0 + lane] : 0;
    for (int r = 0; r < nrow && !overflow; ++r) {
      const int x = __builtin_amdgcn_readlane((int) resid, r);
      const short *er = em + x * Mpad + lane;
      const short xBs = (short) xB;
      short mp = (short) dpp_shr1(mm[C - 1], NEG);
      short ip = (short) dpp_shr1(im[C - 1], NEG);
      short dp = (short) dpp_shr1(dm[C - 1], NEG);
      short rowmax = NEG, dmax = NEG, dcarry = NEG;
#pragma unroll unroll_c(C)
      for (int c = 0; c < C; ++c) {
        const uint4 t = tr[c * 64 + lane];
        short sv = adds16(xBs, lo16(t.x));
        sv = max16(sv, adds16(mp, hi16(t.x)));
        sv = max16(sv, adds16(ip, lo16(t.y)));
        sv = max16(sv, adds16(dp, hi16(t.y)));
        sv = adds16(sv, er[c * 64]);
        rowmax = max16(rowmax, sv);
        mp = mm[c]; ip = im[c]; dp = dm[c];
        im[c] = max16(adds16(mp, hi16(t.z)), adds16(ip, lo16(t.w)));
        mm[c] = sv;
        dm[c] = dcarry;                       // M(i,k-1) -> D(i,k); node c = 0 is patched below
        dcarry = adds16(sv, lo16(t.z));
        dmax = max16(dmax, dcarry);
        tdd[c] = hi16(t.w);
      }
      dm[0] = (short) dpp_shr1(dcarry, NEG);

      const int xE = wave_max_i32((int) rowmax);
      if (xE >= 32767) overflow = true;
      xC = max(xC, xE + a.xw_e);
      xJ = max(xJ, xE + a.xw_e);
      xB = max(xJ + xwm, xN + xwm);

      const int Dmax = wave_max_i32((int) dmax);
      if (Dmax + a.ddbound > xB) {            // lazy F, then the chunk carries relaxed to their fixed point
#pragma unroll unroll_c(C)
        for (int c = 1; c < C; ++c) dm[c] = max16(dm[c], adds16(dm[c - 1], tdd[c - 1]));
        for (int pass = 0; pass < 64; ++pass) {
          const short ddout = adds16(dm[C - 1], tdd[C - 1]);
          const short cand = (short) dpp_shr1(ddout, NEG);
          const int improved = wave_max_i32((cand > dm[0]) ? 1 : 0);
          if (improved == 0) break;
          dm[0] = max16(dm[0], cand);
#pragma unroll unroll_c(C)
          for (int c = 1; c < C; ++c) dm[c] = max16(dm[c], adds16(dm[c - 1], tdd[c - 1]));
        }
      }
    }
  }
  if (lane == 0) a.out[kCalN + s] = overflow ? 32767 : xC;
}

// ======================================================================================= Forward parser
// Row body: the twin of fwd_kernel (p7x_vitfwd.hip) without the stored rows; the same test requires equal scores, bit for bit.
template <int C>
__global__ void __launch_bounds__(kWsBlock) cal_fwd_kernel(const ArgRef ref, const uint8_t *__restrict__ stream)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int Mpad = 64 * C;
  constexpr bool EG = C > 16;         // M > 1024: the emission rows are read through L2
  constexpr bool TG = C > 64;         // M > 4096: the transitions too
  const CalArgs a = load_args<CalArgs>(ref);
  const float4 *tr = TG ? reinterpret_cast<const float4 *>(a.fwd_trans) : reinterpret_cast<const float4 *>(smem);      // [2 Mpad]
  const float *em = EG ? reinterpret_cast<const float *>(a.fwd_emis) : reinterpret_cast<const float *>(smem + (size_t) Mpad * 32);
  {
    if constexpr (!TG) {
      const float4 *gt = reinterpret_cast<const float4 *>(a.fwd_trans);
      float4 *lt = reinterpret_cast<float4 *>(smem);
      for (int i = threadIdx.x; i < 2 * Mpad; i += kWsBlock) lt[i] = gt[i];
    }
    if constexpr (!EG) {
      const float4 *ge = reinterpret_cast<const float4 *>(a.fwd_emis);
      float4 *le = reinterpret_cast<float4 *>(smem + (size_t) Mpad * 32);
      for (int i = threadIdx.x; i < a.K * Mpad / 4; i += kWsBlock) le[i] = ge[i];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int s = cal_sample();
  const uint8_t *sq = stream + kCalOffFwd + (size_t) s * kCalLfwd;
  constexpr int L = kCalLfwd;
  const float pmove = (2.0f + 1.0f) / ((float) L + 2.0f + 1.0f), ploop = 1.0f - pmove;

  float mm[C], im[C], dm[C];
#pragma unroll unroll_c(C)
  for (int c = 0; c < C; ++c) mm[c] = im[c] = dm[c] = 0.0f;
  float ddprod = 1.0f;                // product of this lane's D->D probabilities: the multiplier of an incoming D carry
#pragma unroll unroll_c(C)
  for (int c = 0; c < C; ++c) ddprod *= tr[2 * (c * 64 + lane) + 1].w;

  float xN = 1.0f, xB = pmove, xJ = 0.0f, xC = 0.0f, xE = 0.0f, totscale = 0.0f;
  for (int i0 = 0; i0 < L; i0 += 64) {
    const int nrow = min(64, L - i0);
    const uint32_t resid = (lane < nrow) ? sq[i0 + lane] : 0;
    for (int r = 0; r < nrow; ++r) {
      const int x = __builtin_amdgcn_readlane((int) resid, r);
      const float *er = em + x * Mpad + lane;
      float mp = dpp_shr1f(mm[C - 1], 0.0f), ip = dpp_shr1f(im[C - 1], 0.0f), dp = dpp_shr1f(dm[C - 1], 0.0f);
      float esum = 0.0f, dcarry = 0.0f;
      float tdd[C], tmd[C];
#pragma unroll unroll_c(C)
      for (int c = 0; c < C; ++c) {
        const F8 t = load_f8(tr, c * 64 + lane);
        float sv = xB * t.bm;
        sv = sv + mp * t.mm;
        sv = sv + ip * t.im;
        sv = sv + dp * t.dm;
        sv = sv * er[c * 64];
        esum = esum + sv;
        mp = mm[c]; ip = im[c]; dp = dm[c];
        im[c] = mp * t.mi + ip * t.ii;
        mm[c] = sv;
        tdd[c] = t.dd; tmd[c] = t.md;
      }
      // D(i,k) = M(i,k-1) tMD(k-1) + D(i,k-1) tDD(k-1): serial inside the lane, affine scan across the lanes
      float A = 0.0f;
#pragma unroll unroll_c(C)
      for (int c = 0; c < C; ++c) { dm[c] = A; A = mm[c] * tmd[c] + A * tdd[c]; }
      float sa = A, sp = ddprod;
      affine_scan_up(sa, sp);
      dcarry = dpp_shr1f(sa, 0.0f);
      {
        float w = dcarry;
#pragma unroll unroll_c(C)
        for (int c = 0; c < C; ++c) { dm[c] = dm[c] + w; esum = esum + dm[c]; w = w * tdd[c]; }
      }
      xE = wave_sum_f32(esum);
      xN = xN * ploop;
      xC = (xC * ploop) + (xE * a.xf_e_move);
      xJ = (xJ * ploop) + (xE * a.xf_e_loop);
      xB = (xJ * pmove) + (xN * pmove);
      if (xE > 1.0e4f) {
        xN = xN / xE; xC = xC / xE; xJ = xJ / xE; xB = xB / xE;
        const float inv = (float) (1.0 / (double) xE);
#pragma unroll unroll_c(C)
        for (int c = 0; c < C; ++c) { mm[c] *= inv; dm[c] *= inv; im[c] *= inv; }
        totscale = (float) ((double) totscale + log((double) xE));
        xE = 1.0f;
      }
    }
  }
  if (lane == 0) {
    float sc;
    if (xC != xC) sc = __builtin_nanf("");
    else if (xC == 0.0f || __builtin_isinf(xC)) sc = __builtin_inff();
    else sc = (float) ((double) totscale + log((double) (xC * pmove)));
    a.out[2 * kCalN + s] = __builtin_bit_cast(int32_t, sc);
  }
}

// ---------------------------------------------------------------------------- host side
// (dynamic LDS: the layouts of p7x_kernels.hpp, with the K rows of the canonical residues that the kernels stage)
template <typename Kern>
static int cal_launch(Kern kernel, size_t lds, const ArgRef &ref, int nmodels, const uint8_t *d_stream, hipStream_t st)
{
  const int gst = kernel_grant_lds(kernel, lds);
  if (gst != P7X_OK) return gst;
  hipLaunchKernelGGL(kernel, dim3(kCalN / (kWsBlock / 64), (unsigned) nmodels), dim3(kWsBlock), lds, st, ref, d_stream);
  P7X_HIP(hipGetLastError());
  return P7X_OK;
}

// what a calibration leases: a stream, the argument records and the raw results, device and pinned host
struct CalSet {
  int device = -1;
  hipStream_t stream = nullptr;
  DeviceBuf d_args, d_out, d_own;      // d_own: the stream of a model that is calibrated alone
  PinnedBuf h_args, h_out, h_own;
};

// the resident samples of a device: one per (alphabet, background, seed, generator), made on first use and kept -- the
// kCalStreamsKept most recently made per process; a caller holds its stream for the length of its call, so one that leaves
// the list (a builder with seed 0 asks for a new seed every time) is released when its last user is done
struct CalStream { int device, abc_type, generator; uint32_t seed; std::vector<float> bg; DeviceBuf buf; };
constexpr size_t kCalStreamsKept = 8;
static std::mutex &cal_streams_mu() { static std::mutex *m = new std::mutex(); return *m; }
static std::vector<std::shared_ptr<CalStream>> &cal_streams() { static auto *v = new std::vector<std::shared_ptr<CalStream>>(); return *v; }

static int resident_stream(DeviceCtx *ctx, CalSet &set, const Profile &p, uint32_t seed, int generator, std::shared_ptr<CalStream> *out)
{
  std::lock_guard<std::mutex> lk(cal_streams_mu());
  for (const auto &s : cal_streams())
    if (s->device == ctx->device && s->abc_type == p.abc_type && s->seed == seed && s->generator == generator &&
        std::memcmp(s->bg.data(), p.bgf, sizeof(float) * p.K) == 0) { *out = s; return P7X_OK; }
  auto s = std::make_shared<CalStream>();
  s->device = ctx->device; s->abc_type = p.abc_type; s->generator = generator; s->seed = seed; s->bg.assign(p.bgf, p.bgf + p.K);
  int st = set.h_own.reserve(P7X_CAL_RESIDUES);
  if (st != P7X_OK) return st;
  if ((st = p7x_calibration_stream(p.abc_type, p.bgf, seed, generator, set.h_own.as<uint8_t>())) != P7X_OK) return st;
  if ((st = s->buf.reserve(ctx, P7X_CAL_RESIDUES)) != P7X_OK) return st;
  P7X_HIP(hipMemcpyAsync(s->buf.as<uint8_t>(), set.h_own.as<uint8_t>(), P7X_CAL_RESIDUES, hipMemcpyHostToDevice, set.stream));
  P7X_HIP(hipStreamSynchronize(set.stream));
  if (cal_streams().size() >= kCalStreamsKept) cal_streams().erase(cal_streams().begin());
  cal_streams().push_back(s);
  *out = s;
  return P7X_OK;
}

static CalArgs cal_args(const Profile &p, const DevProfile *dp, int32_t *d_out)
{
  CalArgs a{};
  a.M = p.M; a.C = dp->vitC; a.K = p.K;
  a.msv_emis = dp->msvw_emis; a.vit_trans = dp->vit_trans; a.vit_emis = dp->vit_emis; a.fwd_trans = dp->fwd_trans; a.fwd_emis = dp->fwd_emis;
  a.base_b = p.base_b; a.bias_b = p.bias_b; a.tec_b = p.tec_b;
  a.tjbm = (int) unbiased_byteify(p.scale_b, logf(3.0f / (float) (kCalLmsv + 3))) + (int) p.tbm_b;
  a.xwm = wordify(p.scale_w, logf((2.0f + 1.0f) / ((float) kCalLvit + 2.0f + 1.0f)));
  a.base_w = p.base_w; a.xw_e = p.xw[XE][MOVE]; a.ddbound = p.ddbound_w;
  a.xf_e_move = p.xf[XE][MOVE]; a.xf_e_loop = p.xf[XE][LOOP];
  a.out = d_out;
  return a;
}

// The three stages of n models (argument records h_args[0..n), sorted by tier) against <d_stream>: queued on the set's stream,
// raw results copied to h_out; returns after the one synchronisation.
static int cal_run(CalSet &set, int n, const uint8_t *d_stream)
{
  const CalArgs *ha = set.h_args.as<CalArgs>();
  P7X_HIP(hipMemcpyAsync(set.d_args.as<CalArgs>(), ha, sizeof(CalArgs) * (size_t) n, hipMemcpyHostToDevice, set.stream));
  for (int lo = 0; lo < n;) {
    int hi = lo;
    while (hi < n && ha[hi].C == ha[lo].C) ++hi;
    const ArgRef ref{ set.d_args.as<CalArgs>() + lo, (uint32_t) sizeof(CalArgs) };
    const int K = ha[lo].K, nm = hi - lo;
    const int st = node_tier_dispatch(ha[lo].C, "model too long for the calibration kernels", [&](auto tier) {
      constexpr int CC = decltype(tier)::value;
      int s1 = cal_launch(cal_msv_kernel<CC>, msv_wave_lds_bytes(CC, K), ref, nm, d_stream, set.stream);
      if (s1 == P7X_OK) s1 = cal_launch(cal_vit_kernel<CC>, vit_lds_bytes(CC, K), ref, nm, d_stream, set.stream);
      if (s1 == P7X_OK) s1 = cal_launch(cal_fwd_kernel<CC>, fwd_lds_bytes(CC, K), ref, nm, d_stream, set.stream);
      return s1;
    });
    if (st != P7X_OK) return st;
    lo = hi;
  }
  P7X_HIP(hipMemcpyAsync(set.h_out.as<int32_t>(), set.d_out.as<int32_t>(), sizeof(int32_t) * 3 * kCalN * (size_t) n, hipMemcpyDeviceToHost, set.stream));
  P7X_HIP(hipStreamSynchronize(set.stream));
  return P7X_OK;
}

static int cal_fit(const p7x_oprofile *om, const int32_t *raw, float *evparam)
{
  float sc[3 * kCalN];
  uint8_t ovf[2 * kCalN];
  int st = p7x_calibration_scores(om, raw, raw + kCalN, sc, ovf);
  if (st != P7X_OK) return st;
  std::memcpy(sc + 2 * kCalN, raw + 2 * kCalN, sizeof(float) * kCalN);
  return p7x_calibration_fit(sc, ovf, om->p.relent_mh, evparam);
}

// A model one of whose samples overflowed: its own stream, found by throwing away the first overflowed draw, drawing the rest
// again and scoring them, until no kept sample overflows.
static int cal_alone(DeviceCtx *ctx, CalSet &set, const p7x_oprofile *om, const DevProfile *dp, uint32_t seed, int generator,
                     int32_t *raw, float *evparam)
{
  const Profile &p = om->p;
  std::vector<int32_t> skipped;
  int st = P7X_OK;
  if ((st = set.d_own.reserve(ctx, P7X_CAL_RESIDUES)) != P7X_OK) return st;
  if ((st = set.h_own.reserve(P7X_CAL_RESIDUES)) != P7X_OK) return st;
  for (int round = 0; round < 64; ++round) {
    const int32_t *h = set.h_out.as<int32_t>();
    if (round > 0) std::memcpy(raw, h, sizeof(int32_t) * 3 * kCalN);
    int first = -1;
    for (int i = 0; i < 2 * kCalN && first < 0; ++i) if (i < kCalN ? raw[i] < 0 : raw[i] >= 32767) first = i;
    if (first < 0) return cal_fit(om, raw, evparam);
    skipped.push_back(p7x_calibration_draw_of(first, skipped.data(), (int) skipped.size()));
    if ((st = p7x_calibration_redraw(p.abc_type, p.bgf, seed, generator, skipped.data(), (int) skipped.size(), set.h_own.as<uint8_t>())) != P7X_OK) return st;
    P7X_HIP(hipMemcpyAsync(set.d_own.as<uint8_t>(), set.h_own.as<uint8_t>(), P7X_CAL_RESIDUES, hipMemcpyHostToDevice, set.stream));
    set.h_args.as<CalArgs>()[0] = cal_args(p, dp, set.d_out.as<int32_t>());
    if ((st = cal_run(set, 1, set.d_own.as<uint8_t>())) != P7X_OK) return st;
  }
  set_error("calibration: the model's samples keep overflowing the filters");
  return P7X_ERANGE;
}

} // namespace p7x

using namespace p7x;

extern "C" {

int p7x_calibrate_batch(p7x_oprofile *const *oms, size_t nq, int device, uint32_t seed, float *out_evparam, int32_t *out_scores)
{
  if (!oms || !out_evparam) { set_error("p7x_calibrate_batch: bad arguments"); return P7X_EINVAL; }
  DeviceCtx *ctx = nullptr;
  int st = get_ctx(device, &ctx);
  if (st != P7X_OK) return st;
  if (nq == 0) return P7X_OK;
  const int generator = P7X_CAL_GENERATOR;
  for (size_t q = 0; q < nq; ++q) {
    if (!oms[q]) { set_error("p7x_calibrate_batch: bad arguments"); return P7X_EINVAL; }
    const Profile &p = oms[q]->p, &p0 = oms[0]->p;
    if (!(p.relent_mh > 0.0)) { set_error("calibration needs the relative entropy of the core model: '" + p.name + "' does not carry it"); return P7X_EINVAL; }
    if (p.abc_type != p0.abc_type || std::memcmp(p.bgf, p0.bgf, sizeof(float) * p.K) != 0) { set_error("the profiles of a calibration batch share one alphabet and one background"); return P7X_EINVAL; }
    if (vit_pick_C(p.M) <= 0) { set_error(model_too_long("model too long for the calibration kernels")); return P7X_EINVAL; }
  }
  auto lease = LeasePool<CalSet>::instance().lease(ctx->device, [](const CalSet &, const CalSet *b) { return !b; });
  CalSet &set = *lease;
  if (set.stream == nullptr) P7X_HIP(hipStreamCreateWithFlags(&set.stream, hipStreamNonBlocking));
  std::shared_ptr<CalStream> resident;
  if ((st = resident_stream(ctx, set, oms[0]->p, seed, generator, &resident)) != P7X_OK) return st;
  const uint8_t *d_stream = resident->buf.as<uint8_t>();
  const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  constexpr size_t kChunk = 1024;             // models per launch set
  std::vector<DevProfile *> dps;
  std::vector<int> order;
  for (size_t base = 0; base < nq; base += kChunk) {
    const int n = (int) std::min(kChunk, nq - base);
    dps.assign((size_t) n, nullptr);
    if ((st = get_dev_profiles(oms + base, n, ctx, dps.data(), (int) hw)) != P7X_OK) return st;
    order.resize((size_t) n);
    for (int i = 0; i < n; ++i) order[(size_t) i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return dps[(size_t) x]->vitC < dps[(size_t) y]->vitC; });
    if ((st = set.h_args.reserve(sizeof(CalArgs) * (size_t) n)) != P7X_OK) return st;
    if ((st = set.d_args.reserve(ctx, sizeof(CalArgs) * (size_t) n)) != P7X_OK) return st;
    if ((st = set.h_out.reserve(sizeof(int32_t) * 3 * kCalN * (size_t) n)) != P7X_OK) return st;
    if ((st = set.d_out.reserve(ctx, sizeof(int32_t) * 3 * kCalN * (size_t) n)) != P7X_OK) return st;
    for (int j = 0; j < n; ++j) {             // record j = model order[j]; its results at h_out[j]
      const int i = order[(size_t) j];
      set.h_args.as<CalArgs>()[j] = cal_args(oms[base + (size_t) i]->p, dps[(size_t) i], set.d_out.as<int32_t>() + (size_t) j * 3 * kCalN);
    }
    if ((st = cal_run(set, n, d_stream)) != P7X_OK) return st;
    std::vector<int32_t> raw((size_t) n * 3 * kCalN);
    std::memcpy(raw.data(), set.h_out.as<int32_t>(), raw.size() * sizeof(int32_t));
    for (int j = 0; j < n; ++j) {
      const size_t q = base + (size_t) order[(size_t) j];
      int32_t *r = raw.data() + (size_t) j * 3 * kCalN;
      float *ev = out_evparam + q * 6;
      st = cal_fit(oms[q], r, ev);
      if (st == P7X_ERANGE) {
        bool ovf = false;
        for (int i = 0; i < 2 * kCalN; ++i) ovf = ovf || (i < kCalN ? r[i] < 0 : r[i] >= 32767);
        if (ovf) st = cal_alone(ctx, set, oms[q], dps[(size_t) order[(size_t) j]], seed, generator, r, ev);
      }
      if (st != P7X_OK) return st;
      std::memcpy(oms[q]->p.evparam, ev, sizeof(float) * 6);
      if (out_scores) std::memcpy(out_scores + q * 3 * kCalN, r, sizeof(int32_t) * 3 * kCalN);
    }
  }
  return P7X_OK;
}

} // extern "C"
