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
// The rows are the shared ones of p7x_waverows.hpp -- msv_wave_kernel's (one reduction per row), vit_kernel's and
// fwd_kernel's run the same bodies -- so a kernel here is its staging with K rows, its sample, the constant-length row loop
// and one store.
#include "p7x_waverows.hpp"
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
template <int C>
__global__ void __launch_bounds__(kWsBlock) cal_msv_kernel(const ArgRef ref, const uint8_t *__restrict__ stream)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int Mpad = 64 * C, L = kCalLmsv;
  constexpr bool EG = C > 32;         // M > 2048: the table is read where it lies (L2)
  const CalArgs a = load_args<CalArgs>(ref);
  if constexpr (!EG) stage_lds(smem, a.msv_emis, a.K * Mpad / 8);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const short *em = EG ? reinterpret_cast<const short *>(a.msv_emis) : reinterpret_cast<const short *>(smem);
  const int s = cal_sample();
  const uint8_t *sq = stream + (size_t) s * L;
  int mm[C];
  MsvSpecials m;
  msv_init(mm, m, a.base_b, a.tjbm);
  for (int i0 = 0; i0 < L; i0 += 64) {
    const int nrow = min(64, L - i0);
    const uint32_t resid = (lane < nrow) ? sq[i0 + lane] : 0;
    for (int r = 0; r < nrow; ++r) msv_step(mm, m, em + __builtin_amdgcn_readlane((int) resid, r) * Mpad + lane, a.base_b, a.tec_b, a.tjbm);
  }
  if (lane == 0) a.out[s] = m.score(a.bias_b);
}

// ======================================================================================= Viterbi filter
template <int C>
__global__ void __launch_bounds__(kWsBlock) cal_vit_kernel(const ArgRef ref, const uint8_t *__restrict__ stream)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int Mpad = 64 * C, L = kCalLvit;
  constexpr bool EG = C > 32;         // M > 2048: only the transitions are staged
  constexpr bool TG = C > 128;        // M > 8192: the transitions are read through L2 as well (as vit_kernel)
  static_assert(!TG || EG, "transitions through L2 only where the emissions are");
  const CalArgs a = load_args<CalArgs>(ref);
  if constexpr (!TG) stage_lds(smem, a.vit_trans, Mpad);
  if constexpr (!EG) stage_lds(smem + (size_t) Mpad * 16, a.vit_emis, a.K * Mpad / 8);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint4 *tr = TG ? reinterpret_cast<const uint4 *>(a.vit_trans) : reinterpret_cast<const uint4 *>(smem);      // [Mpad]
  const short *em = EG ? reinterpret_cast<const short *>(a.vit_emis) : reinterpret_cast<const short *>(smem + (size_t) Mpad * 16);
  const int s = cal_sample();
  const uint8_t *sq = stream + kCalOffVit + (size_t) s * L;
  short mm[C], im[C], dm[C], tdd[C];
  ViterbiSpecials v;
  vit_init(mm, im, dm, tdd, v, a.base_w, a.xwm);
  for (int i0 = 0; i0 < L && !v.overflow; i0 += 64) {
    const int nrow = min(64, L - i0);
    const uint32_t resid = (lane < nrow) ? sq[i0 + lane] : 0;
    for (int r = 0; r < nrow && !v.overflow; ++r) {
      const int xE = vit_cells(mm, im, dm, tdd, v, tr, em + __builtin_amdgcn_readlane((int) resid, r) * Mpad + lane, lane);
      vit_finish(dm, tdd, v, xE, a.xw_e, a.xwm, a.ddbound);
    }
  }
  if (lane == 0) a.out[kCalN + s] = v.score();
}

// ======================================================================================= Forward parser
template <int C>
__global__ void __launch_bounds__(kWsBlock) cal_fwd_kernel(const ArgRef ref, const uint8_t *__restrict__ stream)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int Mpad = 64 * C, L = kCalLfwd;
  constexpr bool EG = C > 16;         // M > 1024: the emission rows are read through L2
  constexpr bool TG = C > 64;         // M > 4096: the transitions too
  const CalArgs a = load_args<CalArgs>(ref);
  const TransView<false> tr{ TG ? reinterpret_cast<const float4 *>(a.fwd_trans) : reinterpret_cast<const float4 *>(smem), 0 };      // [2 Mpad]
  const float *em = EG ? reinterpret_cast<const float *>(a.fwd_emis) : reinterpret_cast<const float *>(smem + (size_t) Mpad * 32);
  if constexpr (!TG) stage_lds(smem, a.fwd_trans, 2 * Mpad);
  if constexpr (!EG) stage_lds(smem + (size_t) Mpad * 32, a.fwd_emis, a.K * Mpad / 4);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int s = cal_sample();
  const uint8_t *sq = stream + kCalOffFwd + (size_t) s * L;
  const float pmove = length_pmove((float) L), ploop = 1.0f - pmove;
  float mm[C], im[C], dm[C];
  ForwardRow<C, unroll_c(C), ForwardRefs<C>> f{{mm, im, dm}};
  f.init(tr, lane, pmove);
  for (int i0 = 0; i0 < L; i0 += 64) {
    const int nrow = min(64, L - i0);
    const uint32_t resid = (lane < nrow) ? sq[i0 + lane] : 0;
    for (int r = 0; r < nrow; ++r)
      f.row(tr, em, Mpad, lane, __builtin_amdgcn_readlane((int) resid, r), pmove, ploop, a.xf_e_move, a.xf_e_loop);
  }
  if (lane == 0) a.out[2 * kCalN + s] = __builtin_bit_cast(int32_t, forward_score(f.xC, f.totscale, pmove, L));
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
  a.tjbm = (int) tjb_of(p.scale_b, kCalLmsv) + (int) p.tbm_b;
  a.xwm = xw_move_of(p.scale_w, kCalLvit);
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
