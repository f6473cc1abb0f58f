// p7x_alignlog.hip -- hmmalign's float64 log-space path on CDNA4 (TraceAligner(logspace=True)): the
// mathematics of the host log twin (p7x_logdp.cpp), one whole sequence per WAVEFRONT.
//
// Lane l of the wavefront owns nodes l + 1, l + 65, ...: a row is walked in chunks of 64 consecutive nodes, so every row
// load and store is one coalesced run of 512 bytes.  All row state lives in the wavefront's slab of the workspace (the
// posteriors, the optimal-accuracy matrix, a few rolling rows); nothing is indexed by nodes per lane, so there is ONE
// instantiation for every model length and no private segment.  The D -> D chain of a chunk is a linear recurrence
// D(k) = a(k) (+) b(k) (x) D(k-1) in the log semiring (the max-plus one in optimal accuracy): a wave scan over the pairs
// (a, b), the carry handed from chunk to chunk.  Row sums are running (max, sum of exp) pairs, one logarithm per row.
// The summation order therefore is not the twin's; in float64 the two differ by about 1e-12, and instead of bit identity
// the traceback carries the guard pattern of p7x_oaguard.hpp: a choice on the trace whose two best candidates lie within
// kOaGuard of each other, or a posterior within kDigitBand of a printed digit's boundary, sets status bit 6 and the host
// repeats the sequence with the twin.
#include "p7x_oaguard.hpp"
#include "p7x_logdp.hpp"
#include "p7x_host.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>

namespace p7x {

namespace {

constexpr double kOaGuard = 1.0e-9;       // relative + absolute half-width of a near-tie between optimal-accuracy values
constexpr double kDigitBand = 2.0e-6;     // of (p + 0.05) * 10 around an integer: two float32 ulps of p and then some

struct LogAlignArgs {
  int M, W, Q, Kp, nseq, Lmax;
  const double *t;          // [8][W] log transitions
  const double *e;          // [Kp][W] log match odds
  const uint8_t *gates;     // [W] open transitions of a node
  const uint8_t *dsq;
  const int64_t *sq;        // [nseq] offset in dsq of the first residue
  const int32_t *len;       // [nseq]
  const double *lm;         // [nseq][2] log pmove, log ploop of the sequence's length model
  double *work; long long work_stride;      // per-wavefront slab (alignlog_work_doubles), rows 0..Lmax
  const int64_t *tr_off;    // [nseq] first trace element; capacity len + M + 16 each
  uint32_t *tr_a; int32_t *tr_i; float *tr_pp;
  int32_t *tr_n, *status;   // status: bit 2 traceback failure, bit 6 a close call on the trace
  float *out_sc;            // [nseq][2] Forward score (nats), optimal-accuracy score
};

__device__ __forceinline__ double up1(double v, double fill, int lane) { const double u = __shfl_up(v, 1); return lane == 0 ? fill : u; }
__device__ __forceinline__ double wave_max_f64(double v)
{
  for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d));
  return v;
}

// running log-sum: max and the sum of exp(v - max)
struct Lse {
  double m = kLogZero, s = 0.0;
  __device__ __forceinline__ void add(double v)
  {
    if (v > m) { s = s * exp(m - v) + 1.0; m = v; }
    else if (v > kLogZero) s += exp(v - m);
  }
  __device__ __forceinline__ double wave_total() const
  {
    const double mx = wave_max_f64(m);
    double part = (m > kLogZero) ? s * exp(m - mx) : 0.0;
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
    return (mx > kLogZero) ? mx + log(part) : kLogZero;
  }
};

// D(k) = a(k) (+) (b(k) + D(k-1)) over the 64 nodes of a chunk, D(first - 1) = carry; log semiring
__device__ __forceinline__ double chain_logsum(double a, double b, double carry, int lane)
{
  for (int d = 1; d < 64; d <<= 1) {
    const double au = __shfl_up(a, d), bu = __shfl_up(b, d);
    if (lane >= d) { a = logsum(a, b + au); b = b + bu; }
  }
  return logsum(a, b + carry);
}
// ... and the max-plus semiring (b is 0 or -inf)
__device__ __forceinline__ double chain_max(double a, double b, double carry, int lane)
{
  for (int d = 1; d < 64; d <<= 1) {
    const double au = __shfl_up(a, d), bu = __shfl_up(b, d);
    if (lane >= d) { a = fmax(a, b + au); b = b + bu; }
  }
  return fmax(a, b + carry);
}

// the carving of a wavefront's slab
struct Slab {
  double *pm, *pi, *om, *oi, *od, *roll, *x, *oN, *oC, *oE, *ppN, *ppC;
  __device__ Slab(double *base, int W, int rows)
  {
    const size_t mat = (size_t) rows * W;
    pm = base; pi = pm + mat; om = pi + mat; oi = om + mat; od = oi + mat;
    roll = od + mat; x = roll + (size_t) 6 * W;
    oN = x + (size_t) rows * LX_N; oC = oN + rows; oE = oC + rows; ppN = oE + rows; ppC = ppN + rows;
  }
};

struct DevView {
  int M, W, Q, L, lane;
  const double *om, *oi, *od, *pm, *pi, *oN, *oC, *oE, *ppN, *ppC;
  const uint8_t *g;
  __device__ double oM(int i, int k) const { return om[(size_t) i * W + k]; }
  __device__ double oI(int i, int k) const { return oi[(size_t) i * W + k]; }
  __device__ double oD(int i, int k) const { return od[(size_t) i * W + k]; }
  __device__ double pM(int i, int k) const { return pm[(size_t) i * W + k]; }
  __device__ double pI(int i, int k) const { return pi[(size_t) i * W + k]; }
  __device__ double xN(int i) const { return oN[i]; }
  __device__ double xC(int i) const { return oC[i]; }
  __device__ double xE(int i) const { return oE[i]; }
  __device__ double pN(int i) const { return ppN[i]; }
  __device__ double pC(int i) const { return ppC[i]; }
  __device__ unsigned gates(int k) const { return g[k]; }
  // E <- M / D: the cell OaView::pick_E's sequential walk ends on is the LAST match cell (in the striped visiting order)
  // that holds the row maximum, or, when no match cell does, the FIRST delete cell that holds it
  template <class Guard> __device__ void pick_E(int i, int *k, int *s, Guard &guard) const
  {
    const double *mr = om + (size_t) i * W, *dr = od + (size_t) i * W;
    double mx = kLogZero;
    for (int kk = lane + 1; kk <= M; kk += 64) mx = fmax(mx, fmax(mr[kk], dr[kk]));
    mx = wave_max_f64(mx);
    const double thr = mx - (fabs(mx) * kOaGuard + kOaGuard);
    int lastM = -1, firstD = 0x7fffffff, close = 0;
    for (int kk = lane + 1; kk <= M; kk += 64) {
      const int q = (kk - 1) % Q, z = (kk - 1) / Q;
      const double m = mr[kk], d = dr[kk];
      if (m == mx) lastM = max(lastM, q * 8 + z);
      if (d == mx) firstD = min(firstD, q * 8 + 4 + z);
      close += m >= thr ? 1 : 0;
    }
    for (int d = 32; d >= 1; d >>= 1) {
      lastM = max(lastM, __shfl_xor(lastM, d));
      firstD = min(firstD, __shfl_xor(firstD, d));
      close += __shfl_xor(close, d);
    }
    // D cells copy the match cell they derive from (a structural tie, the same in any order of operations): only a second
    // MATCH cell within the guard of the maximum -- or an end in a delete state -- makes the end cell a close call
    if (close > 1 || lastM < 0) guard.flag = 1;
    if (lastM >= 0) { *s = LT_M; *k = (lastM & 7) * Q + (lastM >> 3) + 1; }
    else if (firstD != 0x7fffffff) { *s = LT_D; *k = ((firstD & 7) - 4) * Q + (firstD >> 3) + 1; }
    else { *s = -1; *k = 0; }
  }
};

struct DevGuard {
  int flag = 0;
  __device__ void tie(double x, double y) { if (fabs(x - y) <= fabs(fmax(x, y)) * kOaGuard + kOaGuard) flag = 1; }
  __device__ void digit(double p)
  {
    const double v = (p + 0.05) * 10.0;
    if (fabs(v - rint(v)) < kDigitBand && v > 0.75) flag = 1;
  }
};

__global__ __launch_bounds__(64) void alignlog_kernel(const LogAlignArgs a)
{
  const int lane = (int) threadIdx.x, M = a.M, W = a.W;
  const int rows = a.Lmax + 1;
  Slab sl(a.work + (size_t) blockIdx.x * (size_t) a.work_stride, W, rows);
  const double *bm = a.t + (size_t) tBM * W, *mm = a.t + (size_t) tMM * W, *im = a.t + (size_t) tIM * W, *dm = a.t + (size_t) tDM * W;
  const double *md = a.t + (size_t) tMD * W, *mi = a.t + (size_t) tMI * W, *ii = a.t + (size_t) tII * W, *dd = a.t + (size_t) tDD * W;

  for (int s = (int) blockIdx.x; s < a.nseq; s += (int) gridDim.x) {
    const int L = a.len[s];
    if (L < 1 || L > a.Lmax) { if (lane == 0) { a.status[s] = 4; a.tr_n[s] = 0; } continue; }
    const uint8_t *sq = a.dsq + a.sq[s] - 1;               // 1-based residues
    const double move = a.lm[2 * s], loop = a.lm[2 * s + 1];
    auto residue = [&](int i) { const int x = sq[i]; return x < a.Kp ? x : a.Kp - 1; };

    // ------------------------------------------------------------------ 1. Forward: M and I of every row stay
    double *dprev = sl.roll, *dcur = sl.roll + W;
    for (int k = lane; k < W; k += 64) { sl.pm[k] = kLogZero; sl.pi[k] = kLogZero; dprev[k] = kLogZero; dcur[k] = kLogZero; }
    double fN = 0.0, fB = move, fC = kLogZero;
    if (lane == 0) { double *x = sl.x; x[LX_FN] = fN; x[LX_FB] = fB; x[LX_FC] = fC; x[LX_BN] = kLogZero; x[LX_BC] = kLogZero; }
    phase_fence();
    for (int i = 1; i <= L; ++i) {
      const double *e = a.e + (size_t) residue(i) * W;
      const double *mp = sl.pm + (size_t) (i - 1) * W, *ip = sl.pi + (size_t) (i - 1) * W;
      double *mc = sl.pm + (size_t) i * W, *ic = sl.pi + (size_t) i * W;
      double carryD = kLogZero, carryU = kLogZero;
      Lse accE;
      for (int base = 1; base <= M; base += 64) {
        const bool act = base + lane <= M;
        const int k = act ? base + lane : M + 1;
        const double mv = e[k] + logsum(logsum(fB + bm[k], mp[k - 1] + mm[k]), logsum(ip[k - 1] + im[k], dprev[k - 1] + dm[k]));
        const double iv = logsum(mp[k] + mi[k], ip[k] + ii[k]);
        const double u = act ? mv + md[k] : kLogZero;
        const double dv = chain_logsum(up1(u, carryU, lane), act ? dd[k - 1] : kLogZero, carryD, lane);
        if (act) { mc[k] = mv; ic[k] = iv; dcur[k] = dv; accE.add(mv); accE.add(dv); }
        carryD = __shfl(dv, 63); carryU = __shfl(u, 63);
      }
      if (lane == 0) { mc[0] = ic[0] = dcur[0] = kLogZero; mc[M + 1] = ic[M + 1] = dcur[M + 1] = kLogZero; }
      const double xE = accE.wave_total();
      fN = fN + loop;
      fC = logsum(fC + loop, xE);
      fB = fN + move;
      if (lane == 0) { double *x = sl.x + (size_t) i * LX_N; x[LX_FN] = fN; x[LX_FB] = fB; x[LX_FC] = fC; }
      double *t = dprev; dprev = dcur; dcur = t;
      phase_fence();
    }
    const double tot = fC + move;
    if (!(tot > kLogZero)) { if (lane == 0) { a.status[s] = 4; a.tr_n[s] = 0; } continue; }

    // ------------------------------------------------------------------ 2. Backward on rolling rows; row i's posteriors
    // replace Forward's row i as soon as both are known.  Node k of a chunk sits in lane r - base with r = M - k: the
    // chain runs towards lower nodes and the scan towards higher lanes.
    double *bmn = sl.roll + 2 * (size_t) W, *bin = bmn + W, *bmc = bin + W, *bic = bmc + W;
    for (int k = lane; k < W; k += 64) { bmn[k] = kLogZero; bin[k] = kLogZero; bmc[k] = kLogZero; bic[k] = kLogZero; }
    double bN = kLogZero, bC = move;
    phase_fence();
    for (int i = L; i >= 0; --i) {
      const bool last = i == L;
      const double *e = last ? a.e : a.e + (size_t) residue(i + 1) * W;
      if (!last) bC = bC + loop;
      double *fm = sl.pm + (size_t) i * W, *fi = sl.pi + (size_t) i * W;
      double carryD = kLogZero;
      Lse accB;
      for (int base = 0; base < M; base += 64) {
        const bool act = base + lane < M;
        const int k = act ? M - (base + lane) : 0;
        double a_m = kLogZero, a_d = kLogZero, iv = kLogZero;
        if (!last) {
          const double em0 = e[k] + bmn[k], em1 = e[k + 1] + bmn[k + 1];
          if (act) accB.add(bm[k] + em0);
          a_m = logsum(mm[k + 1] + em1, mi[k] + bin[k]);
          a_d = dm[k + 1] + em1;
          iv = logsum(im[k + 1] + em1, ii[k] + bin[k]);
        }
        if (i == 0) continue;                                // row 0: only B <- M of row 1 is needed (uniform: no lane leaves alone)
        const double dv = chain_logsum(act ? logsum(bC, a_d) : kLogZero, act ? dd[k] : kLogZero, carryD, lane);
        const double down = up1(dv, carryD, lane);           // D(k + 1)
        const double mv = logsum(logsum(bC, a_m), md[k] + down);
        if (act) {
          bmc[k] = mv; bic[k] = iv;
          fm[k] = exp(fm[k] + mv - tot);
          fi[k] = exp(fi[k] + iv - tot);
        }
        carryD = __shfl(dv, 63);
      }
      if (!last) {
        const double xB = accB.wave_total();
        bN = logsum(xB + move, bN + loop);
      }
      if (i == 0) break;
      if (lane == 0) {
        bmc[0] = bic[0] = bmc[M + 1] = bic[M + 1] = kLogZero;
        fm[0] = fi[0] = fm[M + 1] = fi[M + 1] = 0.0;
        const double *xp = sl.x + (size_t) (i - 1) * LX_N;
        sl.ppN[i] = exp(xp[LX_FN] + loop + bN - tot);
        sl.ppC[i] = exp(xp[LX_FC] + loop + bC - tot);
      }
      double *t = bmn; bmn = bmc; bmc = t;
      t = bin; bin = bic; bic = t;
      phase_fence();
    }

    // ------------------------------------------------------------------ 3. optimal accuracy, float64
    for (int k = lane; k < W; k += 64) { sl.om[k] = kLogZero; sl.oi[k] = kLogZero; sl.od[k] = kLogZero; }
    double oN = 0.0, oC = kLogZero;
    if (lane == 0) { sl.oN[0] = 0.0; sl.oC[0] = kLogZero; sl.oE[0] = kLogZero; sl.ppN[0] = 0.0; sl.ppC[0] = 0.0; }
    phase_fence();
    for (int i = 1; i <= L; ++i) {
      const double *mp = sl.om + (size_t) (i - 1) * W, *ip = sl.oi + (size_t) (i - 1) * W, *dp = sl.od + (size_t) (i - 1) * W;
      const double *pm = sl.pm + (size_t) i * W, *pi = sl.pi + (size_t) i * W;
      double *mc = sl.om + (size_t) i * W, *ic = sl.oi + (size_t) i * W, *dc = sl.od + (size_t) i * W;
      double carryD = kLogZero, carryU = kLogZero, xE = kLogZero;
      for (int base = 1; base <= M; base += 64) {
        const bool act = base + lane <= M;
        const int k = act ? base + lane : M + 1;
        const unsigned g = a.gates[k], gp = a.gates[k - 1];
        double sv = oa_gate(g, tBM, oN);
        sv = fmax(sv, oa_gate(g, tMM, mp[k - 1]));
        sv = fmax(sv, oa_gate(g, tIM, ip[k - 1]));
        sv = fmax(sv, oa_gate(g, tDM, dp[k - 1]));
        const double mv = sv + pm[k];
        const double iv = fmax(oa_gate(g, tMI, mp[k]), oa_gate(g, tII, ip[k])) + pi[k];
        const double u = act ? mv : kLogZero;
        const double um = up1(u, carryU, lane);              // M(i, k - 1)
        const double dv = chain_max(act ? oa_gate(gp, tMD, um) : kLogZero, (act && ((gp >> tDD) & 1u)) ? 0.0 : kLogZero, carryD, lane);
        if (act) { mc[k] = mv; ic[k] = iv; dc[k] = dv; xE = fmax(xE, fmax(mv, dv)); }
        carryD = __shfl(dv, 63); carryU = __shfl(u, 63);
      }
      xE = wave_max_f64(xE);
      oC = fmax(oC + sl.ppC[i], xE);
      oN = oN + sl.ppN[i];
      if (lane == 0) {
        mc[0] = ic[0] = dc[0] = mc[M + 1] = ic[M + 1] = dc[M + 1] = kLogZero;
        sl.oN[i] = oN; sl.oC[i] = oC; sl.oE[i] = xE;
      }
      phase_fence();
    }

    // ------------------------------------------------------------------ 4. traceback: every lane walks it, lane 0 writes
    DevView v;
    v.M = M; v.W = W; v.Q = a.Q; v.L = L; v.lane = lane;
    v.om = sl.om; v.oi = sl.oi; v.od = sl.od; v.pm = sl.pm; v.pi = sl.pi;
    v.oN = sl.oN; v.oC = sl.oC; v.oE = sl.oE; v.ppN = sl.ppN; v.ppC = sl.ppC; v.g = a.gates;
    DevGuard guard;
    const int64_t off = a.tr_off[s];
    const int cap = L + M + 16;
    int n = 0, over = 0;
    const bool ok = oa_logspace_trace(v, guard, [&](int st, int k, int i, double pp) {
      if (n >= cap) { over = 1; return; }
      if (lane == 0) { a.tr_a[off + n] = (uint32_t) st | ((uint32_t) k << 8); a.tr_i[off + n] = i; a.tr_pp[off + n] = (float) pp; }
      ++n;
    });
    if (lane == 0) {
      a.status[s] = ((ok && !over) ? 0 : 4) | (guard.flag ? 64 : 0);
      a.tr_n[s] = n;
      a.out_sc[2 * s] = (float) tot; a.out_sc[2 * s + 1] = (float) oC;
    }
    phase_fence();                                           // the slab is used again by this wavefront's next sequence
  }
}

size_t alignlog_work_doubles(int M, int Lmax)
{
  const size_t rows = (size_t) Lmax + 1, W = (size_t) M + 2;
  const size_t d = 5 * rows * W + 6 * W + rows * (LX_N + 5);
  return (d + 31) & ~(size_t) 31;
}

struct LogAlignBuffers {
  int device = -1;
  DeviceBuf work, d_in, d_out;
  PinnedBuf h_in, h_out;
  hipStream_t stream = nullptr;
};

} // namespace

// Sequences <which> (caller indices, longest first) through the log kernel: in rounds of lengths within a factor of two
// and of as many sequences as have per-wavefront slabs within align_budget_bytes(), on a leased stream.  tr / status / origin of p7x_traces are the
// caller's; here: out[t], status[t] for every t of <which>.
int device_align_logspace(const p7x_oprofile *om, DeviceCtx *ctx, const p7x_seqdb *db, const std::vector<int> &which,
                          std::vector<AlignTrace> &out, std::vector<int32_t> &status, int64_t *nrounds, int64_t *work_bytes)
{
  if (which.empty()) return P7X_OK;
  const Profile &p = om->p;
  P7X_HIP(hipSetDevice(db->device));
  LogTables T;
  T.build(p, 1);
  OaGates G;
  G.build(p);
  const int M = p.M, W = T.W;
  const size_t budget = align_budget_bytes();
  Lease<LogAlignBuffers> lease = LeasePool<LogAlignBuffers>::instance().lease(db->device, [](const LogAlignBuffers &a, const LogAlignBuffers *b) { return !b || a.work.capacity() > b->work.capacity(); });
  struct Return { Lease<LogAlignBuffers> &l; ~Return() { sync_and_return(l); } } ret{ lease };
  LogAlignBuffers *lb = lease.get();
  int st = P7X_OK;
  if (!lb->stream && (st = create_tail_stream(ctx, false, &lb->stream)) != P7X_OK) return st;
  hipStream_t s = lb->stream;
  const size_t t_bytes = T.t.size() * 8, e_bytes = T.e.size() * 8, g_bytes = ((size_t) W + 7) & ~(size_t) 7;
  for (size_t pos = 0; pos < which.size();) {
    const int first = which[pos], Lr = db->h_len[(size_t) first];
    const size_t slab = alignlog_work_doubles(M, Lr) * 8;
    if (slab > budget) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "hmmalign: sequence %d (L = %d) alone does not fit the log-space alignment workspace (%.1f GB)", first, Lr, budget / 1e9);
      set_error(buf);
      return P7X_EMEM;
    }
    // a round: every sequence has a wavefront and a slab of its own -- as many as the budget holds, four wavefronts per CU at most
    const size_t resident = std::max<size_t>(1, std::min<size_t>(budget / slab, (size_t) ctx->num_cu * 4));
    size_t end = pos;
    while (end < which.size() && end - pos < resident && 2 * (int64_t) db->h_len[(size_t) which[end]] >= Lr) ++end;
    const size_t n = end - pos;
    const int nblocks = (int) n;
    // inputs: [t][e][gates][sq i64][tr_off i64][lm f64 x 2][len i32]
    const size_t o_t = 0, o_e = o_t + t_bytes, o_g = o_e + e_bytes, o_sq = o_g + g_bytes, o_off = o_sq + n * 8, o_lm = o_off + n * 8, o_len = o_lm + n * 16;
    const size_t in_bytes = o_len + n * 4;
    if ((st = lb->h_in.reserve(in_bytes, in_bytes * 2)) != P7X_OK || (st = lb->d_in.reserve(ctx, in_bytes, in_bytes * 2)) != P7X_OK) return st;
    unsigned char *h_in = lb->h_in.as<unsigned char>(), *d_in = lb->d_in.as<unsigned char>();
    std::memcpy(h_in + o_t, T.t.data(), t_bytes);
    std::memcpy(h_in + o_e, T.e.data(), e_bytes);
    std::memset(h_in + o_g, 0, g_bytes);
    std::memcpy(h_in + o_g, G.g.data(), (size_t) W);
    int64_t *h_sq = reinterpret_cast<int64_t *>(h_in + o_sq), *h_off = reinterpret_cast<int64_t *>(h_in + o_off);
    double *h_lm = reinterpret_cast<double *>(h_in + o_lm);
    int32_t *h_len = reinterpret_cast<int32_t *>(h_in + o_len);
    int64_t ntr = 0;
    for (size_t r = 0; r < n; ++r) {
      const int t = which[pos + r], L = db->h_len[(size_t) t];
      const float pmove = 2.0f / ((float) L + 2.0f), ploop = 1.0f - pmove;       // the engines' float32 constants (LogTables::build)
      h_sq[r] = db->h_off[(size_t) t]; h_len[r] = L; h_off[r] = ntr; ntr += (int64_t) L + M + 16;
      h_lm[2 * r] = std::log((double) pmove); h_lm[2 * r + 1] = ploop > 0.0f ? std::log((double) ploop) : kLogZero;
    }
    const size_t o_st = 0, o_n = o_st + n * 4, o_sc = o_n + n * 4, o_ta = o_sc + n * 8, o_ti = o_ta + (size_t) ntr * 4, o_tp = o_ti + (size_t) ntr * 4;
    const size_t out_bytes = o_tp + (size_t) ntr * 4;
    if ((st = lb->d_out.reserve(ctx, out_bytes, out_bytes * 2)) != P7X_OK || (st = lb->h_out.reserve(out_bytes, out_bytes * 2)) != P7X_OK) return st;
    const size_t work_need = slab * (size_t) nblocks;
    if ((st = lb->work.reserve(ctx, work_need, work_need)) != P7X_OK) return st;
    unsigned char *d_out = lb->d_out.as<unsigned char>();
    LogAlignArgs a{};
    a.M = M; a.W = W; a.Q = T.Q; a.Kp = p.Kp; a.nseq = (int) n; a.Lmax = Lr;
    a.t = reinterpret_cast<const double *>(d_in + o_t); a.e = reinterpret_cast<const double *>(d_in + o_e); a.gates = d_in + o_g;
    a.dsq = db->d_dsq;
    a.sq = reinterpret_cast<const int64_t *>(d_in + o_sq); a.tr_off = reinterpret_cast<const int64_t *>(d_in + o_off);
    a.lm = reinterpret_cast<const double *>(d_in + o_lm); a.len = reinterpret_cast<const int32_t *>(d_in + o_len);
    a.work = lb->work.as<double>(); a.work_stride = (long long) (slab / 8);
    a.status = reinterpret_cast<int32_t *>(d_out + o_st); a.tr_n = reinterpret_cast<int32_t *>(d_out + o_n);
    a.out_sc = reinterpret_cast<float *>(d_out + o_sc);
    a.tr_a = reinterpret_cast<uint32_t *>(d_out + o_ta); a.tr_i = reinterpret_cast<int32_t *>(d_out + o_ti); a.tr_pp = reinterpret_cast<float *>(d_out + o_tp);
    P7X_HIP(hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(alignlog_kernel, dim3((unsigned) nblocks), dim3(64), 0, s, a);
    P7X_HIP(hipGetLastError());
    P7X_HIP(hipMemcpyAsync(lb->h_out.as<void>(), d_out, out_bytes, hipMemcpyDeviceToHost, s));
    P7X_HIP(hipStreamSynchronize(s));
    const unsigned char *h_out = lb->h_out.as<unsigned char>();
    const int32_t *r_st = reinterpret_cast<const int32_t *>(h_out + o_st), *r_n = reinterpret_cast<const int32_t *>(h_out + o_n);
    const float *r_sc = reinterpret_cast<const float *>(h_out + o_sc);
    for (size_t r = 0; r < n; ++r) {
      const int t = which[pos + r];
      status[(size_t) t] = r_st[r];
      if (r_st[r] != 0) continue;
      AlignTrace &at = out[(size_t) t];
      align_trace_from_device(reinterpret_cast<const uint32_t *>(h_out + o_ta) + h_off[r], reinterpret_cast<const int32_t *>(h_out + o_ti) + h_off[r],
                              reinterpret_cast<const float *>(h_out + o_tp) + h_off[r], r_n[r], at);
      at.fwdsc = r_sc[2 * r]; at.oasc = r_sc[2 * r + 1];
    }
    if (nrounds) ++*nrounds;
    if (work_bytes) *work_bytes = std::max<int64_t>(*work_bytes, (int64_t) work_need);
    pos = end;
  }
  return P7X_OK;
}

} // namespace p7x
