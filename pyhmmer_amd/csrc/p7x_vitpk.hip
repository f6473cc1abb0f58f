// p7x_vitpk.hip -- Viterbi filter, packed: T lanes per target (T = 8, 16, 32 or 64), 64/T targets per wavefront.
//
// The wave-per-target kernel in p7x_vitfwd.hip spends most of a row on work that does not shrink with the model:
// wave-wide reductions, the scalar special-state chain, and 16-bit values in 32-bit lanes.  For the common
// Pfam-sized models (M <= 640) this kernel shares those costs between several targets (T = 8, 16); the models of 641 to
// 2,048 nodes get the same packed rows with two targets (T = 32) or one (T = 64) per wavefront:
//   * the nodes are striped over the 2T half-lanes of a group (Farrar): register q of lane s holds node q+1+s*P in
//     its low half and node q+1+(s+T)*P in its high half, so the k-1 neighbour of a register is the register
//     before it and only register 0 takes values from another lane (v_pk_add_i16 clamp / v_pk_max_i16 reproduce
//     _mm_adds_epi16 / _mm_max_epi16 of impl_sse/vitfilter.c exactly);
//   * transitions (8 x int16 per node: BM MM IM DM MD MI II DD) and emissions come from LDS as ds_read_b128,
//     the DP rows (M, I, D) stay in 3P registers, two sets of them (a row reads one and writes the other);
//   * xE and Dmax share one 3- or 4-step DPP butterfly inside the group: each is folded to 16 bits and the two ride in
//     the halves of one dword (T = 32, 64: one or two half exchanges between the 16-lane rows on top,
//     v_permlane16_swap / v_permlane32_swap), the special states are per-lane integers that are uniform within a
//     group; targets that have ended are masked, the row loop runs to the longest target of the wavefront;
//   * lazy F follows upstream in what it decides (Dmax + ddbound > xB, per target), not in when the work is done: the
//     first pass of the D->D closure, two packed ops per register down every stripe, is part of the register loop of
//     every row, and the stripe shift that the row pays for anyway carries the stripe's D->D exit along with M->D.  A
//     target that asks then enters the pass loop (push register 0 down its stripe, carry, repeat until nothing
//     improves: 1.0 to 1.1 passes per row for P >= 8, 2.1 for P = 4), which reads the D->D transitions from LDS again.
// Per row of <8, 8>: 128 packed operations, 37 other VALU, 22 LDS reads (the D->D transitions of the pass loop among
// them); a pass of the closure loop 16 packed, 7 other VALU, 9 scalar (generated code, gfx950;
// profiles/r22_vit_row.md has every instantiation).
// Results are bit-identical to p7x_vitfwd.hip::vit_kernel and to the oracle (tests/test_gpu_filters.py,
// tests/test_gpu_vit_row.py).
#include "p7x_wave.hpp"
#include "p7x_launch.hpp"

namespace p7x {

namespace {

typedef short s2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s2v as_s2v(uint32_t u) { return __builtin_bit_cast(s2v, u); }
__device__ __forceinline__ uint32_t as_u(s2v v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t pk_adds(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_add_sat(as_s2v(a), as_s2v(b))); }
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_max(as_s2v(a), as_s2v(b))); }
__device__ __forceinline__ uint32_t splat16(int v) { const uint32_t w = (uint32_t) v & 0xffffu; return w | (w << 16); }
__device__ __forceinline__ int lo_of(uint32_t w) { return (int) (short) (w & 0xffffu); }
__device__ __forceinline__ int hi_of(uint32_t w) { return (int) (short) (w >> 16); }

constexpr uint32_t kNeg2 = 0x80008000u;      // (-32768, -32768)
// LDS image of the emission rows.  A row is (P+3)/4 chunks, a chunk the uint4 of every lane of a group (pairs 4q .. 4q+3).
// The groups of a wavefront read the rows of different residues, and a ds_read_b128 is served 16 lanes at a time
// (lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... of the 64): which 16-byte slots of the 256-byte bank row those
// lanes hit depends on the residues.
//   T = 16: a chunk is a whole bank row; with a row stride that is a multiple of 16 slots the 16 lanes of a service
//           group always cover 16 different slots, whatever the residues (the odd stride of rounds 1-3 did not).
//   T = 8:  a chunk is half a bank row and a service group takes four lanes of each of four groups (four residues), two of
//           them on slots 0-3 and two on 4-7 of their chunks.  With a stride of 8 mod 16 slots a row starts on either half
//           of a bank row, and a pair conflicts only when its two residues differ and have the same parity: 0.7 extra LDS
//           clocks per service group on average against 1.3 with the odd stride (random residues give random 4-slot
//           windows there, which overlap most of the time).  Measured, KR (M = 262, <8, 17>), 7 queries x 21,113
//           survivors: 3.43 ms against 3.61.  Keeping every chunk twice (slots 0-7 and 8-15, the groups whose second
//           bit is set reading the second copy) removes the conflicts altogether and was slower, 4.07 ms: 40 KB of
//           emissions to stage per workgroup, and the kernel is bound by its packed arithmetic (80 % VALU), not by LDS.
//   T = 32, 64: a chunk is two or four whole bank rows and every service group lies inside one target's group: 16 lanes,
//           16 different slots of one residue row, as for T = 16.
constexpr int vitpk_rowq(int T, int P)
{
  const int n = ((P + 3) / 4) * T;
  return T == 8 ? ((n & 15) == 8 ? n : n + 8) : n;
}

// DPP move.  Every use below either has a source lane for every lane (quad_perm, mirrors, wave_ror) or replaces the one lane
// that has none (wave_shr:1, lane 0 of the wavefront: a group's first lane, which takes the `first` arm of the select in
// stripe_shift).  With bound_ctrl and a zero `old` the move needs no v_mov to materialise the value of the lanes without
// a source; with old = (-32768, -32768) the compiler emitted one in front of every move.
#define P7X_DPP_U(v, ctrl) ((uint32_t) __builtin_amdgcn_update_dpp(0, (int) (v), (ctrl), 0xf, 0xf, true))

// Maxima over the T lanes of a group of two packed pairs at once, every lane receives both: the halves of a are folded
// into the low half of one dword and those of b into its high half (two v_perm_b32 and one packed max), so that one
// butterfly of v_pk_max_i16 serves xE and Dmax.
template <int T>
__device__ __forceinline__ void group_max2(uint32_t a, uint32_t b, int &amax, int &bmax)
{
  uint32_t v = pk_max(__builtin_amdgcn_perm(b, a, 0x05040100u), __builtin_amdgcn_perm(b, a, 0x07060302u));   // (a.lo, b.lo), (a.hi, b.hi)
  v = pk_max(v, P7X_DPP_U(v, 0xB1));      // quad_perm [1,0,3,2]
  v = pk_max(v, P7X_DPP_U(v, 0x4E));      // quad_perm [2,3,0,1]
  v = pk_max(v, P7X_DPP_U(v, 0x141));     // row_half_mirror: 8 lanes
  if constexpr (T >= 16) v = pk_max(v, P7X_DPP_U(v, 0x140));   // row_mirror: 16 lanes
  if constexpr (T >= 32) {      // both operands are v: every lane gets its own value and that of its partner row, in either order
    const auto x = __builtin_amdgcn_permlane16_swap(v, v, false, false);       // rows 0 <-> 1, 2 <-> 3: 32 lanes
    v = pk_max(x[0], x[1]);
  }
  if constexpr (T == 64) {
    const auto x = __builtin_amdgcn_permlane32_swap(v, v, false, false);       // lanes 0-31 <-> 32-63
    v = pk_max(x[0], x[1]);
  }
  amax = lo_of(v); bmax = hi_of(v);
}

#ifdef P7X_VITPK_COUNT
__device__ unsigned long long vitpk_row_counts[3];
#endif

} // namespace

struct RowState { int xN, xB, xJ, xC; bool overflow; };

// Value of the previous stripe for every stripe of a register: lane z-1's register for lanes z >= 1; the first lane of a
// group takes (-32768, lo half of the group's last lane): stripe 0 has no predecessor, stripe T follows stripe T-1.
// T = 32, 64: the last lane of a group is in another DPP row than the first.  T = 64: the rotation of the wavefront brings
// it along.  T = 32 (<hi>: the lane belongs to the second group): two lane reads, both outside the select -- a lane read
// in one arm of a conditional becomes a branch in the row.
template <int T>
__device__ __forceinline__ uint32_t stripe_shift(uint32_t r, bool first, bool hi)
{
  if constexpr (T == 64) {
    const uint32_t w = P7X_DPP_U(r, 0x13C);                           // wave_ror:1: lane 0 <- lane 63
    return first ? ((w << 16) | 0x8000u) : w;
  }
  const uint32_t prev = P7X_DPP_U(r, 0x138);                          // wave_shr:1
  uint32_t last;
  if constexpr (T == 32) {
    const uint32_t l31 = (uint32_t) __builtin_amdgcn_readlane((int) r, 31), l63 = (uint32_t) __builtin_amdgcn_readlane((int) r, 63);
    last = hi ? l63 : l31;
  } else last = P7X_DPP_U(r, T == 8 ? 0x141 : 0x140);                 // row_half_mirror / row_mirror: lane 0 <- lane T-1
  return first ? ((last << 16) | 0x8000u) : prev;
}

// One DP row for the G targets of a wavefront: reads the previous row from (mi, ii, di), writes (mo_, io_, do_).
// Register q of a lane holds the nodes q + 1 + s*P of its two stripes s = lane (low half) and lane + T (high half),
// so the k-1 neighbour of a register is the register before it and only register 0 needs values from another lane.
template <int T, int P>
__device__ __forceinline__ void vit_row(const VitPkArgs &a, const uint4 *tral, const uint4 *trbl, const uint4 *er, bool first, bool hi,
                                        bool active, int xwm, const uint32_t (&mi)[P], const uint32_t (&ii)[P],
                                        const uint32_t (&di)[P], uint32_t (&mo_)[P], uint32_t (&io_)[P], uint32_t (&do_)[P],
                                        RowState &rs)
{
  constexpr int PS = (P + 3) & ~3;
  const uint32_t xBv = splat16(rs.xB);
  uint32_t mp = stripe_shift<T>(mi[P - 1], first, hi), ip = stripe_shift<T>(ii[P - 1], first, hi), dp = stripe_shift<T>(di[P - 1], first, hi);
  uint32_t xEv = kNeg2, dmaxv = kNeg2, dcv = kNeg2;
  uint32_t ddp = kNeg2;                    // D->D transition out of the register before this one
#pragma unroll
  for (int j4 = 0; j4 < PS; j4 += 4) {
    const uint4 e4 = er[(j4 / 4) * T];
    const uint32_t ev[4] = { e4.x, e4.y, e4.z, e4.w };
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int q = j4 + jj;
      if (q < P) {
        const uint4 ta = tral[q * T], tb = trbl[q * T];          // BM MM IM DM | MD MI II DD
        // four independent adds, then a max tree: the same values as the serial chain, half its depth
        const uint32_t a0 = pk_adds(xBv, ta.x), a1 = pk_adds(mp, ta.y), a2 = pk_adds(ip, ta.z), a3 = pk_adds(dp, ta.w);
        uint32_t sv = pk_max(pk_max(a0, a1), pk_max(a2, a3));
        sv = pk_adds(sv, ev[jj]);
        xEv = pk_max(xEv, sv);
        mo_[q] = sv;
        // D(i,k) = max(M(i,k-1) + MD, D(i,k-1) + DD) down the stripe: the first pass of the D->D closure, two packed
        // operations per register among the fourteen others, whether or not a target asks for the closure (below).
        // Register 0 counts as -32768 here: what enters a stripe from the one before is known only after the loop.
        if (q == 1) do_[1] = dcv;
        if (q > 1) do_[q] = pk_max(dcv, pk_adds(do_[q - 1], ddp));
        ddp = tb.w;
        dcv = pk_adds(sv, tb.x);
        dmaxv = pk_max(dmaxv, dcv);
        io_[q] = pk_max(pk_adds(mi[q], tb.y), pk_adds(ii[q], tb.z));
        mp = mi[q]; ip = ii[q]; dp = di[q];
      }
    }
    // keep the LDS loads of later registers behind this point: hoisting all 2P transition loads costs 8 VGPRs each
    asm volatile("" ::: "memory");
  }
  // the first node of a stripe follows the last of the one before: M->D, and the D->D exit of that stripe's first pass
  do_[0] = stripe_shift<T>(pk_max(dcv, pk_adds(do_[P - 1], ddp)), first, hi);
  int xE, Dmax;
  group_max2<T>(xEv, dmaxv, xE, Dmax);
  if (active) {
    if (xE >= 32767) rs.overflow = true;
    rs.xC = max(rs.xC, xE + a.xw_e);               // xw[C][LOOP] = xw[J][LOOP] = xw[N][LOOP] = 0
    rs.xJ = max(rs.xJ, xE + a.xw_e);
    rs.xB = max(rs.xJ + xwm, rs.xN + xwm);
  }
  const bool trig = active && (Dmax + a.ddbound > rs.xB);          // lazy F, per target
  // After the first pass every register but 0 is closed under D->D inside its stripe, and register 0 holds what the
  // stripe before sends.  What remains is to push that value down its own stripe and to carry on from there: the pass
  // loop as it was, entered from a row that is one pass further.  The fixed point of a max-plus relaxation does not
  // depend on the order of the relaxations, so the loop ends where it ended when it started from M->D alone.
  // (A test whether any register 0 of a target that asked beats its register 1, adds(do_[0], DD[0]) > do_[1], would
  // show a row that is closed already.  Measured on 300-residue targets, M = 60 ... 500: it spared 0.0 % of the rows
  // that enter, with 64 lanes there is always one.)
#ifdef P7X_VITPK_COUNT           // build-time experiment: rows of all wavefronts, rows that enter the pass loop, passes
  const bool count_lane = (threadIdx.x & 63) == 0;
  if (count_lane) atomicAdd(&vitpk_row_counts[0], 1ull);
#endif
#ifdef P7X_VITPK_NO_CLOSURE      // build-time experiment (timing only, wrong scores): what the remaining passes cost
  if (false) {
#else
  if (__any(trig)) {
#endif
#ifdef P7X_VITPK_COUNT
    if (count_lane) atomicAdd(&vitpk_row_counts[1], 1ull);
#endif
    // The registers of every target of the wavefront are walked, also of those that did not ask for the closure:
    // relaxing D->D edges of such a target cannot reach the next row's M (that is what the lazy-F bound says), so its
    // score is the same with or without them; the first pass above relies on the same bound.  Only the carry into the
    // next stripe is restricted to the targets that asked, so that the others cannot prolong the loop.  Passes repeat
    // until no stripe improves (2T at most).
    // The D->D transitions come from LDS once more: the registers of the row just read are free here, whereas P
    // registers held from row to row for this loop cost most instantiations a wavefront per SIMD.
    uint32_t tdd[P];
#pragma unroll
    for (int q = 0; q < P; ++q) tdd[q] = trbl[q * T].w;
    int pass = 0;
    bool more;
    do {
#pragma unroll
      for (int q = 1; q < P; ++q) do_[q] = pk_max(do_[q], pk_adds(do_[q - 1], tdd[q - 1]));
      uint32_t c = stripe_shift<T>(pk_adds(do_[P - 1], tdd[P - 1]), first, hi);
      if (!trig) c = kNeg2;
      const uint32_t d0 = pk_max(do_[0], c);
      const bool changed = d0 != do_[0];
      do_[0] = d0;
      more = __any(changed) && ++pass < 2 * T;
#ifdef P7X_VITPK_COUNT
      if (count_lane) atomicAdd(&vitpk_row_counts[2], 1ull);
#endif
    } while (more);
  }
}

// Wavefronts per workgroup.  The tables of a model beyond 640 nodes take 57 to 152 KiB of LDS, so a compute unit holds one
// or two workgroups whatever their size: with four wavefronts each that is one wavefront per SIMD for P >= 17 (T = 32) and
// for every T = 64, and the row's LDS reads and dependent packed operations have nothing to overlap with.  The wide
// instantiations therefore share one copy of the tables between as many wavefronts as their registers allow on a SIMD:
// four (up to 128 VGPRs: P <= 12; T = 32 gets them as two workgroups of eight), three (up to 170: P = 13 ... 16) or two
// (T = 32, P >= 17: <32, 17> spills three registers under the limit of 170).
constexpr int vitpk_waves(int T, int P)
{
  if (T == 64) return P <= 12 ? 16 : 12;
  if (T == 32) return (P >= 13 && P <= 16) ? 12 : 8;
  return 4;
}

// Wavefronts per SIMD that an instantiation is compiled for (the second launch bound): left alone, the register allocator
// lands a few registers beyond a step of the occupancy table for some P and not for its neighbours (<8, 10> took 136
// registers, <8, 12> 126).  These are the steps that the row loop's 6P registers and its temporaries fit; where the
// step is tight (P = 8, 12, 17) one to three per-target values are spilled around the row loop, none inside it.
// T = 32, 64: what vitpk_waves puts on a SIMD.
constexpr int vitpk_simd_waves(int T, int P)
{
  if (T == 64) return P <= 12 ? 4 : 3;
  if (T == 32) return P <= 12 ? 4 : P <= 16 ? 3 : 2;
  return P <= 2 ? 8 : P <= 4 ? 7 : P <= 6 ? 6 : P <= 8 ? 5 : P <= 12 ? 4 : P <= 17 ? 3 : 2;
}

template <int T, int P>
__global__ void __launch_bounds__(64 * vitpk_waves(T, P), vitpk_simd_waves(T, P)) vitpk_kernel(const ArgRef ref)
{
  constexpr int G = 64 / T;                // targets per wavefront
  constexpr int NW = vitpk_waves(T, P), NT = 64 * NW;
  const VitPkArgs a = load_args<VitPkArgs>(ref);
  const int nlist = a.nlist_ptr ? *a.nlist_ptr : a.nlist;
  const int nskip = a.nskip_ptr ? *a.nskip_ptr : 0;         // the longest targets (a prefix of the list) go elsewhere
  if (nskip + (int) (blockIdx.x * NW * G) >= nlist) return;  // no target for this block: skip the table load
  constexpr int PS = (P + 3) & ~3;         // table stride per lane, in pairs
  constexpr int ROWQ = vitpk_rowq(T, P);   // uint4 per emission row (see vitpk_rowq)
  // LDS layouts are lane-minor, so that the 16-byte reads of the T lanes of a group (and of the groups of a
  // ds_read_b128 service group) fall on distinct 4-bank slots:
  //   tra / trb [P][T] uint4   (BM MM IM DM) / (MD MI II DD) of pair j, lane s (every group reads the same address)
  //   em        [nrows][ROWQ]  uint4 q*T + s = pairs 4q..4q+3 of lane s
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *tra = reinterpret_cast<uint4 *>(smem);
  uint4 *trb = tra + P * T;
  uint4 *em = trb + P * T;
  {
    const uint4 *gt = reinterpret_cast<const uint4 *>(a.trans);
    for (int i = threadIdx.x; i < 2 * P * T; i += NT) tra[i] = gt[i];
    const uint4 *ge = reinterpret_cast<const uint4 *>(a.emis);
    for (int i = threadIdx.x; i < a.nrows * ROWQ; i += NT) em[i] = ge[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int s = lane % T, g = lane / T;
  const bool first = (s == 0), hi = (g != 0);
  const int wave0 = rfl((int) (blockIdx.x * NW + (threadIdx.x >> 6)));
  const int nwaves = (int) gridDim.x * NW;
  const uint4 *tral = tra + s, *trbl = trb + s, *eml = em + s;
  for (int it0 = nskip + wave0 * G; it0 < nlist; it0 += nwaves * G) {
    const int it = it0 + g;
    const bool have = it < nlist;
    const int slot = have ? (a.list ? a.list[it] : it) : 0;
    const int L = have ? a.slot_len[slot] : 0;
    const uint8_t *sq = a.dsq + (have ? a.slot_off[slot] : 0);
    const int xwm = (int) a.xwmove_tab[L];
    const int Lmax = wave_max_i32(L);

    // Two register sets for the rows: a row reads one and writes the other, so the old M / I / D of a pair stay
    // where they are while the new ones are produced (one set would cost a register copy per pair and array per row)
    uint32_t mA[P], iA[P], dA[P], mB[P], iB[P], dB[P];
#pragma unroll
    for (int j = 0; j < P; ++j) mA[j] = iA[j] = dA[j] = kNeg2;
    RowState rs;
    rs.xN = a.base_w; rs.xB = rs.xN + xwm; rs.xJ = -32768; rs.xC = -32768; rs.overflow = false;

    for (int i0 = 0; i0 < Lmax; i0 += 4 * T) {
      // residues of the next 4T rows: lane s holds rows i0+4s .. i0+4s+3 of its target (clamped reads; rows past the
      // end of a target are masked below)
      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int r = i0 + 4 * s + b;
        const uint32_t x = (r < L) ? (uint32_t) sq[r] : 0u;
        word |= x << (8 * b);
      }
      const int nrow = min(4 * T, Lmax - i0);
      // The four residues of rows r .. r|3 come to the group from lane r/4 (one ds_bpermute); a pair of rows fetches the
      // word of the pair after it, so that no row's emission address waits for that round trip.
      auto fetch = [&](int r) -> uint32_t { return (uint32_t) __shfl((int) word, g * T + min(r >> 2, T - 1)); };
      auto residue = [](uint32_t w, int r) -> uint32_t { return (w >> (8 * (r & 3))) & 0xffu; };
      uint32_t w = fetch(0);
      int r = 0;
      for (; r + 1 < nrow; r += 2) {
        const uint32_t wn = fetch(r + 2);
        vit_row<T, P>(a, tral, trbl, eml + residue(w, r) * ROWQ, first, hi, i0 + r < L, xwm, mA, iA, dA, mB, iB, dB, rs);
        vit_row<T, P>(a, tral, trbl, eml + residue(w, r + 1) * ROWQ, first, hi, i0 + r + 1 < L, xwm, mB, iB, dB, mA, iA, dA, rs);
        w = wn;
      }
      if (r < nrow) {     // odd row count (only the last block of a group): one more row, then back into set A
        vit_row<T, P>(a, tral, trbl, eml + residue(w, r) * ROWQ, first, hi, i0 + r < L, xwm, mA, iA, dA, mB, iB, dB, rs);
#pragma unroll
        for (int j = 0; j < P; ++j) { mA[j] = mB[j]; iA[j] = iB[j]; dA[j] = dB[j]; }
      }
    }
    const bool overflow = rs.overflow; const int xC = rs.xC;
    if (have && s == 0) a.out_xC[it] = overflow ? 32767 : xC;
  }
}

// ---------------------------------------------------------------------------- host side
// The instantiations, X(T, P), by increasing model length 2 T P: vitpk_pick takes the first that holds the model,
// vitpk_launch dispatches on the same list.
#define P7X_VITPK_TILES(X) \
  X(8, 2) X(8, 4) X(8, 6) X(8, 8) X(8, 10) X(8, 12) X(8, 14) X(8, 15) X(8, 16) X(8, 17) X(8, 18) X(8, 19) X(8, 20) \
  X(16, 11) X(16, 12) X(16, 13) X(16, 14) X(16, 15) X(16, 16) X(16, 17) X(16, 18) X(16, 19) X(16, 20) \
  X(32, 11) X(32, 12) X(32, 13) X(32, 14) X(32, 15) X(32, 16) X(32, 17) X(32, 18) X(32, 19) X(32, 20) \
  X(64, 11) X(64, 12) X(64, 13) X(64, 14) X(64, 15) X(64, 16)

bool vitpk_pick(int M, int *T, int *P)
{
  const bool wide = debug_opt(OPT_VIT_WIDE) != 0;       // 0: A/B and test seam: models beyond 640 nodes stay with vit_kernel
#define P7X_PK(TT, PP) if (M <= 2 * TT * PP) { if (TT >= 32 && !wide) return false; *T = TT; *P = PP; return true; }
  P7X_VITPK_TILES(P7X_PK)
#undef P7X_PK
  return false;
}

// trans: uint4 [2][P][T] = (BM MM IM DM) then (MD MI II DD) of register j of lane s, each dword (node lo, node hi)
// = nodes j + 1 + s*P and j + 1 + (s+T)*P (Farrar striping over the 2T half-lanes of a group);
// emis: uint4 [nrows][ROWQ], q*T + s = pairs 4q .. 4q+3 of lane s.  Nodes beyond M and unused pairs hold -32768.
void vitpk_build_tables(const Profile &p, int T, int P, std::vector<uint32_t> &trans, std::vector<uint32_t> &emis)
{
  const int rowq = vitpk_rowq(T, P), nrows = p.Kp + 1;
  auto pack = [](int lo, int hi) { return ((uint32_t) lo & 0xffffu) | (((uint32_t) hi & 0xffffu) << 16); };
  trans.assign((size_t) 2 * P * T * 4, kNeg2);
  emis.assign((size_t) nrows * rowq * 4, kNeg2);
  for (int s = 0; s < T; ++s)
    for (int j = 0; j < P; ++j) {
      const int k0 = s * P + j + 1, k1 = (s + T) * P + j + 1;      // stripes s (low half) and s + T (high half)
      for (int t = 0; t < NTRANS; ++t) {
        const int lo = (k0 <= p.M) ? p.tw[(size_t) t * (p.M + 1) + k0] : -32768;
        const int hi = (k1 <= p.M) ? p.tw[(size_t) t * (p.M + 1) + k1] : -32768;
        trans[((size_t) (t / 4) * P * T + (size_t) j * T + s) * 4 + (t % 4)] = pack(lo, hi);
      }
      for (int x = 0; x < p.Kp; ++x) {
        const int lo = (k0 <= p.M) ? p.rw[(size_t) x * (p.M + 1) + k0] : -32768;
        const int hi = (k1 <= p.M) ? p.rw[(size_t) x * (p.M + 1) + k1] : -32768;
        emis[((size_t) x * rowq + (size_t) (j / 4) * T + s) * 4 + (j % 4)] = pack(lo, hi);
      }
    }
}

template <int T, int P>
static int launch_pk(const ArgRun<VitPkArgs> &a, int num_cu, hipStream_t st)
{
  const size_t lds = ((size_t) 2 * P * T + (size_t) a.at(0).nrows * vitpk_rowq(T, P)) * 16;
  auto kern = vitpk_kernel<T, P>;
  constexpr int NW = vitpk_waves(T, P), NT = 64 * NW;
  int per_cu = 0;
  const int pst = kernel_blocks_per_cu(kern, NT, lds, &per_cu);
  if (pst != P7X_OK) return pst;
  long want = 0;
  for (int i = 0; i < a.n; ++i) want = std::max<long>(want, ((long) a.at(i).nlist + NW * (64 / T) - 1) / (NW * (64 / T)));   // nlist bounds the list
  if (want <= 0) return P7X_OK;
  hipLaunchKernelGGL(kern, dim3(lane_grid(want, (long) num_cu * per_cu, a.n), (unsigned) a.n), dim3(NT), lds, st, a.ref());
  P7X_HIP(hipGetLastError());
  return P7X_OK;
}

int vitpk_launch(int T, int P, const ArgRun<VitPkArgs> &a, int num_cu, hipStream_t st)
{
  if (a.n <= 0) return P7X_OK;
#define P7X_PK(TT, PP) if (T == TT && P == PP) return launch_pk<TT, PP>(a, num_cu, st);
  P7X_VITPK_TILES(P7X_PK)
#undef P7X_PK
  set_error("no packed Viterbi kernel for this model length");
  return P7X_EINVAL;
}

} // namespace p7x

#ifdef P7X_VITPK_COUNT
// out[0..2]: rows of all wavefronts since the library was loaded, those that entered the pass loop (a target asked for
// the closure), passes of that loop (not part of the C-ABI: the symbol exists only in a build with the flag)
extern "C" int p7x_vitpk_row_counts(unsigned long long *out)
{
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(p7x::vitpk_row_counts), 3 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
