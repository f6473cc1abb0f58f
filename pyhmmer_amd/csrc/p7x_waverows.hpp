// p7x_waverows.hpp -- the row bodies of the wave-per-target recurrences, each written once: one wavefront scores one
// sequence, lane z owns nodes zC+1 .. zC+C, the tables are stored [c*64 + lane], and the row state lives in registers.
//   ForwardRow<C, U, State>   p7_Forward (impl_sse/fwdback.c): env_kernel and ens_forward_kernel (U = unroll_env(C), the
//                             state its own), fwd_kernel and cal_fwd_kernel (U = unroll_c(C), over the kernel's arrays).  The
//                             host twin's forward_lanes() (p7x_domaindef.cpp) performs the same operations in the same
//                             order; what is decided from these values is decided alike on both sides.
//   vit_init / vit_restart / vit_cells / vit_finish   p7_ViterbiFilter (impl_sse/vitfilter.c): vit_kernel, cal_vit_kernel.
//   msv_init / msv_held / msv_step                    p7_MSVFilter (impl_sse/msvfilter.c): msv_wave_kernel, cal_msv_kernel.
// In the filter and calibration kernels the cell rows are the kernel's own arrays, taken by reference, with the special states
// in a small record next to them: everything is inlined, so the arrays stay the separate objects the compiler keeps in
// registers.  One object holding arrays and scalars together goes to scratch memory as a whole in the rolled instantiations
// (C > 32) and cost registers in others (profiles/r21_waverows.md); the envelope and ensemble kernels have always held
// Forward's state that way and go on doing so (ForwardOwn), which keeps their code what it was.  A kernel keeps what is its
// own: where the tables lie, its work items and length model, what it stores.  The units are built with -ffp-contract=off, so
// every user of a row computes the same bits.
#pragma once
#include "p7x_wave.hpp"

namespace p7x {

// node loops of the envelope kernel: unrolled (row state in registers) up to this many nodes per lane, rolled beyond
#ifndef P7X_ENV_UNROLL_MAX
#define P7X_ENV_UNROLL_MAX 32
#endif
constexpr int unroll_env(int C) { return C <= P7X_ENV_UNROLL_MAX ? C : 1; }

// ======================================================================================= Forward
// float, probability space, upstream's sparse rescaling (xE > 1e4); D->D is an affine scan over the lanes.  The envelope
// kernel runs the row for the envelope score and the per-row scale factors in phase 1 and AGAIN next to the decoding in
// phase 3 (same code, same operations in the same order: bit-identical values), which is what lets it park only Backward's
// rows in HBM.
// State: the cell rows held (ForwardOwn) or the caller's arrays (ForwardRefs: `float mm[C], im[C], dm[C];
// ForwardRow<C, U, ForwardRefs<C>> f{{mm, im, dm}};`), then ddprod -- the product of this lane's D->D probabilities, the
// multiplier of an incoming D carry -- and the special states; scale is the factor the last row was divided by.
// U: the unroll factor of the node loops.  TV: a TransView, by value (through a reference the compiler no longer sees at once
// which memory its pointer names, and fwd_kernel needs more registers).
template <int C> struct ForwardOwn  { float mm[C], im[C], dm[C]; float ddprod; float xN, xB, xJ, xC, xE, scale, totscale; };
template <int C> struct ForwardRefs { float (&mm)[C], (&im)[C], (&dm)[C]; float ddprod; float xN, xB, xJ, xC, xE, scale, totscale; };
template <int C, int U, class State = ForwardOwn<C>>
struct ForwardRow : State {
  using State::mm; using State::im; using State::dm; using State::ddprod;
  using State::xN; using State::xB; using State::xJ; using State::xC; using State::xE; using State::scale; using State::totscale;
  template <class TV>
  __device__ __forceinline__ void init(const TV tr, int lane, float pmove)
  {
#pragma unroll U
    for (int c = 0; c < C; ++c) mm[c] = im[c] = dm[c] = 0.0f;
    ddprod = 1.0f;
#pragma unroll U
    for (int c = 0; c < C; ++c) ddprod *= tr.dd(c * 64 + lane);
    xN = 1.0f; xB = pmove; xJ = 0.0f; xC = 0.0f; xE = 0.0f; scale = 1.0f; totscale = 0.0f;
  }
  template <class TV>
  __device__ __forceinline__ void row(const TV tr, const float *em, int Mpad, int lane, int x, float pmove, float ploop,
                                      float xf_e_move, float xf_e_loop)
  {
    const float *er = em + x * Mpad + lane;
    float mp = dpp_shr1f(mm[C - 1], 0.0f), ip = dpp_shr1f(im[C - 1], 0.0f), dp = dpp_shr1f(dm[C - 1], 0.0f);
    float esum = 0.0f;
    float t_dd[C], t_md[C];
#pragma unroll U
    for (int c = 0; c < C; ++c) {
      const F8 t = tr.at(c * 64 + lane);
      float sv = xB * t.bm;
      sv = sv + mp * t.mm;
      sv = sv + ip * t.im;
      sv = sv + dp * t.dm;
      sv = sv * er[c * 64];
      esum = esum + sv;
      mp = mm[c]; ip = im[c]; dp = dm[c];
      im[c] = mp * t.mi + ip * t.ii;
      mm[c] = sv;
      t_dd[c] = t.dd; t_md[c] = t.md;
    }
    // D(i,k) = M(i,k-1) tMD(k-1) + D(i,k-1) tDD(k-1): serial inside the lane, affine scan across the lanes
    float A = 0.0f;                                     // this lane's outgoing carry for a zero incoming carry
#pragma unroll U
    for (int c = 0; c < C; ++c) { dm[c] = A; A = mm[c] * t_md[c] + A * t_dd[c]; }
    float sa = A, sp = ddprod;                          // inclusive scan of (carry, multiplier)
    affine_scan_up(sa, sp);
    {
      float w = dpp_shr1f(sa, 0.0f);                    // exclusive: the carry entering this lane
#pragma unroll U
      for (int c = 0; c < C; ++c) { dm[c] = dm[c] + w; esum = esum + dm[c]; w = w * t_dd[c]; }
    }
    xE = wave_sum_f32(esum);
    xN = xN * ploop;
    xC = (xC * ploop) + (xE * xf_e_move);
    xJ = (xJ * ploop) + (xE * xf_e_loop);
    xB = (xJ * pmove) + (xN * pmove);
    scale = 1.0f;
    if (xE > 1.0e4f) {
      xN = xN / xE; xC = xC / xE; xJ = xJ / xE; xB = xB / xE;
      const float inv = (float) (1.0 / (double) xE);
#pragma unroll U
      for (int c = 0; c < C; ++c) { mm[c] *= inv; dm[c] *= inv; im[c] *= inv; }
      scale = xE;
      totscale = (float) ((double) totscale + log((double) xE));        // float += double, as upstream (and the host twin) has it
      xE = 1.0f;
    }
  }
};

// Forward's score after the last of L rows: NaN stays NaN, a C state that ran to zero or to infinity is out of range (+inf).
// (env_kernel makes a two-way choice of its own from the same values: there a NaN is out of range too, and its status word
// says so.)
__device__ __forceinline__ float forward_score(float xC, float totscale, float pmove, int L)
{
  if (xC != xC) return __builtin_nanf("");
  if ((L > 0 && xC == 0.0f) || __builtin_isinf(xC)) return __builtin_inff();
  return (float) ((double) totscale + log((double) (xC * pmove)));
}

// ======================================================================================= Viterbi filter
// int16 with saturating adds (v_add_i16 clamp), as upstream.  D->D is serial inside the lane; across the lanes HMMER's
// lazy-F test (Dmax + ddbound > xB) decides whether a D->D path can beat B->M on the next row at all, and then the chunk
// carries are relaxed until no lane improves -- a fixed point of max-plus, hence bit-identical to the serial evaluation.
// A row is vit_cells() then vit_finish(): vit_kernel's long-target branch sits between the row maximum and the special states.
struct ViterbiSpecials {
  int xN, xB, xJ, xC;
  short dmax;                        // this lane's largest M->D of the row, kept for the lazy-F test
  bool overflow;
  __device__ __forceinline__ int score() const { return overflow ? 32767 : xC; }
};
constexpr short kVitNeg = (short) -32768;

template <int C>
__device__ __forceinline__ void vit_restart(short (&mm)[C], short (&im)[C], short (&dm)[C])
{
#pragma unroll unroll_c(C)
  for (int c = 0; c < C; ++c) mm[c] = im[c] = dm[c] = kVitNeg;
}

template <int C>
__device__ __forceinline__ void vit_init(short (&mm)[C], short (&im)[C], short (&dm)[C], short (&tdd)[C], ViterbiSpecials &s, int base_w, int xwm)
{
#pragma unroll unroll_c(C)
  for (int c = 0; c < C; ++c) { mm[c] = im[c] = dm[c] = kVitNeg; tdd[c] = kVitNeg; }
  s.xN = base_w; s.xB = s.xN + xwm; s.xJ = -32768; s.xC = -32768;
  s.overflow = false;
}

// the cells of one row; tr: the transitions [Mpad], er: the emission row of the residue, from this lane's first node.  Returns xE.
template <int C>
__device__ __forceinline__ int vit_cells(short (&mm)[C], short (&im)[C], short (&dm)[C], short (&tdd)[C], ViterbiSpecials &s,
                                         const uint4 *tr, const short *er, int lane)
{
  const short NEG = kVitNeg;
  const short xBs = (short) s.xB;
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
  s.dmax = dmax;
  return wave_max_i32((int) rowmax);
}

// the special states of the row and the D->D closure; xw[C][LOOP] = xw[J][LOOP] = xw[N][LOOP] = 0
template <int C>
__device__ __forceinline__ void vit_finish(short (&dm)[C], const short (&tdd)[C], ViterbiSpecials &s, int xE, int xw_e, int xwm, int ddbound)
{
  const short NEG = kVitNeg;
  if (xE >= 32767) s.overflow = true;
  s.xC = max(s.xC, xE + xw_e);
  s.xJ = max(s.xJ, xE + xw_e);
  s.xB = max(s.xJ + xwm, s.xN + xwm);

  const int Dmax = wave_max_i32((int) s.dmax);
  if (Dmax + ddbound > s.xB) {            // lazy F: only now can a D->D path beat B->M on the next row
#pragma unroll unroll_c(C)
    for (int c = 1; c < C; ++c) dm[c] = max16(dm[c], adds16(dm[c - 1], tdd[c - 1]));
    for (int pass = 0; pass < 64; ++pass) { // a carry can cross at most 63 lane boundaries
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

// ======================================================================================= MSV
// int arithmetic with the u8 semantics of impl_sse/msvfilter.c reproduced as in msv_kernel (p7x_msv.hip): the floor at 0
// is implied by the next row's max(., xB); the 255 clip can only follow a row that already reported overflow.
struct MsvSpecials {
  int xJ, xEmax, xB;
  // the filter's result: -1 where a row overflowed the byte range
  __device__ __forceinline__ int score(int bias) const { return (xEmax >= 255 - bias) ? -1 : xJ; }
};

template <int C>
__device__ __forceinline__ void msv_init(int (&mm)[C], MsvSpecials &s, int base, int tjbm)
{
#pragma unroll unroll_c(C)
  for (int c = 0; c < C; ++c) mm[c] = 0;
  s.xJ = 0; s.xEmax = 0;
  s.xB = max(base - tjbm, 0);
}

// one row with xB held and nothing across the lanes but the one-lane shift; its maximum goes into this lane's <acc>.
// er: the emission row of the residue, from this lane's first node
template <int C>
__device__ __forceinline__ void msv_held(int (&mm)[C], int xB, const short *er, int &acc)
{
  int mp = dpp_shr1(mm[C - 1], 0);
#pragma unroll unroll_c(C)
  for (int c = 0; c < C; ++c) {
    const int sv = max(mp, xB) + (int) er[c * 64];
    mp = mm[c];
    mm[c] = sv;
    acc = max(acc, sv);
  }
}

// one row as the recurrence is written: the reduction of its maximum, then the special states
template <int C>
__device__ __forceinline__ void msv_step(int (&mm)[C], MsvSpecials &s, const short *er, int base, int tec, int tjbm)
{
  int rowmax = kNegPad;
  msv_held(mm, s.xB, er, rowmax);
  const int xE = wave_max_i32(rowmax);
  s.xEmax = max(s.xEmax, xE);
  s.xJ = max(s.xJ, xE - tec);
  s.xB = max(max(base, s.xJ) - tjbm, 0);
}

} // namespace p7x
