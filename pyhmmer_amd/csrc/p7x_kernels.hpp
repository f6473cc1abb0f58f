// p7x_kernels.hpp -- launch interfaces of the HIP kernels (one translation unit per kernel family).
#pragma once
#include <string>
#include <type_traits>
#include "p7x_device.hpp"

namespace p7x {

// ---- batched launches
// Every kernel of the cascade takes its arguments from DEVICE memory, one record per profile ("lane") of a batch of
// queries that run against the same resident target block: blockIdx.y selects the record, blockIdx.x walks that lane's
// work exactly as it did when a launch served one profile.  Records are <stride> bytes apart, so they can be members
// of a larger per-lane struct (LaneArgs in p7x_pipeline.hip).  One query alone is a batch of one.
struct ArgRef { const void *base; uint32_t stride; };
#if defined(__HIPCC__)
template <class A> __device__ __forceinline__ A load_args(const ArgRef r)
{ // constant address space: the record is not written while the kernel runs, so it is fetched with scalar loads
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) A *cptr;
  return *(cptr) (unsigned long long) (static_cast<const char *>(r.base) + (size_t) blockIdx.y * r.stride);
#else
  return *reinterpret_cast<const A *>(static_cast<const char *>(r.base) + (size_t) blockIdx.y * r.stride);   // host pass: never run
#endif
}
#endif
// A run of consecutive lanes that share one kernel instantiation: host copies of the records (for grid sizing) and
// the device copies the kernel reads.
template <class A> struct ArgRun {
  const A *host = nullptr; const void *dev = nullptr; uint32_t stride = 0; int n = 0;
  const A &at(int i) const { return *reinterpret_cast<const A *>(reinterpret_cast<const char *>(host) + (size_t) i * stride); }
  ArgRef ref() const { return ArgRef{ dev, stride }; }
};
// blocks per lane: <want> of them are expected to have work (every kernel walks its list with a grid-stride loop, so
// an estimate that is too low only costs balance, and blocks without work leave before they load their tables); at
// most what is resident at once per lane -- the lanes' blocks queue up behind each other
inline unsigned lane_grid(long want, long resident, int nlanes)
{
  (void) nlanes;
  if (want > resident) want = resident;
  return (unsigned) (want < 1 ? 1 : want);
}

// ... for a kernel whose wavefronts PULL their work items (the lane-per-target MSV kernels: an atomic counter per lane, longest
// groups first): with many lanes in a launch -- a scan's thousands of profiles against a few dozen 64-target groups -- a lane
// gets only as many blocks as it takes to keep the device twice subscribed, down to ONE: its wavefronts then balance the items
// among themselves (the longest group beside the sum of the short ones), where nine blocks of four wavefronts for 33 items give
// every wavefront one item and hold a CU for the longest of them (round 6: profiles/r06_scan_lane_blocks.txt).
inline unsigned lane_grid_pull(long want, long resident, int nlanes, bool old_rule)
{
  if (old_rule || nlanes < 32) return lane_grid(want, resident, nlanes);      // a few lanes with thousands of groups each (a search): as many blocks as are resident
  long b = (2 * resident + nlanes - 1) / nlanes;
  if (b > resident) b = resident;
  if (b > want) b = want;
  return (unsigned) (b < 1 ? 1 : b);
}

// ---- MSV (p7x_msv.hip)
struct MsvArgs {
  const uint32_t *tab;      // [2][kTabRows][S] dwords: parity 0 = "odd" alignment, parity 1 = "even"; K = 8: [kTabRows][S], one alignment
  const uint4 *tiles;
  const int64_t *grp_off;
  const int32_t *grp_nblk;
  const int32_t *slot_len;
  const uint8_t *tjb_tab;
  int ngroups;
  int group_first;          // groups below this one are left to the wave-per-target kernel (the longest targets)
  int base, bias, tec, tbm;
  int *counter;
  int16_t *out_xJ;          // [ngroups*64] slot order; -1 = overflow
  // fast variant: groups whose result is ambiguous are appended here and redone by the exact kernel
  int *amb_count; int *amb_groups; int *counter2;
  const int *group_list; const int *group_count;   // exact kernel: optional list of groups to process
  int R;                    // the lane's register tile (read by the tier kernels, which serve several tiles in one launch)
};
int  msv_pick(int M, int *K);       // row registers per lane and lanes per target (K = 1, 2, 4, 8) of the lane kernels; -1: none fits
int  msv_stride(int R, int K);     // dwords per table row
void msv_build_tables(const Profile &p, int R, int K, std::vector<uint32_t> &out);
// fast kernel over <main> followed by the exact kernel over each lane's list of ambiguous groups (<amb>: records with
// group_list / group_count set); amb == nullptr: the exact kernel over every group of <main>
int  msv_launch(int R, int K, const ArgRun<MsvArgs> &main, const ArgRun<MsvArgs> *amb, int num_cu, hipStream_t st);
// The fast kernel for the lanes of several register tiles in one launch (half-float flavour), and the exact kernel over the
// ambiguous groups of one tile's lanes afterwards.  msv_tier: the tier a tile belongs to (0..kMsvTiers-1); lanes of a
// launch must share it.
constexpr int kMsvTiers = 6;
int  msv_tier(int R, int K);
int  msv_tier_launch(int tier, const ArgRun<MsvArgs> &main, int num_cu, hipStream_t st);
int  msv_exact_launch(int R, int K, const ArgRun<MsvArgs> &amb, int num_cu, hipStream_t st);

// ---- wave-per-sequence stages (p7x_vitfwd.hip): Viterbi filter, Forward / Backward parsers
// Node k = z*C + c + 1 lives in lane z, chunk position c; device tables are stored [c*64 + z].
// The tiers of C, nodes per lane, that the wave-per-sequence kernels, the envelope / alignment kernel and the ensemble
// fill are instantiated for (M <= 64 C; the last one bounds the model length: max_model_length()): every dispatch on C and
// vit_pick_C() expand this list.  Beyond 128 nodes per lane (M > 8192: sequence queries, phmmer) the steps are wide -- such
// models are a handful per proteome and every tier is another instantiation of every kernel: 192 (M <= 12,288).  The list
// ends where the runtime still grants env_kernel's scratch memory: tiers of 320 and 576 were refused on the MI355X.
#define P7X_NODE_TIERS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(8) X(10) X(12) X(16) X(20) X(24) X(32) X(48) X(64) X(96) X(128) X(192)
// the longest model the device kernels take: 64 x the last tier (p7x_max_model_length() of p7x.h)
int max_model_length();
// "<what> (M > max_model_length() nodes)": the text of every refusal of a model for its length
std::string model_too_long(const char *what);
// f(std::integral_constant<int, C>()) where C is a tier (f picks and launches its kernel's instantiation for it), else
// the error model_too_long(<too_long>)
template <class F> int node_tier_dispatch(int C, const char *too_long, F &&f)
{
  switch (C) {
#define P7X_TIER_CASE(CC) case CC: return f(std::integral_constant<int, CC>());
    P7X_NODE_TIERS(P7X_TIER_CASE)
#undef P7X_TIER_CASE
    default: set_error(model_too_long(too_long)); return P7X_EINVAL;
  }
}
struct WaveSeqArgs {
  int M, C;                 // C = nodes per lane, Mpad = 64*C
  const void *trans;        // Viterbi: uint4[Mpad] (8 x int16); Forward: float4[2*Mpad] (8 x f32)
  const void *emis;         // Viterbi: int16[kTabRows][Mpad]; Forward: float[kTabRows][Mpad]
  const uint8_t *dsq;       // sentinel-framed residues
  const int64_t *slot_off;  // [nslots] offset of x1
  const int32_t *slot_len;
  const int32_t *list;      // slots to process (NULL: 0..nlist-1)
  int nlist;
  const int *nlist_ptr;     // if non-NULL the list length is read from device memory (no host sync between stages)
  const int *abort_flag;    // optional: non-zero on the device = skip all work (buffers not sized for this list)
  int nrows;                // residue rows in the emission table (Kp + 1)
  int *counter;
  // Viterbi
  const int16_t *xwmove_tab; int base_w, xw_e, ddbound;
  int32_t *out_xC;          // [nlist]
  // Viterbi, long-target variant (p7_ViterbiFilter_longtarget): a row whose best match cell reaches the item's score
  // threshold is recorded (item, row, node: one record per cell holding that score) and the DP rows are cleared
  const int *lt_thresh;     // [nlist] per item; NULL: the standard filter
  int *lt_nrec; int *lt_rec; int lt_cap;      // records [cap][3]
  // Forward / Backward
  float xf_e_move, xf_e_loop;
  float *out_sc;            // [nlist] nats
  float *xmx;               // optional [sum (L+1)*6]; rows E,N,J,B,C,SCALE
  const int64_t *xmx_off;   // [nlist] float offset of each target's block
  const float *fwd_xmx;     // Backward only: Forward's blocks (for the scale factors)
};
int vit_pick_C(int M);
// Dynamic LDS of the wave-per-target layouts (the search, envelope / alignment and calibration kernels index LDS by them).
// Viterbi filter: the transitions, 16 bytes per node (M > 8192: read through L2), and the emission rows up to M = 2048
inline size_t vit_lds_bytes(int C, int nrows) { return C > 128 ? (size_t) 256 : (size_t) 64 * C * (16 + (C <= 32 ? nrows * 2 : 0)); }
// Parsers and envelopes: the transitions, 32 bytes per node (M > 4096: read through L2), and, where <emis>, the emission rows
// while they fit beside them (M <= 1024: the instantiations without EG)
inline size_t fwd_lds_bytes(int C, int nrows, bool emis = true) { return C > 64 ? (size_t) 256 : (size_t) 64 * C * (32 + (emis && C <= 16 ? (size_t) nrows * 4 : 0)); }
// MSV, one target per wavefront: the emission rows up to M = 2048
inline size_t msv_wave_lds_bytes(int C, int nrows) { return C > 32 ? (size_t) 256 : (size_t) 64 * C * nrows * 2; }
// every record of a run has the same C (and nrows); nlist of the host copies bounds the lists and sizes the grid
int vit_launch(const ArgRun<WaveSeqArgs> &a, int num_cu, hipStream_t st);
int fwd_launch(const ArgRun<WaveSeqArgs> &a, int num_cu, hipStream_t st);
// grouped Forward parser, scores only (p7x_fwdpk.hip): WaveSeqArgs::C = T * 256 + C, trans / emis in its own layout
bool fwdg_pick(int M, int vitC, int *T, int *C);
int fwdg_launch(const ArgRun<WaveSeqArgs> &a, int num_cu, hipStream_t st);
void fwdg_build_tables(const Profile &p, int T, int C, std::vector<float> &trans, std::vector<float> &emis);
int bck_launch(const ArgRun<WaveSeqArgs> &a, int num_cu, hipStream_t st);

// ---- MSV for models beyond the register-resident kernels (p7x_vitfwd.hip::msv_wave_kernel), every tier of P7X_NODE_TIERS
struct MsvWaveArgs {
  int C, nrows;
  const void *emis;         // int16 [nrows][64*C], (bias - cost) in lane-chunk order, kNegPad outside the model / pad row
  const void *emis_pk;      // long models (C >= 20): the same as packed pairs, [nrows][C/4][64] x (pair, pair) for msv_wavepk_kernel
  const uint8_t *dsq; const int64_t *slot_off; const int32_t *slot_len; const uint8_t *tjb_tab;
  int nslots, base, bias, tec, tbm;
  int16_t *out_xJ;
};
int msv_wave_launch(const ArgRun<MsvWaveArgs> &a, int num_cu, hipStream_t st);

// ---- packed Viterbi filter (p7x_vitpk.hip): T lanes per target, 2P nodes per lane, for M <= 2048
struct VitPkArgs {
  const void *trans, *emis;     // vitpk_build_tables()
  const uint8_t *dsq; const int64_t *slot_off; const int32_t *slot_len;
  const int32_t *list; int nlist; const int *nlist_ptr;     // as WaveSeqArgs
  const int *nskip_ptr;     // optional: the first *nskip_ptr list items are left to the wave-per-target kernel
  int nrows;
  const int16_t *xwmove_tab; int base_w, xw_e, ddbound;
  int32_t *out_xC;
};
bool vitpk_pick(int M, int *T, int *P);
void vitpk_build_tables(const Profile &p, int T, int P, std::vector<uint32_t> &trans, std::vector<uint32_t> &emis);
int  vitpk_launch(int T, int P, const ArgRun<VitPkArgs> &a, int num_cu, hipStream_t st);

// ---- envelope rescoring and hmmalign (p7x_envkernel.hpp, instantiated by p7x_envelope.hip and p7x_align.hip): Forward + Backward + decoding/null2/optimal accuracy + traceback,
// one domain envelope per wavefront.  Trace steps come back in traceback order (T first): tr_a = state | k << 8,
// tr_i = residue index inside the envelope (1..Ld, as the traceback saw it), tr_pp = posterior of that step.
struct EnvArgs {
  int M, C, K, nrows;       // K: canonical residues (null2 vector length); nrows: residue rows of the emission table
  const void *trans;        // Forward tables of the profile (float4[2*Mpad], float[nrows][Mpad])
  const void *emis;
  const uint8_t *dsq;
  float nj, xf_e_move, xf_e_loop;   // unihit: 0, 1, 0
  int nenv;
  const int64_t *env_sq;    // [nenv] offset in dsq of the first residue of the envelope
  const int32_t *env_len;   // [nenv] envelope length Ld
  const int32_t *env_L;     // [nenv] full target length (the length model is not re-configured per envelope)
  const int32_t *order;     // [nenv] envelopes by decreasing length: the order in which wavefronts draw them
  int *cursor;              // the job's queue position (zero at launch)
  float *work; int64_t work_stride; int Lmax;    // per-wavefront workspace (env_work_floats), rows 0..Lmax
  int nblocks, slab_base;   // blocks of this job (blockIdx.x beyond them exit); first workspace slab of the job
  float *out_sc;            // [nenv][2] envelope Forward score (nats), optimal accuracy score
  const float *env_emis;    // long-target envelopes: per-envelope match odds [nenv][nrows][Mpad] (NULL: the profile's own table)
  long long env_emis_stride;  // floats per envelope table
  float *out_orig;          // long-target envelopes: [nenv] Forward score with the profile's unmodified odds
  float oa_guard;           // near-tie guard of the optimal-accuracy traceback (p7x_pipeline_cfg.oa_guard)
  int32_t *out_status;      // [nenv] bit 0 Forward range, 1 decoding range (envelope dropped), 2-5 traceback failures,
                            // 6 a near-tie on the trace: the host stage repeats the envelope in the reference's order
                            // (bits 8-15 say where: M / I / D cell choice, C<-E, J<-E, end cell, B<-N/J, posterior digit)
  float *out_null2;         // [nenv][32] null2 odds of the canonical residues
  const int64_t *tr_off;    // [nenv] first trace element; capacity Ld + M + 16 each
  uint32_t *tr_a; int32_t *tr_i; float *tr_pp;
  int32_t *tr_n;            // [nenv] trace length
};
// wavefronts (= envelopes in flight) per block of env_kernel: eight (two per SIMD, 256 registers each); from eight
// nodes per lane on, four (one per SIMD, 512 registers): the row state of two would spill to scratch, which made the
// envelopes of long models 1.4-3.6x slower than half the occupancy does (scripts/env_by_length.py)
constexpr int env_waves(int C) { return C >= 8 ? 4 : 8; }
// What env_kernel is instantiated for: a protein envelope; a long-target envelope (EnvArgs::env_emis, out_orig); hmmalign:
// the four steps over whole sequences (env_len = env_L), float posteriors on the trace, no null2
enum class EnvMode { Envelope, LongTarget, Align };
// floats per wavefront of EnvArgs::work, every mode: the carving at the top of env_kernel
inline size_t env_work_floats(int C, int Lmax)
{
  const size_t rows = (size_t) Lmax + 1, Mpad = (size_t) 64 * C;
  size_t f = 2 * rows * Mpad + rows * (6 + 6 + 5 + 3 + 1);
  f += (rows * Mpad + 1) / 2;          // back-pointers, near-tie flags and posterior digits: 16 bits per cell
  return (f + 63) & ~(size_t) 63;
}
// Align: as the envelope modes, through align_max_blocks / align_launch of p7x_align.hip
int env_max_blocks(EnvMode mode, int C, int nrows, int num_cu, int *nblocks);
// every record of the run has the same C, nrows and mode; grid.x = the widest job's nblocks
int env_launch(EnvMode mode, const ArgRun<EnvArgs> &a, hipStream_t st);
// Half-width of the guard band around a PP digit boundary, in posterior units.  The device's float posteriors differ from
// the host twin's by an error that grows with the model (at most 1.25e-6 for the fixture models of <= 262 nodes against the
// proteome, 7.5e-6 at M = 6,000; about 1e-9 M): the band is at least three times that, and never below 1e-5.  A residue on
// the trace whose posterior lies within it flags the sequence (kernel); a PP_cons column whose mean does is averaged
// again over host-twin posteriors (p7x_tracealign.cpp).
__host__ __device__ inline float align_pp_guard(int M) { return 1.0e-5f + 2.5e-9f * (float) M; }
// The band of pp_code_guarded() (p7x_oaguard.hpp) around a PP digit boundary, in units of 10 p + 0.5, that this guard makes
__host__ __device__ inline float align_pp_band(int M) { return 0.5f - 10.0f * align_pp_guard(M); }
int align_max_blocks(int C, int nrows, int num_cu, int *nblocks);
int align_launch(const ArgRun<EnvArgs> &a, hipStream_t st);

// ---- stochastic traceback ensembles of multi-domain regions (p7x_ensemble.hip; upstream p7_domaindef.c
// region_trace_ensemble): a multihit Forward fill of the region that leaves, per cell and per row, the integer
// thresholds of every choice a stochastic traceback can face there (p7x_choice.hpp), then one wavefront per region that
// walks the region's tracebacks through those records, consuming the region's single generator stream.
struct ChoiceCell; struct ChoiceRow;
struct EnsRegion {          // one multi-domain region, as both kernels see it
  int64_t sq;               // offset in dsq of the region's first residue
  int64_t cell0;            // first cell record: (Lr + 1) rows of M + 1 cells, row-major, node-minor (node 0 unused)
  int64_t row0;             // first row record; rows 0 .. Lr.  The null2 accumulators use the same offsets
  int64_t dom0;             // first domain record of the region's output
  int32_t Lr, L;            // region length; full target length (the length model)
  int32_t job, dom_cap;     // the profile; room for this many domain records at dom0
};
struct EnsJob {             // per query profile
  int M, C, K, Kp, nrows, Q;          // Q = p7O_NQF(M): select_e walks the reference's striped order
  const void *trans, *emis;           // Forward tables of the device image
  const float *rft;                   // [M + 1][32] match odds, residue-minor (p7_Null2_ByTrace)
  const uint8_t *degen;               // [32][32] degeneracy matrix of the alphabet (esl_abc_FAvgScVec)
  int reg_first, nreg;                // the job's regions in EnsArgs::regions
};
struct EnsArgs {
  const EnsJob *jobs; const EnsRegion *regions; int nregions;
  const uint8_t *dsq;
  ChoiceCell *cells; float2 *md; ChoiceRow *rows;      // md: Forward's M and D cell (select_e)
  uint32_t seed_x;          // the generator's state after esl_randomness_Init(seed): every region starts there
  int nsamples;
  float *n2acc;             // [rows] per residue: sum over the samples of the null2 odds ratio (1 outside domains)
  int32_t *dom;             // [5] per domain: sample, sqfrom, sqto (1-based inside the region), hmmfrom, hmmto
  int32_t *out_ndom; int32_t *out_status;               // per region
  int lds_bytes;            // dynamic LDS of the walk kernel: what fits of a region's row records, accumulators and odds table lives there
  uint32_t guard;           // near-threshold guard of the walk, in units of the generator's 2^-32 (p7x_pipeline_cfg.ens_guard x 2^32); 0: off
};

// ---- long-target SSV scan (p7x_ssvlong.hip): one chunk of one strand per wavefront, model split across the lanes
struct SsvLongArgs {
  const uint32_t *tab4q;      // [2 parities][4][(R+3)/4][64] uint4: quads of packed emission pairs of A, C, G, T (staged in LDS)
  const uint32_t *tab_full;   // [2][Kp][R][64] the pairs of every residue code (degenerate residues, read from global memory)
  const uint8_t *dsq;         // the target, 1-based (dsq[0] is a sentinel)
  const uint8_t *comp;        // [Kp] complement of every residue code
  int pair_slack;             // the most a cell can lose in one row with a canonical residue (byte units)
  const long long *chunk_list;  // NULL: every chunk; else the nchunks chunk numbers to scan (a part of a search dealt over devices)
  long long L;                // target length
  int M, Kp;
  int chunk_len;              // rows per chunk
  long long chunks_per_strand, nchunks;     // nchunks = strands x chunks_per_strand; chunk c of strand strand0 + c / chunks_per_strand
  int strand0;                // 1: only the reverse-complement strand is scanned
  int thresh_s;               // score threshold, relative to the begin score and offset by -32768 (the cells' representation)
  int xB, Q16;                // the begin score in byte units; vectors per row of the reference's striped layout (tie-breaks)
  // rows that reach the threshold: position on the strand, strand, and the cell upstream would pick (node, byte score)
  int *nrec; long long *rec_pos; uint8_t *rec_strand; int *rec_k; int *rec_sc; int rec_cap;
  // a scan in chained parts (a model of more nodes than one launch holds; read by the boundary instantiations only, M, Q16 and
  // pair_slack stay the whole model's): the part's nodes are node0 + 1 .. node0 + nloc, its tables are built for them
  int node0, nloc;
  int out_lane;               // boundary-out: the part's last node is the top register's cell of this lane (high half on odd rows, low on even ones)
  unsigned short *bnd;        // [nchunks][bnd_stride] the native 16-bit cell of the cut node after every row of a chunk, warm-up included:
  long long bnd_stride;       //   written by a part with a successor, read (and overwritten in place) by the next one
  long long chunk0;           // no chunk_list: the launch scans chunks chunk0 .. chunk0 + nchunks - 1 (a round of a scan in parts)
};
// <pair>: the row maximum only on every second row, against a threshold lowered by pair_slack, tables with the virtual node
int  ssvlong_pick_R(int M, bool pair);
// The parts of a scan: nodes lo .. hi with R packed registers per lane.  A part with a successor ends on node
// lo + 2 R t - 3 for a lane t - 1 (out_lane): there its last cell is the top register's in both row parities.
struct SsvPart { int lo, hi, R, out_lane; };
// The fewest parts that hold M nodes (parts_forced = 2 .. 4: that many, if the model has two nodes for each and they hold
// it), among those the smallest R, parts as equal as that R allows; one part: { 1, M, ssvlong_pick_R(M, pair) }.  Empty: M is
// beyond max_model_length().
std::vector<SsvPart> ssvlong_plan(int M, bool pair, int parts_forced);
// tables of nodes lo .. hi (hi = 0: the whole model); <pair>: with the virtual node hi + 1
void ssvlong_build_tables(const Profile &p, int R, bool pair, std::vector<uint32_t> &tab4q, std::vector<uint32_t> &tab_full, int *pair_slack, int lo = 1, int hi = 0);
int  ssvlong_capacity(int R, bool pair, bool half, int num_cu, long long *waves);      // half: binary16 cells (the default), else int16
// <bin> / <bout>: the part takes its cell 0 from the boundary buffer / leaves its last cell there
int  ssvlong_launch(int R, bool pair, bool half, const SsvLongArgs &a, int num_cu, hipStream_t st, bool bin = false, bool bout = false);

// ---- the batched long-target SSV scan (p7x_ssvlong.hip; nhmmscan): one target, many models, a model per blockIdx.y.
// What a block reads of its model.  Every model of a launch has the launch's R, rows (PAIR) and cells (H).
struct SsvModelRec {
  long long tab4q_off;        // of its quads in SsvMultiArgs.tab4q, in uint4 (2 x 4 x ceil(R/4) x 64 of them)
  long long full_off;         // of its full table in SsvMultiArgs.tab_full, in dwords ([2][Kp][R][64])
  long long chunks_per_strand;
  int M, Q16;
  int thresh_s, xB;           // as in SsvLongArgs
  int pair_slack;
  int chunk_len;              // rows per chunk of this model: any multiple of 64 (the warm-up is M rows whatever it is)
  int index;                  // the model's number in the batch: what its rows are labelled with
  int pad_;
};
struct SsvMultiArgs {
  const uint32_t *tab4q, *tab_full;     // the tables of every model of the library, end to end
  const SsvModelRec *models;            // [gridDim.y] the models of this launch
  const uint8_t *dsq, *comp;            // the target (1-based) and the complement table: shared by all blocks
  long long L;
  int Kp, nstrands, strand0;            // chunk c of a model is on strand strand0 + c / chunks_per_strand
  int *nrec; long long *rec_pos; uint8_t *rec_strand; int *rec_k; int *rec_sc; int *rec_model; int rec_cap;      // one counter per scan
};
// one launch: <nmodels> models (at most 65,535) whose longest chunk list has <max_chunks> entries
int  ssvlong_multi_launch(int R, bool pair, bool half, const SsvMultiArgs &a, int nmodels, long long max_chunks, int num_cu, hipStream_t st);
int  ssvlong_multi_capacity(int R, bool pair, bool half, int num_cu, long long *waves);
size_t ssvlong_lds_bytes(int R);         // dynamic LDS of both scan kernels with R registers per lane
int  ssvlong_tile_count();               // the kernels' register tiles, ascending
int  ssvlong_tile(int i);

// ---- thread-per-sequence small stages (p7x_pipeline.hip)
} // namespace p7x
