/* p7x.h -- C ABI of libp7x, the MI355X-native replacement for the libhmmer calls that
 * pyhmmer's plan7.Pipeline makes on its hot path.
 *
 * Every entry point cites the reference interface it replaces (paths relative to the
 * pyhmmer tree, v0.12.3).  Plain pointers and sizes only: no torch types, no C++ types.
 * All functions return an Easel-style status (include/libeasel/__init__.pxd:29-58):
 *   P7X_OK 0, P7X_EINVAL 11 (-> MissingCutoffs, plan7.pyx:6424-6425), P7X_ERANGE 16
 *   (-> OverflowError, plan7.pyx:6445-6446), anything else -> UnexpectedError (plan7.pyx:6447-6448).
 * P7X_ENODEVICE is returned -- never a CPU fallback -- when a device entry point is called
 * and no HIP device is usable.
 *
 * Ownership: inputs are borrowed for the duration of the call (as plan7.pyx:5116-5119);
 * handles returned by *_create() are owned by the caller and released with *_destroy().
 * Thread-safety: one p7x_pipeline per host thread (as hmmer/_base.py:324-325); profiles and
 * sequence databases are immutable after creation and may be shared between pipelines
 * (the per-target length model is computed inside the kernels instead of mutating the
 * profile as p7_oprofile_ReconfigLength does, plan7.pyx:6438).
 */
#ifndef P7X_H
#define P7X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P7X_ABI_VERSION 8

enum {
  P7X_OK = 0, P7X_EMEM = 5, P7X_EFORMAT = 7, P7X_EINVAL = 11, P7X_ERANGE = 16, P7X_ENORESULT = 19,
  P7X_ENODEVICE = 100, P7X_EDEVICE = 101
};

enum { P7X_RNA = 1, P7X_DNA = 2, P7X_AMINO = 3 };                 /* libeasel/alphabet.pxd */
enum { P7X_SEARCH_SEQS = 0, P7X_SCAN_MODELS = 1 };                /* p7_pipeline.pxd:26-28 */
enum { P7X_ZSETBY_NTARGETS = 0, P7X_ZSETBY_OPTION = 1, P7X_ZSETBY_FILEINFO = 2 }; /* p7_pipeline.pxd:30-33 */
enum { P7X_MMU = 0, P7X_MLAMBDA, P7X_VMU, P7X_VLAMBDA, P7X_FTAU, P7X_FLAMBDA };  /* libhmmer/__init__.pxd:30-37 */
enum { P7X_GA1 = 0, P7X_GA2, P7X_TC1, P7X_TC2, P7X_NC1, P7X_NC2 };               /* libhmmer/__init__.pxd:39-46 */
#define P7X_CUTOFF_UNSET (-99999.0f)
#define P7X_EVPARAM_UNSET (-99999.0f)
enum { P7X_IS_INCLUDED = 1, P7X_IS_REPORTED = 2, P7X_IS_NEW = 4, P7X_IS_DROPPED = 8, P7X_IS_DUPLICATE = 16 }; /* p7_tophits.pxd:13-18 */
enum { P7X_BITCUT_NONE = 0, P7X_BITCUT_GA = 1, P7X_BITCUT_NC = 2, P7X_BITCUT_TC = 3 }; /* p7_pipeline.pxd p7_pipemodes */

/* ------------------------------------------------------------------ host utilities */

int p7x_abi_version(void);

/* The longest model (nodes; a sequence query's length) the device kernels take: 64 lanes x the widest tier of nodes per
 * lane they are instantiated for.  A longer model is refused with P7X_EINVAL by every device entry point, and the message
 * states this number.  The reference has no limit (plan7.pyx:6156-6262).  nhmmer's SSV scan takes a model beyond
 * what one launch holds in chained parts (p7x_debug_ssv_plan). */
int p7x_max_model_length(void);

/* expf(-v) exactly as upstream read_asc30hmm parses an HMMER3/f ASCII save file
 * ('*' is passed as +inf and yields 0).  Replaces the C parser behind HMMFile (plan7.pyx:3656-4050). */
void p7x_expf_neg(const double *in, float *out, size_t n);

/* ------------------------------------------------------------------ profiles
 * p7x_hmm_view mirrors the P7_HMM fields the path needs (include/libhmmer/p7_hmm.pxd:48-78). */
typedef struct p7x_hmm_view {
  int32_t M;
  int32_t abc_type;            /* P7X_AMINO | P7X_DNA | P7X_RNA */
  const float *t;              /* [(M+1)*7] MM,MI,MD,IM,II,DM,DD probabilities */
  const float *mat;            /* [(M+1)*K] */
  const float *ins;            /* [(M+1)*K] */
  const float *compo;          /* [K] or NULL (model had no COMPO line) */
  float evparam[6];
  float cutoff[6];
  int32_t max_length;
  const char *name;            /* required */
  const char *acc;             /* or NULL */
  const char *desc;            /* or NULL */
  const char *consensus;       /* [M+2] as P7_HMM.consensus, or NULL */
  const char *rf, *mm, *cs;    /* optional annotation lines [M+2], or NULL */
} p7x_hmm_view;

typedef struct p7x_oprofile p7x_oprofile;   /* opaque: replaces P7_PROFILE + P7_OPROFILE */

/* p7_ProfileConfig (modelconfig.pxd:7-10; plan7.pyx:8082) followed by p7_oprofile_Convert
 * (impl_sse/p7_oprofile.pxd:121; plan7.pyx:4961), local multihit mode, length model L.
 * bg_f is P7_BG.f (p7_bg.pxd:10-30); K floats. */
int  p7x_oprofile_create(const p7x_hmm_view *hmm, const float *bg_f, int32_t L, p7x_oprofile **out);
/* p7_Builder_MaxLength(hmm, emit_thresh) (include/libhmmer/p7_builder.pxd; called by LongTargetsPipeline.search_hmm,
 * plan7.pyx:7346-7354 with window_beta): the smallest length W such that the core model, entered at its first match
 * state, emits a W-th residue with probability below <beta>.  Reproduces the MAXL lines hmmbuild wrote into the
 * nucleotide fixtures (beta = 1e-7: RF00001 305, bmyD 1736).  P7X_ERANGE if no such length below 200,000. */
int  p7x_hmm_max_length(const p7x_hmm_view *hmm, double beta, int32_t *out);
void p7x_oprofile_destroy(p7x_oprofile *om);

typedef struct p7x_oprofile_info {          /* scalars of P7_OPROFILE (impl_sse/p7_oprofile.pxd:52-108) */
  int32_t M, K, Kp, abc_type, L, max_length, mode;
  int32_t Q16, Q8, Q4;                       /* p7O_NQB/NQW/NQF (p7_oprofile.pxd:24-26) */
  uint8_t tbm_b, tec_b, tjb_b, base_b, bias_b;
  float   scale_b;
  int16_t xw[4][2];                          /* [E,N,J,C][MOVE,LOOP] */
  float   scale_w; int16_t base_w, ddbound_w; float ncj_roundoff;
  float   xf[4][2];
  float   evparam[6], cutoff[6], compo[20];
  float   nj;
} p7x_oprofile_info;
int p7x_oprofile_get_info(const p7x_oprofile *om, p7x_oprofile_info *info);

/* Striped (Farrar) views exactly as impl_sse stores them, for the OptimizedProfile properties
 * rbv/sbv/rwv/twv/rfv/tfv (plan7.pyx:4623-4813) and for checking against pressed .h3f/.h3p files.
 * which: 0 rbv u8 [Kp][Q16*16]; 1 sbv i8 [Kp][(Q16+17)*16]; 2 rwv i16 [Kp][Q8*8]; 3 twv i16 [8*Q8*8];
 *        4 rfv f32 [Kp][Q4*4]; 5 tfv f32 [8*Q4*4].  Returns bytes written, or -1. */
int64_t p7x_oprofile_striped(const p7x_oprofile *om, int which, void *out, size_t out_bytes);

/* Pressed profiles: one record of a `.h3f` (MSV part) and of a `.h3p` (everything else) file, the formats
 * `hmmpress` writes (reference hmmer/_hmmpress.py:29-66, OptimizedProfile.write plan7.pyx:5078-5105,
 * HMMPressedFile plan7.pyx:4051-4197).  write: pass NULL buffers to obtain the sizes; offs = byte offsets of this
 * model in the .h3m/.h3f/.h3p files (NULL: zeros).  read: parses one record from each buffer and returns the bytes
 * consumed; the log-odds tables come out exactly as stored. */
int p7x_oprofile_write_pressed(const p7x_oprofile *om, const int64_t offs[3], uint8_t *h3f, size_t cap_f, size_t *len_f,
                               uint8_t *h3p, size_t cap_p, size_t *len_p);
/* name (0), accession (1), description (2), consensus line with its leading pad (3): copies at most n-1 characters,
 * returns the full length, 0 when absent, -1 on bad arguments. */
int p7x_oprofile_get_string(const p7x_oprofile *om, int which, char *buf, size_t n);
int p7x_oprofile_read_pressed(const uint8_t *h3f, size_t nf, const uint8_t *h3p, size_t np, const float *bg_f,
                              p7x_oprofile **out, size_t *used_f, size_t *used_p, int64_t offs[3]);

/* FASTA text -> packed block (the input format of p7x_seqdb_create) in one pass; the reference reads sequence files
 * through Easel's C parser (easel.pyx SequenceFile.read_block, 8168-8192).  lut[256]: digital code per character,
 * 255 = illegal, 254 = ignored.  First call with dsq == NULL returns the sizes (nseq, nres, bytes of the string
 * table); second call fills dsq[nres + nseq + 1], offsets/lengths[nseq], strtab (NUL-terminated name then
 * description per record) and its two index arrays.  P7X_EFORMAT + *bad_pos on an illegal character. */
int p7x_fasta_parse(const char *text, size_t n, const uint8_t *lut, size_t *nseq, size_t *nres, size_t *strbytes,
                    uint8_t *dsq, int64_t *offsets, int32_t *lengths, char *strtab, int64_t *name_off, int64_t *desc_off,
                    size_t *bad_pos);

/* ------------------------------------------------------------------ devices */
int p7x_device_count(void);                       /* 0 when no HIP device is usable */
int p7x_device_name(int device, char *buf, size_t n);

/* ------------------------------------------------------------------ sequence database (device resident)
 * Replaces the `const ESL_SQ**` array of a DigitalSequenceBlock handed to _search_loop
 * (plan7.pyx:6393-6398; easel.pyx:8168-8192).  dsq holds the residues of target t at
 * dsq[offsets[t] .. offsets[t]+lengths[t]-1], digital codes 0..Kp-1.  Packed once, searched
 * by any number of profiles. */
typedef struct p7x_seqdb p7x_seqdb;
int  p7x_seqdb_create(int device, int32_t abc_type, const uint8_t *dsq, const int64_t *offsets,
                      const int32_t *lengths, size_t n, p7x_seqdb **out);
void p7x_seqdb_destroy(p7x_seqdb *db);
int64_t p7x_seqdb_ntargets(const p7x_seqdb *db);
int64_t p7x_seqdb_nresidues(const p7x_seqdb *db);

/* ------------------------------------------------------------------ single-stage entry points (unit-test seam)
 * Mirror OptimizedProfile.msv_filter / ssv_filter (plan7.pyx:4969-5070): one digital sequence,
 * score in nats; P7X_ERANGE + *sc=+inf on overflow.  dsq[0..L-1] are the residues (no sentinels). */
int p7x_msv_filter(const p7x_oprofile *om, int device, const uint8_t *dsq, int32_t L, float *sc);
int p7x_vit_filter(const p7x_oprofile *om, int device, const uint8_t *dsq, int32_t L, float *sc);
int p7x_fwd_parser(const p7x_oprofile *om, int device, const uint8_t *dsq, int32_t L, float *sc);
int p7x_bck_parser(const p7x_oprofile *om, int device, const uint8_t *dsq, int32_t L, float *sc);

/* Batched raw filter outputs over a whole database (parity tests and bench).
 * xJ[t]  : integer MSV end state (p7_MSVFilter's xJ), -1 on overflow.
 * xC[t]  : integer Viterbi end state (p7_ViterbiFilter's xC), 32767 on overflow.
 * fwd[t] : Forward score in nats (p7_ForwardParser). Any output pointer may be NULL.
 * The Viterbi filter is split as in the cascade: where the packed kernel takes the model, the database's longest
 * targets (its long prefix, option "vit_long_cut") go to the wave-per-target kernel. */
int p7x_filters_batch(const p7x_oprofile *om, const p7x_seqdb *db, int32_t *xJ, int32_t *xC,
                      float *fwd, float *bias_filtersc);

/* ------------------------------------------------------------------ the pipeline
 * p7x_pipeline_cfg mirrors the P7_PIPELINE fields reachable through the Python property
 * setters (p7_pipeline.pxd:58-107; plan7.pyx:5635-5950). */
typedef struct p7x_pipeline_cfg {
  int32_t by_E; double E, T; int32_t dom_by_E; double domE, domT; int32_t use_bit_cutoffs;
  int32_t inc_by_E; double incE, incT; int32_t incdom_by_E; double incdomE, incdomT;
  double  Z, domZ; int32_t Z_setby, domZ_setby;
  double  F1, F2, F3;
  int32_t do_max, do_biasfilter, do_null2;
  uint32_t seed;             /* do_reseeding = (seed != 0), plan7.pyx:5684-5688 */
  int32_t mode;              /* P7X_SEARCH_SEQS | P7X_SCAN_MODELS */
  int32_t host_threads;      /* workers for host-side domain definition; 0 = hardware_concurrency */
  int32_t host_envelopes;    /* 0 (default): single-domain envelopes are rescored by the device kernel; 1: on the host.  Long targets:
                              * 0 the device when the number of envelopes makes it pay (a few long envelopes are faster on the host
                              * workers), 1 always the host, 2 always the device */
  int32_t host_regions;      /* 0 (default): posterior decoding of the specials + region scan on the device; 1: on the host */
  /* long targets (nhmmer): p7_pipeline.pxd:80-87, 103-107; LongTargetsPipeline.__init__ plan7.pyx:6957-7060 */
  int32_t long_targets;      /* p7_Pipeline_LongTarget semantics: every domain is a hit, E-values from residues searched */
  int32_t strands;           /* P7X_STRAND_BOTH | _TOPONLY | _BOTTOMONLY */
  int32_t B1, B2, B3;        /* window lengths of the biased-composition modifier for the MSV / Viterbi / Forward filters */
  int32_t block_length;      /* residues per block read from a long target (W); consecutive blocks overlap by max_length */
  int32_t window_length;     /* > 0: overrides the model's max_length (nhmmer --w_length) */
  int32_t evalue_window_length; /* > 0: the window length p7_tophits_ComputeNhmmerEvalues is given when it differs from the scan's
                              * (an HMM query without window_length: p7_Builder_MaxLength(hmm, window_beta), plan7.pyx:7346-7354,
                              * while the scan keeps the max_length the optimized profile was built with); <= 0: the scan's */
  int32_t lt_part, lt_nparts; /* nhmmer over several devices: this call takes part lt_part of lt_nparts of the (target, block, strand)
                              * units of the search -- consecutive units, units counted in the order of the reference's loop
                              * (plan7.pyx:7582-7655) -- and returns an unfinished hit list; p7x_tophits_merge_longtargets finishes the
                              * parts together (E-values for all residues searched, duplicates, thresholds).  Default 0 of 1 */
  float   oa_guard;          /* near-tie guard of the device's optimal-accuracy traceback: with g > 0 a choice on the trace between
                              * candidates within |v| * g + g of each other (or a posterior that close to the next printed digit) sends
                              * the envelope to the host stage, which repeats it with Forward / Backward / null2 summed in UPSTREAM's
                              * order (impl_sse's four stripes: forward_full_upstream, p7x_domaindef.cpp), so that a decision the
                              * device's summation order cannot be trusted with is the reference's.  Default 4e-6 since ABI 8 (about
                              * 2 % of the envelopes; scripts/oa_guard_sweep2.py: no differing domain left at 3e-6 over 26,000); 0:
                              * off, and a kernel without the guard's arithmetic (the device is then compared with its own host twin,
                              * option "host_order" = 1, which sums in the device's order) */
  float   f3_guard;          /* relative half-width of the band around F3 inside which a target's Forward P-value is not trusted to the
                              * device's summation order: the device passes P <= F3 (1 + g), the host stage re-scores the targets with
                              * P > F3 (1 - g) with p7x_forward_parser_exact and applies F3 to that.  Default 4e-3 (a band of about 6e-3 bit, three times the stated tolerance of the device Forward score); 0: no guard */
  uint64_t lt_resident_key;  /* p7x_search_longtargets: nonzero = the caller's promise that a target buffer passed with this key always
                              * has the same contents (a token of the packed image, not of its address).  The device copy is then kept
                              * after the call and a later search with the same key and size does not upload the targets again (one
                              * copy per device; a new key replaces it).  0 (default): upload per call, nothing kept */
  int32_t host_ensembles;    /* 0 (default): the stochastic traceback ensembles of multi-domain regions (p7_domaindef.c
                              * region_trace_ensemble: 200 sampled tracebacks per region, p7_Null2_ByTrace of every sampled domain) run
                              * on the device and the clustered envelopes are rescored there in a second round; 1: on the host
                              * workers.  Identical results (one generator stream per region, the same choices: p7x_choice.hpp).
                              * Without re-seeding (seed 0) the regions of a search share one stream and the host samples them. */
  float   ens_guard;         /* ABI 8.  Near-threshold guard of the device's stochastic tracebacks: a choice of a sampled traceback
                              * whose deviate lies within g (as a fraction of the deviate's range) of one of its thresholds -- they
                              * come from a Forward matrix summed in the device's order -- flags the region, and the host stage
                              * samples flagged regions itself from a Forward matrix in upstream's order (status bit 6 of
                              * EnsembleResult).  Default 2.5e-7 = 2^-22: between the two orders no threshold of a reachable cell was seen
                              * further apart than 2^-21, and 5 in a million further than 2^-22 (scripts/order_spread.py, 3.6e8
                              * thresholds, profiles/r06_order_spread.txt); 0: off */
} p7x_pipeline_cfg;
enum { P7X_STRAND_BOTH = 0, P7X_STRAND_TOPONLY = 1, P7X_STRAND_BOTTOMONLY = 2 };
void p7x_pipeline_cfg_default(p7x_pipeline_cfg *cfg);   /* p7_pipeline_Create(NULL,...) defaults, plan7.pyx:5413-5421 */

typedef struct p7x_counters {   /* accounting, p7_pipeline.pxd:88-101 */
  uint64_t nmodels, nseqs, nres, nnodes;
  uint64_t n_past_msv, n_past_bias, n_past_vit, n_past_fwd;
  uint64_t n_output, pos_past_msv, pos_past_bias, pos_past_vit, pos_past_fwd, pos_output;
} p7x_counters;

typedef struct p7x_domain {     /* P7_DOMAIN, p7_domain.pxd:10-26 */
  int64_t ienv, jenv, iali, jali, iorf, jorf;
  float envsc, domcorrection, dombias, oasc, bitscore;
  double lnP;
  int32_t is_reported, is_included;
  /* alignment display, P7_ALIDISPLAY p7_alidisplay.pxd:26-53 (strings owned by the tophits handle) */
  int32_t N, hmmfrom, hmmto, M;
  int64_t sqfrom, sqto, L;
  const char *model, *mline, *aseq, *ppline, *rfline, *mmline, *csline;
  const char *hmmname, *hmmacc, *hmmdesc, *sqname, *sqacc, *sqdesc;
} p7x_domain;

typedef struct p7x_hit {        /* P7_HIT, p7_hit.pxd:27-58 */
  const char *name, *acc, *desc;
  int64_t seqidx;               /* index of the target in the searched block */
  int32_t window_length;
  double sortkey;
  float score, pre_score, sum_score;
  double lnP, pre_lnP, sum_lnP;
  float nexpected;
  int32_t nregions, nclustered, noverlaps, nenvelopes, ndom;
  uint32_t flags;
  int32_t nreported, nincluded, best_domain;
} p7x_hit;

typedef struct p7x_tophits p7x_tophits;   /* opaque: replaces P7_TOPHITS + the copied P7_PIPELINE (plan7.pyx:8813-8817) */

/* Pipeline._search_loop (plan7.pyx:6393-6453): p7_pli_NewModel once, then for every target
 * p7_pli_NewSeq / p7_bg_SetLength / p7_oprofile_ReconfigLength / p7_Pipeline / p7_pipeline_Reuse;
 * followed by p7_tophits_SortBySortkey + p7_tophits_Threshold (plan7.pyx:6255-6256).
 * targets' names/accessions/descriptions are NUL-separated string tables indexed by target
 * (may be NULL: hits then carry only seqidx). */
int p7x_search_block(const p7x_pipeline_cfg *cfg, const p7x_oprofile *om, const float *bg_f,
                     const p7x_seqdb *db, const char *const *names, const char *const *accs,
                     const char *const *descs, p7x_tophits **out);

/* The same search in two stages, for callers that overlap consecutive queries (the reference runs its queries on
 * worker threads, _hmmsearch.py:294-436): begin = filters + parsers on the device (blocks until they are done),
 * finish = domain definition + hit list; finish consumes the handle.  begin/finish of different searches may run
 * on different host threads at the same time. */
typedef struct p7x_pending p7x_pending;
int  p7x_search_block_begin(const p7x_pipeline_cfg *cfg, const p7x_oprofile *om, const float *bg_f,
                            const p7x_seqdb *db, p7x_pending **out);
int  p7x_search_block_finish(p7x_pending *pending, const char *const *names, const char *const *accs,
                             const char *const *descs, p7x_tophits **out);
void p7x_pending_destroy(p7x_pending *pending);
/* begin in two halves, for a caller that keeps several searches of one host thread in flight (hmmscan: one per model,
 * the OptimizedProfileBlock loop of plan7.pyx:6624-6677 turned inside out): enqueue queues stage 1 on its own device
 * stream and returns at once; wait blocks until that work is done (idempotent; finish calls it when the caller did
 * not).  Both halves of one search, and destroy of an un-waited handle, belong to the thread that called enqueue. */
int  p7x_search_block_enqueue(const p7x_pipeline_cfg *cfg, const p7x_oprofile *om, const float *bg_f,
                              const p7x_seqdb *db, p7x_pending **out);
int  p7x_search_block_wait(p7x_pending *pending);
/* A batch of query profiles against one resident target block: the many-query loops of the reference -- hmmsearch
 * over an iterable of HMMs (_hmmsearch.py:294-436, one Pipeline.search_hmm per query) and Pipeline._scan_loop over an
 * OptimizedProfileBlock (plan7.pyx:5072-5338, 6624-6677) -- as ONE set of device launches: every kernel of the cascade
 * takes the profile of its work item from the batch (blockIdx.y), so a launch serves all nq profiles.  Results are
 * those of nq separate searches (tests/test_gpu_search.py).  oms[q] may have any lengths; out of finish is a caller
 * array of nq hit lists, in the order of oms.  wait is p7x_search_block_wait; the threading rules are the same. */
int  p7x_search_batch_enqueue(const p7x_pipeline_cfg *cfg, const p7x_oprofile *const *oms, size_t nq, const float *bg_f,
                              const p7x_seqdb *db, p7x_pending **out);
int  p7x_search_batch_finish(p7x_pending *pending, const char *const *names, const char *const *accs,
                             const char *const *descs, p7x_tophits **outs);
size_t p7x_pending_nqueries(const p7x_pending *pending);
/* Test seam of the bias filter's logarithm: out[i] = the device's (float) log((double) in[i]) as bias_kernel takes it at every
 * residue (a table + series evaluation in double; claimed to round to the same float as the C library's logarithm, which
 * is what the reference's esl_hmm_Forward calls: tests/test_gpu_filters.py checks every float of [2^-7, 2^7)). */
int  p7x_debug_log_of_float(int device, const float *in, float *out, size_t n);
/* Test seam of the memory pools (csrc/p7x_devmem.hpp), in bytes: out[0] = device memory obtained from the runtime through the
 * slab pool of <device> and not yet freed, [1] = of that, parked in the pool; [2] = pinned host memory obtained (process-wide),
 * [3] = of that, parked.  A workload that runs a second time on pooled objects must leave all four as they were. */
int  p7x_debug_memory_stats(int device, int64_t out[4]);
/* Test seam of the cascades' stream layout (csrc/p7x_device.hpp: DeviceCtx), no HIP call: the order in which a device context
 * creates the streams of its cascade sets.  out[0] = sets, [1] = streams per set (the main stream and its side streams),
 * [2] = which side stream (0-based) is the partner of the main stream, [3] = spacer streams; then, set by set, the creation
 * position (0-based, in the context's order of creation) of the set's main stream and of its side streams in their order;
 * then the positions of the spacers.  Returns the number of values (all of them are written if cap is at least that).
 * *hw_queues = GPU_MAX_HW_QUEUES as the environment had it when the library was loaded; 0: it was unset and the library
 * asked for eight (which holds only if the HIP runtime was not initialised yet); -1: set to something that is no number. */
int64_t p7x_debug_stream_plan(int32_t *out, size_t cap, int32_t *hw_queues);
/* Test seams of the stochastic traceback ensembles (p7_domaindef.c region_trace_ensemble; p7_domaindef.pxd:23-59).
 * p7x_debug_choice: one choice point of p7_StochasticTrace with n paths of weights p[], for the generator state x after the
 *   draw: the path taken through the integer thresholds the product uses and through esl_rnd_FChoose as the reference
 *   writes it (they must agree for every p and x).
 * p7x_debug_ensemble: the 200 sampled tracebacks of region i..j (1-based) of one target of a resident block, on the device
 *   (use_device != 0) or by the host twin: dom[ndom][5] = sample, first / last residue inside the region, first / last
 *   node, a sample's domains first to last; n2[pos], pos = 1..j-i+1: the summed null2 odds ratios of the residue;
 *   status 0 = sampled. */
int  p7x_debug_choice(const float *p, int n, uint32_t x, int *via_thresholds, int *via_fchoose);
/* Calibration seam of the ensemble walk's near-threshold guard: the Forward matrix of region i..j of dsq1[1..L] in the device's
 * summation order and in upstream's, and for every cell the integer thresholds of its choice points in both: out12[0] =
 * thresholds compared, [1] = largest difference / 2^32, [2 + b] = how many differ by more than 2^-(24 - b), b = 0..9. */
int  p7x_debug_order_spread(const p7x_oprofile *om, const uint8_t *dsq1, int32_t L, int32_t i, int32_t j, int multihit, double *out12);
/* Test seam of the host parsers in upstream's summation order (the rows-only Forward / Backward engines of the host stage,
 * whose rows the region-scan guard scans again): the special-state rows of dsq1[1..L], multihit with the length model of L,
 * fx / bx = (L+1) x [E,N,J,B,C,SCALE] floats each. */
int  p7x_debug_parser_rows(const p7x_oprofile *om, const uint8_t *dsq1, int32_t L, float *fx, float *bx);
/* Test seam of the bias filter's host twin (bias_filter_score: what the F3 guard and the long-target windows score with, the
 * same float32 operations as bias_kernel): p7_bg_FilterScore of dsq1[1..L] in nats.  L = 0: the null1 score of an empty
 * target, no residue read. */
int  p7x_debug_bias_filter_host(const p7x_oprofile *om, const uint8_t *dsq1, int32_t L, float *sc);
/* Test seam of the long-target SSV scan's tables (host code, no device): the registers per lane R the kernel takes for this
 * model, the most a cell can lose in one row with a canonical residue (byte units), and the table it stages in LDS --
 * [parity][x < 4][q][lane][c] packed pairs (lo, hi) of bias - rb[x][k], register j = 4q + c of the lane holding nodes
 * (2g - 1, 2g) on odd rows (parity 0) and (2g, 2g + 1) on even rows, g = lane * R + j; <pair> != 0: with the virtual node
 * M + 1 (emission 0) of the every-second-row flavour.  Returns the number of 32-bit words of the table (written when
 * cap_words is large enough), or a negative status. */
int64_t p7x_debug_ssv_tables(const p7x_oprofile *om, int pair, int32_t *R, int32_t *pair_slack, uint32_t *tab4q, size_t cap_words);
/* Test seams of the SSV scan in chained parts (host code, no device).  One launch of the kernel holds the model in
 * registers; a model beyond that is cut into P consecutive parts that run one after the other, each taking the score of
 * the node before its first one from the part before, row by row.
 * p7x_debug_ssv_plan: the parts of a model of M nodes -- nodes lo[q] .. hi[q], R[q] registers per lane, q < min(P, cap) --
 * with parts_forced = 0 the library's plan, 2 .. 4 that many parts where the model has two nodes for each (what the option
 * "ssv_parts" does to a scan).  Returns P, or a negative status (M beyond p7x_max_model_length()).
 * p7x_debug_ssv_part_tables: p7x_debug_ssv_tables for part <part> of that plan: cell c of the layout is node lo - 1 + c,
 * padding outside lo .. hi (cell 0 included), the virtual node hi + 1 in the last part only.
 * p7x_debug_ssv_merge_rows: the host's merge of the rows the parts report, n records (position, strand, node, byte score)
 * in any order -> one record per (strand, position), in that order: the highest score, on a tie the node that comes
 * first in upstream's striped order, ((k - 1) % Q16) * 16 + (k - 1) / Q16.  Returns the number of rows written (<= n). */
int     p7x_debug_ssv_plan(int M, int pair, int parts_forced, int32_t *lo, int32_t *hi, int32_t *R, int cap);
int64_t p7x_debug_ssv_part_tables(const p7x_oprofile *om, int pair, int parts_forced, int part, int32_t *lo, int32_t *hi, int32_t *R,
                                  uint32_t *tab4q, size_t cap_words);
int64_t p7x_debug_ssv_merge_rows(int Q16, size_t n, const int64_t *pos, const int32_t *strand, const int32_t *k, const int32_t *sc,
                                 int64_t *out_pos, int32_t *out_strand, int32_t *out_k, int32_t *out_sc);
/* Test / diagnostic seam: process-wide knobs, by name; value -1 = not set (the library decides).  The library itself reads no
 * environment variables.  Kernel families for parity tests: "small_block" (0: never the wave-per-target filters for small
 * blocks), "vit_wave" (1: the wave-per-target Viterbi kernel for every model), "msv_exact" (1: no fast MSV pass),
 * "msv_long_groups" (0: the longest groups stay with the lane kernel), "msv_blocks_per_cu" (cap), "device_clustered" (0 / 1:
 * with host ensembles, where their clustered envelopes are rescored), "env_workspace_gb" (cap of the envelope kernel's
 * workspace), "ssv_kernel" (long-target SSV scan: 3 = the row maximum in every row, 4 = in every second row whatever the
 * model), "ssv_parts" (2 / 3 / 4: the scan in that many chained parts, for any model with two nodes for each; 0: the
 * library's plan), "ssv_scan_chunk" (n: the chunk length of the batched scan, a multiple of 64 >= 64 whatever the model).
 * Traces on stderr: "trace_finish", "trace_longtarget", "trace_envelope", "host_profile" (1: on). */
int  p7x_debug_set_option(const char *name, int value);
/* Test seam of the envelope kernel's schedule (csrc/p7x_envscore.hip: DeviceEnvelopeScorer::begin, all three modes), no HIP
 * call: process-wide totals since the last reset, read before <reset> != 0 clears them.  out[0] = begin calls that had
 * envelopes, [1] = jobs with envelopes, [2] = envelopes, [3] = kernel launches, [4] = wavefronts launched (the sum over jobs
 * of nblocks * env_waves(C)), [5] = the sum over jobs of max(0, nenv - nblocks * env_waves(C)): at least this many envelopes
 * came second or later in their wavefront, on a workspace slab another envelope had used, [6] = jobs whose queue order is
 * not the identity, [7] = the most jobs in any one launch.  The option "env_blocks" = n (p7x_debug_set_option) gives a job at
 * most n blocks, so that a small input runs the queue a library search runs. */
int  p7x_debug_env_plan(int64_t out[8], int reset);
int  p7x_debug_ensemble(const p7x_oprofile *om, const p7x_seqdb *db, int64_t target, int32_t i, int32_t j, uint32_t seed,
                        int use_device, int32_t *ndom, int32_t *dom, int32_t dom_cap, float *n2, int32_t *status);
/* Test seams of the float64 reference of the ensembles (tests/ensemble_reference.py); additions, the ABI number stays.
 * p7x_debug_ensemble_traces: host code, no device.  The 200 paths the host twin samples from region i..j of dsq1[1..L] in
 *   the "host_order" option's summation order: step s of sample t is st / k / pos[off201[t] + s] (p7T_* state code, node,
 *   residue inside the region; S first, T last), *nsteps steps in all (at most step_cap are written); dom / ndom / n2 as
 *   p7x_debug_ensemble returns them for the host twin.
 * p7x_debug_ensemble_records: the choice records of every cell and row of the region (p7x_choice.hpp: 8 words per cell,
 *   cells[(j-i+2)][M+1][8], and 8 per row, rows[j-i+2][8]) as the Forward fill kernel wrote them (use_device != 0: the region
 *   of target <target> of <db>; what the kernel leaves untouched -- row 0 of the cells, node 0 -- is zero) or as the host
 *   twin forms them for every cell (use_device == 0; with db == NULL the region is of dsq1[1..L], else dsq1 / L are ignored).
 *   md (may be NULL): md[(j-i+2)][M+1][2], the scaled Forward values M(r, k) and D(r, k) kept beside the records: the E
 *   state chooses among them, each times the row's factor (float) (1 / xE) in word 4 of its row record.
 * p7x_debug_ens_walk_plan: host code, no device.  What the walk kernel keeps in LDS for a region of Lr residues of a model
 *   of M nodes, in a launch whose longest model has maxM >= M nodes and whose longest region maxLr >= Lr residues (the
 *   launch's LDS is sized for those), under an LDS cap of lds_kb KiB; lds_kb <= 0: what the library would choose now, the
 *   option "ens_lds_kb" honoured.  out[38]: lds_bytes, least, want; rows, residues in LDS (0 / 1); the accumulators' home
 *   (0 registers, 1 LDS, 2 memory); odds, Forward rows in LDS; index bits of the match cache and of the insert / delete
 *   cache; match cache by row; cell numbers fit the tags; bytes used before and after the caches; then (offset, bytes) of
 *   the twelve sections in LDS order -- visit counts, null2 vector, its partial sums, Forward-row tags, row records, 1 / xE,
 *   residues, accumulators, odds, Forward rows, match cache, insert / delete cache -- offset -1 for a piece kept in memory.
 *   Returns the number of words written, or a negative status. */
int  p7x_debug_ens_walk_plan(int M, int Lr, int maxM, int maxLr, int lds_kb, int32_t *out);
int  p7x_debug_ensemble_traces(const p7x_oprofile *om, const uint8_t *dsq1, int32_t L, int32_t i, int32_t j, uint32_t seed,
                               int8_t *st, int32_t *k, int32_t *pos, int64_t step_cap, int32_t *off201, int64_t *nsteps,
                               int32_t *ndom, int32_t *dom, int32_t dom_cap, float *n2);
int  p7x_debug_ensemble_records(const p7x_oprofile *om, const p7x_seqdb *db, int64_t target, const uint8_t *dsq1, int32_t L,
                                int32_t i, int32_t j, int use_device, uint32_t *cells, uint32_t *rows, float *md);
/* Parity seam of the batched cascade (the multi-profile twin of p7x_filters_batch): runs stage 1 exactly as
 * p7x_search_batch_enqueue queues it -- profiles grouped into kernel classes, the hybrid lane / wave MSV split, the work
 * lists -- and returns what the stages left behind, [nq][ntargets] in caller order of both: xJ (every target; -1
 * overflow), xC of the targets that reached the Viterbi filter (INT32_MIN elsewhere; 32767 overflow) and the last
 * stage each target passed (0 none, 1 MSV, 2 bias, 3 Viterbi, 4 Forward).  Any output may be NULL. */
int  p7x_search_batch_raw(const p7x_pipeline_cfg *cfg, const p7x_oprofile *const *oms, size_t nq, const float *bg_f,
                          const p7x_seqdb *db, int32_t *xJ, int32_t *xC, uint8_t *stage);

/* nhmmer: LongTargetsPipeline.search_hmm / _search_loop_longtargets (plan7.pyx:7272-7418, 7541-7664) for a block of
 * long DNA / RNA targets.  Per target and strand: the SSV scan of p7_Pipeline_LongTarget (p7_pipeline.pxd:131-143) runs
 * on the device over the whole strand (reverse complement formed on the fly); the windows it seeds go through
 * p7_Pipeline_LongTarget's tail on the host (window MSV + bias, long-target Viterbi, Forward / Backward, domain
 * definition with long_target = TRUE, one hit per domain), followed by p7_tophits_ComputeNhmmerEvalues, target lengths,
 * p7_tophits_RemoveDuplicates, sort and threshold (plan7.pyx:7390-7412).  Targets: residues dsq[offsets[t] ..
 * offsets[t] + lengths[t] - 1] (64-bit lengths: chromosomes); cfg.long_targets must be set.
 * Records that lie end to end in dsq with one sentinel (a code outside the alphabet) between them -- the layout of
 * p7x_seqdb_create -- are scanned where they are, all of them with one launch (the sentinel ends every diagonal); any
 * other layout is packed that way first.  The window stages run one device batch per stage for the whole target set. */
int p7x_search_longtargets(const p7x_pipeline_cfg *cfg, const p7x_oprofile *om, int device,
                           const uint8_t *dsq, const int64_t *offsets, const int64_t *lengths, size_t n,
                           const char *const *names, const char *const *accs, const char *const *descs, p7x_tophits **out);
/* The device copy that cfg.lt_resident_key keeps between searches is dropped: on <device> (-1: every device), if it carries
 * <key> (0: whatever it carries).  The reference has no counterpart (its targets live in host memory); here the owner of a
 * target image calls this when the image goes (pyhmmer_amd does, from a finalizer of the packed block), so that a genome
 * does not stay pinned in HBM for the life of the process.  A search still scanning the copy keeps it until it is done. */
int p7x_longtargets_release_resident(int device, uint64_t key);
/* SSV window seeds of one strand of one target block as p7_SSVFilter_longtarget emits them (position of the diagonal's
 * first residue, model node of its last cell, diagonal length), for tests against the oracle: the device scan followed
 * by upstream's sequential bookkeeping.  seeds: caller array of cap x 3 int64; returns the number found (may exceed cap)
 * or a negative status. */
int64_t p7x_ssv_longtarget_seeds(const p7x_pipeline_cfg *cfg, const p7x_oprofile *om, int device, const uint8_t *dsq, int64_t L,
                                 int complement, int64_t *seeds, size_t cap);
/* CPU test seam: the host tail of the long-target pipeline for seeds found elsewhere (the oracle's scan); no device. */
int p7x_longtarget_from_seeds(const p7x_pipeline_cfg *cfg, const p7x_oprofile *om,
                              const uint8_t *dsq, const int64_t *offsets, const int64_t *lengths, size_t n,
                              const char *const *names, const char *const *accs, const char *const *descs,
                              const int64_t *seed_target, const int64_t *seed_block, const int32_t *seed_strand,
                              const int64_t *seeds, size_t nseeds, p7x_tophits **out);

/* nhmmscan: ONE long nucleotide sequence against a library of models (the scan orientation of p7x_search_longtargets; an
 * extension: pyhmmer's LongTargetsPipeline.scan_seq raises).  Additions of ABI 8: the number and p7x_pipeline_cfg stay.
 *
 * p7x_lt_library: the SSV tables of a batch of optimized profiles on one device, built and uploaded once and scanned by any
 * number of query sequences.  The profiles must outlive it.  Which launch a model goes into (p7x_debug_ssv_batch_plan) is
 * fixed when the library is created, from the options "ssv_kernel" / "ssv_parts" as they are then.
 *
 * p7x_scan_longtargets: sequence dsq[1..L] (dsq[0] and dsq[L+1] hold a code outside the alphabet) against oms[0..nmodels-1].
 * The SSV scan of all models runs as one launch per (register tile, row flavour) group over one upload of the sequence
 * (resident_key != 0: the upload is kept as cfg.lt_resident_key keeps it); a model that the scan takes in chained parts
 * (M > 6,141, or "ssv_parts") goes through the single-model scan.  Then, per model and side by side on the cfg.host_threads
 * workers, exactly what p7x_search_longtargets does with that model's rows: seeds per (block, strand), windows, domains.
 * out[m] is what a lone p7x_search_longtargets of model m against the sequence returns -- E-values for this sequence's
 * residues, duplicates removed, thresholds applied --; a model without seeds gets its empty list without touching the
 * device again.  evalue_window_lengths (may be NULL): per model, what cfg.evalue_window_length is for a lone search of it
 * (<= 0: the scan's).  lib (may be NULL: tables built for this call) must have been created from the same oms. */
typedef struct p7x_lt_library p7x_lt_library;
int  p7x_lt_library_create(const p7x_oprofile *const *oms, size_t nmodels, int device, p7x_lt_library **out);
void p7x_lt_library_destroy(p7x_lt_library *lib);
int  p7x_scan_longtargets(const p7x_pipeline_cfg *cfg, const p7x_oprofile *const *oms, size_t nmodels, int device,
                          const uint8_t *dsq, int64_t L, const char *name, const char *acc, const char *desc,
                          const int32_t *evalue_window_lengths, p7x_lt_library *lib, uint64_t resident_key, p7x_tophits **out);
/* The per-model lists of one query sequence (p7x_scan_longtargets, or any finished or unfinished long-target lists of
 * single-model searches against that one sequence) -> one scan-mode hit list.  Host code, no device.  Every model's hits are
 * finished as its lone search finishes them (an unfinished list: p7_tophits_ComputeNhmmerEvalues with its own residue count
 * and window length, duplicates removed WITHIN the model), renamed to the model's name / accession / description, numbered
 * model_index[m] (NULL: in the order they come, continuing a list begun earlier), and appended to *inout (NULL: a new list
 * for the sequence name / acc / desc / length).  Hits of different models that overlap on the sequence are all kept.
 * nmodels_total > 0 finishes the list: the lnP of every hit and domain gets + log(nmodels_total) -- upstream's nhmmscan
 * scales the E-value by the number of models the same way --, the hits are sorted by key, and reporting and inclusion are
 * thresholded on the scaled values.  nmodels_total == 0: more batches follow (a library of unknown size: finish with a last
 * call, nmodels = 0 allowed); nmodels_total < 0: finish, the models collected so far are the whole library (none: an empty
 * list).  The per-model lists are left to the caller.  The result does not depend on how the models
 * were dealt into calls, nor on their order when model_index is given. */
int  p7x_scan_collect_longtargets(p7x_tophits *const *per_model, const int64_t *model_index, size_t nmodels, int64_t nmodels_total,
                                  const p7x_pipeline_cfg *cfg, const char *name, const char *acc, const char *desc, int64_t length,
                                  p7x_tophits **inout);
/* Test seam: the seeds of one strand of dsq[0..L-1] for every model of a batch through the batched scan, as
 * p7x_ssv_longtarget_seeds gives them for one: model after model in <seeds> (cap x 3 int64), count[m] of them for model m.
 * Returns the total (may exceed cap) or a negative status. */
int64_t p7x_ssv_longtarget_seeds_batch(const p7x_pipeline_cfg *cfg, const p7x_oprofile *const *oms, size_t nmodels, int device,
                                       const uint8_t *dsq, int64_t L, int complement, int64_t *seeds, size_t cap, int64_t *count);
/* Host only: the launches of the batched scan for models of M[i] nodes that lose at most pair_slack[i] units per row, under
 * the options as they are.  launch_of[i] = the model's launch, -1: it goes through the single-model scan (chained parts).
 * Per launch (at most cap are written): R, PAIR (0 / 1) and the dynamic LDS in bytes.  lds_limit (may be NULL): the most a
 * launch may ask for.  Returns the number of launches or a negative status. */
int  p7x_debug_ssv_batch_plan(const int32_t *M, const int32_t *pair_slack, int n, int32_t *launch_of, int32_t *launch_R,
                              int32_t *launch_pair, int64_t *launch_lds, int cap, int64_t *lds_limit);
/* Process-wide totals of the batched scan since the last reset (read before <reset> != 0 clears them): out[0] = libraries
 * whose tables were built and uploaded, [1] = scans, [2] = batched launches, [3] = models scanned in batched launches,
 * [4] = models that went through the single-model scan, [5] = scans repeated with a larger record buffer, [6] = the last
 * scan's kernel time in microseconds (HIP events), [7] = its cells (rows x nodes, warm-up not counted). */
int  p7x_debug_ssv_batch_stats(int64_t out[8], int reset);

/* The Forward parser score (nats) of residues dsq[1..L] in the summation order of the reference's striped vectors
 * (impl_sse/fwdback.c forward_engine, do_full = FALSE; multihit, length model of L): what the host stage uses to decide
 * targets whose Forward P-value falls within the guard band around F3 (cfg.f3_guard).  Host code; no device. */
int p7x_forward_parser_exact(const p7x_oprofile *om, const uint8_t *dsq, int32_t L, float *sc);

/* hmmscan orientation (Pipeline.scan_seq / _scan_loop, plan7.pyx:6534-6677; hmmer/_hmmscan.py): search every model
 * against the block of query sequences with cfg.mode = P7X_SCAN_MODELS (one device pass per model, nothing pruned), then
 * transpose: out[s] (caller-provided array of nseqs pointers) receives the hit list of query sequence s, its hits
 * named after the models, reportability tested with the running Z = models seen so far, E-values with Z = nmodels,
 * counters per sequence (nmodels, nnodes, n_past_* = models whose filters the sequence passed). */
int p7x_scan_collect(p7x_tophits *const *per_model, size_t nmodels, const p7x_pipeline_cfg *cfg, size_t nseqs,
                     const char *const *seq_names, const char *const *seq_accs, const char *const *seq_descs,
                     const int32_t *seq_lengths, p7x_tophits **out);
/* The same, incrementally: the per-model results are folded in as the device batches of a scan come back (in model order;
 * the running Z of p7_pli_NewModel is the model's number) and can be destroyed right after, so a scan over a library of
 * any size holds one batch of per-model results at a time, as the reference's loop over the pressed file holds one
 * profile (plan7.pyx:6680-6737).  p7x_scan_accum_finish consumes the accumulator. */
typedef struct p7x_scan_accum p7x_scan_accum;
int  p7x_scan_accum_create(const p7x_pipeline_cfg *cfg, size_t nseqs, const char *const *seq_names, const char *const *seq_accs,
                           const char *const *seq_descs, const int32_t *seq_lengths, p7x_scan_accum **out);
int  p7x_scan_accum_add(p7x_scan_accum *acc, p7x_tophits *const *per_model, size_t nmodels);
/* the same for results that come back in any order (batches of a length-sorted profile database): model_index[i] is the
 * number of per_model[i]'s profile in the database (0-based, each exactly once over the scan); callable from several threads.
 * The running Z of a model is its number + 1 either way, and p7x_scan_accum_finish restores the database's order. */
int  p7x_scan_accum_add_indexed(p7x_scan_accum *acc, p7x_tophits *const *per_model, const int64_t *model_index, size_t nmodels);
/* Test seam: the last filter every target passed (0 none, 1 MSV, 2 bias, 3 Viterbi, 4 Forward), as the device path records it
 * in a scan's per-model results and p7x_scan_accum_* turn into per-sequence accounting; lets the CPU tests attach the
 * oracle's stages to results of p7x_postprocess_targets. */
int  p7x_debug_tophits_set_stages(p7x_tophits *th, const uint8_t *stage, size_t n);
int  p7x_scan_accum_finish(p7x_scan_accum *acc, p7x_tophits **out);
void p7x_scan_accum_destroy(p7x_scan_accum *acc);

/* Host half of p7_Pipeline for targets that already passed the Forward filter: Backward-derived domain
 * definition (p7_domaindef_ByPosteriorHeuristics, p7_domaindef.pxd:69-72), per-sequence / per-domain scores,
 * reporting thresholds, sort.  p7x_search_block calls this internally with the device parsers' output; it is
 * exported so the host logic can be tested without a GPU from any Forward/Backward parser rows.
 * surv[i] = target index; fwdsc[i] nats; fwd_xmx / bck_xmx + xmx_off[i] = (L+1) x [E,N,J,B,C,SCALE] rows
 * (impl_sse/p7_omx.pxd:16-38).  offsets[t] >= 1.  stage_counts = n_past_{msv,bias,vit,fwd} or NULL. */
int p7x_postprocess_targets(const p7x_pipeline_cfg *cfg, const p7x_oprofile *om, const uint8_t *dsq,
                            const int64_t *offsets, const int32_t *lengths, size_t n, const int32_t *surv,
                            size_t nsurv, const float *fwdsc, const float *fwd_xmx, const float *bck_xmx,
                            const int64_t *xmx_off, const uint64_t *stage_counts, const char *const *names,
                            const char *const *accs, const char *const *descs, p7x_tophits **out);

void     p7x_tophits_destroy(p7x_tophits *th);
/* n results at once (a scan batch is thousands of per-model lists that only pass through the caller); the slots are zeroed */
void     p7x_tophits_destroy_many(p7x_tophits **th, size_t n);
p7x_tophits *p7x_tophits_clone(const p7x_tophits *th);   /* TopHits.copy, plan7.pyx:9150-9170 */
int64_t  p7x_tophits_nhits(const p7x_tophits *th);
int      p7x_tophits_abc_type(const p7x_tophits *th);     /* alphabet of the query (P7X_AMINO / _DNA / _RNA); 0: not known (the lists of a scan) */
int      p7x_tophits_get_counters(const p7x_tophits *th, p7x_counters *c);
int      p7x_tophits_get_cfg(const p7x_tophits *th, p7x_pipeline_cfg *cfg);   /* Z/domZ as finally set */
int      p7x_tophits_get_hit(const p7x_tophits *th, int64_t i, p7x_hit *hit);
int      p7x_tophits_get_domain(const p7x_tophits *th, int64_t i, int32_t d, p7x_domain *dom);
/* p7_tophits_Merge + p7_pipeline_Merge + re-threshold (plan7.pyx:9172-9276): merges src into dst. */
int      p7x_tophits_merge(p7x_tophits *dst, const p7x_tophits *src);
/* The parts of one long-target search (cfg.lt_nparts > 1, one p7x_search_longtargets call per part, typically one per
 * device) -> the hit list of the whole search: p7_tophits_ComputeNhmmerEvalues with the residues of all parts,
 * p7_tophits_RemoveDuplicates across them, sort, threshold (plan7.pyx:7390-7412).  The parts are consumed. */
int      p7x_tophits_merge_longtargets(p7x_tophits **parts, size_t nparts, p7x_tophits **out);
/* Many queries x many shards in one call, threaded over the queries: blobs[q * nparts + r] / sizes[...] = the
 * p7x_tophits_serialize image of query q on shard r (NULL / 0: that shard had nothing to say, e.g. an empty shard that
 * was never searched).  outs[q] = what TopHits.merge gives for the same lists in shard order.  threads <= 0: every usable CPU. */
int      p7x_tophits_merge_many(const void *const *blobs, const size_t *sizes, size_t nq, size_t nparts, int threads, p7x_tophits **outs);
/* Flat byte image of a hit list (the reference pickles TopHits through p7_hit_Serialize, plan7.pyx:8394-8572);
 * used to move per-device / per-process results to the merging host.  serialize returns the size needed. */
int64_t  p7x_tophits_serialize(const p7x_tophits *th, void *buf, size_t cap);
p7x_tophits *p7x_tophits_deserialize(const void *buf, size_t n);
int      p7x_tophits_sort_by_key(p7x_tophits *th);       /* p7_tophits_SortBySortkey, plan7.pyx:8820-8824 */
int      p7x_tophits_threshold(p7x_tophits *th);         /* p7_tophits_Threshold, plan7.pyx:8804-8818 */
int      p7x_tophits_sort_by_seqidx(p7x_tophits *th);    /* p7_tophits_SortBySeqidxAndAlipos, TopHits.sort(by="seqidx") plan7.pyx:9120-9148 */
int      p7x_tophits_is_sorted(const p7x_tophits *th, int by_seqidx);   /* TopHits.is_sorted, plan7.pyx:9078-9118; 1 / 0 */
/* Hit.reported / included / dropped / duplicate setters (plan7.pyx:2125-2235): replace the P7X_IS_* flag word of hit i. */
int      p7x_tophits_set_hit_flags(p7x_tophits *th, int64_t i, uint32_t flags);
/* p7_tophits_CompareRanking (TopHits.compare_ranking, plan7.pyx:8897-8930; what a jackhmmer round does with the hits of the
 * round before): ranked[nranked] are the names of the hits the previous round included.  Walks the list in its current
 * order: an included hit whose name is not among them gets P7X_IS_NEW and is counted, a hit that is not included and
 * whose name is among them gets P7X_IS_DROPPED; no flag is cleared.  included[0 .. min(*nincluded, cap)) receive the
 * positions of the included hits in list order (the next ranking), *nincluded their number.  Returns the number of new
 * hits, -1 on bad arguments. */
int64_t  p7x_tophits_compare_ranking(p7x_tophits *th, const char *const *ranked, size_t nranked, int64_t *included, size_t cap,
                                     int64_t *nincluded);
/* Hit.name / accession / description setters (plan7.pyx:1960-2050): which = 1 name (not NULL), 2 accession, 4 description
 * (NULL clears); pointers handed out earlier by p7x_tophits_get_hit for this hit are invalidated. */
int      p7x_tophits_set_hit_text(p7x_tophits *th, int64_t i, int which, const char *value);
/* Timing slots of the search that produced a hit list, milliseconds unless noted; the lower-cased names are the keys of
 * TopHits.timings_ms, in this order.  A query carries the timings of the batch it travelled in. */
enum p7x_timing {
  P7X_MS_MSV = 0,            /* HIP events: MSV kernels and the P-value pass.  Long targets: SSV scan and seeds, wall */
  P7X_MS_BIAS,               /* HIP events: bias filter and the Viterbi work list.  Long targets: the windows' MSV / bias / Viterbi
                              * batches on the device, wall */
  P7X_MS_VITERBI,            /* HIP events: Viterbi filter and its P-value pass */
  P7X_MS_FORWARD,            /* HIP events: Forward parser (scores only) and its P-value pass */
  P7X_MS_FWD_ROWS,           /* HIP events: Forward with rows for the survivors (a stage-by-stage batch: their row layout only) */
  P7X_MS_HOST_DOMAINDEF,     /* the host stage (domain definition), wall, P7X_MS_ENVELOPES included.  Long targets: everything
                              * after the seeds, wall, P7X_MS_BIAS included */
  P7X_MS_TOTAL,              /* P7X_MS_STAGE1 + P7X_MS_STAGE2 */
  P7X_MS_MSV_KERNEL,         /* HIP events: the MSV kernels alone; a batch of several kernel classes: its largest fast-MSV launch.
                              * Long targets: the SSV scan kernels */
  P7X_MS_ENVELOPES,          /* device rescoring of domain envelopes: wall from the first launch to the last result, transfers included */
  P7X_MS_HOST_MULTI,         /* the host's own share of the multi-domain regions (overlaps P7X_MS_ENVELOPES) */
  P7X_MS_STAGE1,             /* wall of stage 1 (p7x_search_batch_enqueue until _wait returns) */
  P7X_MS_STAGE2,             /* wall of stage 2 (p7x_search_batch_finish) */
  P7X_MS_HOST_STAGE_BUSY,    /* max(0, P7X_MS_HOST_DOMAINDEF - P7X_MS_ENSEMBLE_WAIT - P7X_MS_ENVELOPE_WAIT) */
  P7X_MS_ENSEMBLE_WAIT,      /* of the host stage: waiting for the ensemble kernels */
  P7X_MS_ENVELOPE_WAIT,      /* of the host stage: waiting for the two envelope rounds */
  P7X_MS_BATCH_QUERIES,      /* a count: queries of the batch */
  P7X_MS_MSV_LAUNCH_LANES,   /* a count: lanes (queries) that the launch timed in P7X_MS_MSV_KERNEL covered */
  P7X_MS_MSV_LAUNCH_NODES,   /* a count: model nodes of those lanes */
  P7X_MS_COUNT
};
/* ms[0 .. min(n, P7X_MS_COUNT)) = the slots above */
int      p7x_tophits_get_timings(const p7x_tophits *th, double *ms, int n);
/* how often the two guards acted in the search that produced <th>: targets the F3 guard took back out of the device's
 * survivor list, device envelopes the optimal-accuracy near-tie guard repeated on the host (0 after a merge /
 * deserialisation), and the latter by the kind of choice that was close: the predecessor of a match / insert / delete
 * cell, C<-E, J<-E, the end cell, B<-N/J, a printed posterior digit (an envelope can count under several) */
int      p7x_tophits_get_guard_counts(const p7x_tophits *th, int64_t *f3_dropped, int64_t *oa_redone, int64_t oa_why[8]);
/* ABI 8: multi-domain regions whose traceback ensemble the device sampled, regions its near-threshold guard
 * (p7x_pipeline_cfg.ens_guard) flagged and the host stage sampled again in upstream's summation order, and targets whose
 * region scan (rt1 / rt2 / rt3 against posteriors from the device parsers' rows) had a comparison within 2e-5 of its
 * threshold and was repeated by the host stage on parser rows in upstream's order (active with oa_guard > 0) */
int      p7x_tophits_get_ensemble_counts(const p7x_tophits *th, int64_t *sampled_on_device, int64_t *redone_by_host, int64_t *region_scans_redone);

/* ------------------------------------------------------------------ hmmalign
 * Traces of whole sequences against one profile (TraceAligner.compute_traces, plan7.pyx:9773-9830, upstream
 * p7_tracealign_computeTraces): the profile unihit local with each sequence's own length model; Forward, Backward,
 * posterior decoding, optimal accuracy and its traceback over the whole sequence.  On the device (p7x_align.hip) unless
 * the test seam "host_align" = 1 asks for the host twin; device traces with a near-tie on the trace or a posterior digit
 * within the guard band are repeated by the host twin in upstream's order.  Input: the packed block of
 * p7x_seqdb_create.  P7X_ENODEVICE without a device (and without the seam); P7X_ERANGE when posterior decoding
 * overflows on a sequence (upstream's generic-DP fallback is not implemented; p7x_last_error names the sequence);
 * P7X_EMEM when one sequence alone does not fit the workspace budget ("align_workspace_gb").  host_threads: workers of
 * the host twin (hmmalign's cpus; 0: the library's default). */
typedef struct p7x_traces p7x_traces;
enum { P7X_TRACE_HAS_PP = 1, P7X_TRACE_DEVICE = 2, P7X_TRACE_LOGSPACE = 4 };     /* p7x_traces_get origin bits */
int     p7x_tracealign_compute(const p7x_oprofile *om, int device, const uint8_t *dsq, const int64_t *offsets,
                               const int32_t *lengths, size_t n, int host_threads, p7x_traces **out);
/* The same with options (the call above passes flags = 0).  P7X_ALIGN_LOGSPACE: a sequence whose Backward leaves Forward's
 * scale factors (row sum xB > 1e16: two strong domains of one family), or whose posterior decoding overflows, is aligned
 * by the float64 log-space path instead -- nothing scaled, exact log-sums, optimal accuracy in float64 on the float64
 * posteriors; on the device (p7x_alignlog.hip), with the host log twin (p7x_logdp.cpp) for the traces the device flags
 * and under "host_align".  Such traces carry P7X_TRACE_LOGSPACE, their posteriors are the float64 ones rounded to float,
 * and no sequence raises P7X_ERANGE.  Every other sequence takes the scaled path unchanged.  The test seam
 * "align_logspace" = 1 sends every non-empty sequence through the log-space path, whatever the flag. */
enum { P7X_ALIGN_LOGSPACE = 1 };
int     p7x_tracealign_compute_opts(const p7x_oprofile *om, int device, const uint8_t *dsq, const int64_t *offsets,
                                    const int32_t *lengths, size_t n, int host_threads, int flags, p7x_traces **out);
/* Trace accessors (Traces.__getitem__, Trace.M / L / posterior_probabilities, plan7.pyx:9280-9540): N steps in forward
 * order (P7_TRACE st / k / i / pp), sc2 = Forward score and optimal-accuracy score (nats), the device's status word (0
 * for host-twin traces), origin bits.  copy: st[N] k[N] i[N] pp[N], any of them NULL. */
int64_t p7x_traces_count(const p7x_traces *tr);
int64_t p7x_traces_nflagged(const p7x_traces *tr);           /* device traces the host twin repeated */
/* out4: traces kept from the device, device traces the host twin repeated, device rounds, the largest device workspace
 * (bytes) a round laid out -- at most the budget ("align_workspace_gb") */
int     p7x_traces_stats(const p7x_traces *tr, int64_t out4[4]);
/* out2: sequences the log-space path aligned, and of those the device traces its host twin repeated */
int     p7x_traces_logspace_stats(const p7x_traces *tr, int64_t out2[2]);
int     p7x_traces_get(const p7x_traces *tr, int64_t idx, int32_t *N, int32_t *M, int32_t *L, float *sc2, int32_t *status, uint8_t *origin);
int     p7x_traces_copy(const p7x_traces *tr, int64_t idx, int8_t *st, int32_t *k, int32_t *i, float *pp);
void    p7x_traces_destroy(p7x_traces *tr);

/* The multiple alignment of traces (TraceAligner.align_traces, plan7.pyx:9832-9925, upstream p7_tracealign_Seqs):
 * traces concatenated (toff[n + 1]), origin[n] as above (P7X_TRACE_HAS_PP: the row gets a PP line; with om != NULL a
 * PP_cons column within the guard of a digit boundary is averaged again over host-twin posteriors of its P7X_TRACE_DEVICE
 * rows, the log twin's for rows with P7X_TRACE_LOGSPACE), sequences as for p7x_tracealign_compute, cs = the model's CS line [M+2] or NULL (-> SS_cons).  Rows in text
 * form; P7X_MSA_DIGITIZE is the caller's (easel.DigitalMSA). */
enum { P7X_MSA_TRIM = 1, P7X_MSA_ALL_CONSENSUS_COLS = 2, P7X_MSA_DIGITIZE = 4 };     /* p7_TRIM, p7_ALL_CONSENSUS_COLS, p7_DIGITIZE */
typedef struct p7x_msa p7x_msa;
int     p7x_msa_from_traces(int32_t M, size_t n, const int8_t *st, const int32_t *k, const int32_t *i, const float *pp,
                            const int64_t *toff, const uint8_t *origin, const uint8_t *dsq, const int64_t *offsets,
                            const int32_t *lengths, int32_t abc_type, const char *cs, int flags, const p7x_oprofile *om,
                            p7x_msa **out);
int64_t p7x_msa_alen(const p7x_msa *msa);
/* which: 0 row idx, 1 its PP line ("" when none), 2 PP_cons, 3 RF, 4 SS_cons ("" when none); 5 - 8: see
 * p7x_tophits_to_msa ("" for an alignment made by p7x_msa_from_traces): copies at most cap-1
 * characters and returns the full length, -1 on bad arguments (MSA.alignment / TextMSA, easel.pyx MSA 5790-6400) */
int64_t p7x_msa_get(const p7x_msa *msa, int64_t idx, int which, char *buf, size_t cap);
void    p7x_msa_destroy(p7x_msa *msa);
/* The rows of an alignment made with P7X_MSA_DIGITIZE as digital codes, out[n][alen] row-major (a residue in either case
 * is its code, '-' and '.' the alphabet's gap code): what p7x_msa_counts takes, without a second pass over the text.
 * Returns n * alen and writes the matrix when nbytes holds it; -1 for an alignment made without the flag, and under the
 * test seam "msa_codes" = 0 (the caller then encodes the text rows, as it did before the matrix was kept). */
int64_t p7x_msa_codes(const p7x_msa *msa, uint8_t *out, size_t nbytes);
/* Stockholm text as Easel writes it (MSA.write(fh, "stockholm"), easel.pyx MSA.write; esl_msafile_stockholm.c): names
 * padded to the longest, 200 columns per block, #=GS AC / DE, #=GR PP per row, #=GC SS_cons / PP_cons / RF.  accs,
 * descs, pps and the annotation lines may be NULL (or hold NULL / ""); every row, and every PP / annotation line that is
 * given, must have alen characters.  Returns the length of the text and writes it (not NUL-terminated) when cap is large
 * enough; -1 on bad arguments (a line of another length included). */
int64_t p7x_msa_write_stockholm(size_t n, int64_t alen, const char *const *names, const char *const *accs,
                                const char *const *descs, const char *const *aseqs, const char *const *pps,
                                const char *ss_cons, const char *pp_cons, const char *rf, char *buf, size_t cap);

/* p7_alidisplay_Backconvert (upstream p7_alidisplay.c): the alignment display of one domain -- model line, sequence line,
 * posterior line (or NULL), hmmfrom..hmmto, sqfrom..sqto, target length L -- back to a trace in the arrays
 * p7x_msa_from_traces takes, filled as p7_trace_AppendWithPP fills them (i and pp 0 where nothing is emitted; a PP character
 * decoded as p7_alidisplay_DecodePostProb: '*' 1.0, '.' 0, a digit d d/10, the middle of the values printed as d), and to the digital residues of the aligned
 * subsequence (the display's own text without its gaps).
 *   whole = 0: upstream's faux trace of the SUBSEQUENCE, S N B <one M / D / I per column> E C T, residues numbered from 1
 *     (N = columns + 6, the trace's L is the subsequence's length); what p7_tophits_Alignment aligns.  sqfrom > sqto (the
 *     reverse strand of a long target) is fine: nothing but the text is read.
 *   whole = 1 (an extension): the trace of the whole TARGET the display was cut from: N emits residues 1..sqfrom-1 and C
 *     residues sqto+1..L (posterior 1.0), the core steps carry the target's own coordinates.  Needs sqfrom <= sqto.
 * *N / *subL receive the number of steps and of residues; st / k / i / pp (N entries) and dsq (subL) are written when cap
 * holds them, cap >= N (N <= columns + 6 + L).  P7X_EINVAL when the display is not one (a character outside the alphabet,
 * lines of different lengths, coordinates that do not match the columns). */
int     p7x_alidisplay_backconvert(int32_t abc_type, const char *model, const char *aseq, const char *ppline, int32_t hmmfrom,
                                   int32_t hmmto, int64_t sqfrom, int64_t sqto, int64_t L, int whole, int32_t *N, int32_t *subL,
                                   int8_t *st, int32_t *k, int32_t *i, float *pp, uint8_t *dsq, size_t cap);
/* The alignment of the included domains of a hit list (TopHits.to_msa, plan7.pyx:8966-9069; upstream p7_tophits_Alignment):
 * first the nextra sequences the caller brings with their traces (as for p7x_msa_from_traces; names / accessions /
 * descriptions may be NULL), then, for every hit with P7X_IS_INCLUDED in the list's current order, one row per domain with
 * is_included: the back-converted display (whole = 0), named "<target>/<sqfrom>-<sqto>", with the target's accession and the
 * description "[subseq from] <description, or name>".  M <= 0: the model length the hits carry.  The rows go through
 * p7x_msa_from_traces (flags: P7X_MSA_*; no model annotation, so RF marks the consensus columns and there is no SS_cons);
 * p7x_msa_get gives them back, with which = 5 / 6 / 7 the name / accession / description of row idx and 8 the name of the
 * alignment (the query's).  P7X_EINVAL: nothing to align (no included domain and no extra sequence), the per-sequence lists
 * of a scan, an alphabet other than the hits', an M other than theirs. */
int     p7x_tophits_to_msa(const p7x_tophits *th, int32_t abc_type, int32_t M, size_t nextra, const int8_t *st, const int32_t *k,
                           const int32_t *i, const float *pp, const int64_t *toff, const uint8_t *origin, const uint8_t *dsq,
                           const int64_t *offsets, const int32_t *lengths, const char *const *names, const char *const *accs,
                           const char *const *descs, int flags, p7x_msa **out);
/* Test seams of the two (host code, no device).  from_displays: a hit list of one query (name, alphabet, M) made of the given
 * alignment displays -- hit h has ndom[h] domains, doms in hit order; of a p7x_domain the display fields, is_included and
 * is_reported are read -- with hit flags as given, in the given order.  from_trace: the display p7_alidisplay_Create makes
 * of the first domain of a trace over dsq1[1..L], as the one domain of a one-hit list named <name>. */
int     p7x_debug_tophits_from_displays(const char *qname, int32_t abc_type, int32_t M, size_t nhits, const char *const *names,
                                        const char *const *accs, const char *const *descs, const uint32_t *flags,
                                        const int32_t *ndom, const p7x_domain *doms, p7x_tophits **out);
int     p7x_debug_tophits_from_trace(const p7x_oprofile *om, const uint8_t *dsq1, int32_t L, int32_t N, const int8_t *st,
                                     const int32_t *k, const int32_t *i, const float *pp, const char *name, p7x_tophits **out);

/* ------------------------------------------------------------------ sequence queries (phmmer): p7x_builder.cpp, p7x_calibrate.hip
 * The single-sequence model of a protein (Builder.build, plan7.pyx:911-1016; upstream p7_builder_LoadScoreSystem, p7_Seqmodel,
 * p7_SingleBuilder): M = L nodes; t[(L+1)*7] MM MI MD IM II DM DD, mat / ins[(L+1)*20], caller-allocated.  dsq[0..L-1]: the
 * query's digital residues (a degenerate code gets the normalised sum of its residues' rows).  Host code; no device.
 * P7X_EINVAL: an alphabet other than amino, a score matrix other than "BLOSUM62", a gap or missing-data symbol. */
int p7x_builder_single(int32_t abc_type, const uint8_t *dsq, int32_t L, const float *bg_f, const char *score_matrix,
                       double popen, double pextend, float *t, float *mat, float *ins);
/* The sequences of p7_Calibrate's defaults (upstream evalues.c): P7X_CAL_N samples of 200 residues for the MSV filter, as many
 * of 200 for the Viterbi filter and of 100 for the Forward parser, drawn in that order from one stream (esl_rsq_xfIID over
 * bg_f) of one of Easel's two generators, seeded as esl_randomness_Init seeds it.  out[P7X_CAL_RESIDUES]: the samples end to
 * end, no sentinels.  For one alphabet, background, seed and generator this is a constant. */
#define P7X_CAL_N 200
#define P7X_CAL_RESIDUES 100000
enum { P7X_RNG_MERSENNE = 0, P7X_RNG_FAST = 1 };   /* esl_randomness_Create / esl_randomness_CreateFast */
#define P7X_CAL_GENERATOR P7X_RNG_FAST              /* the one p7x_calibrate_batch draws with: upstream's builder makes its
                                                    * generator with esl_randomness_CreateFast and re-seeds it for every model */
int p7x_calibration_stream(int32_t abc_type, const float *bg_f, uint32_t seed, int generator, uint8_t *out);
/* The same stream for a model some of whose samples overflowed a filter: upstream draws such a sample again, so every
 * later sample moves.  skipped[nskipped]: increasing numbers of the DRAWS (kept or not, counted from 0) that are thrown
 * away; out receives the 600 kept samples.  A model's own stream is found by calling this until no kept sample overflows. */
int p7x_calibration_redraw(int32_t abc_type, const float *bg_f, uint32_t seed, int generator, const int32_t *skipped,
                           int nskipped, uint8_t *out);
/* The number of the draw that kept sample <kept> (0 .. 599) of p7x_calibration_redraw(skipped) is: what the device path adds to
 * <skipped> (increasing) when that sample overflows in its turn. */
int32_t p7x_calibration_draw_of(int32_t kept, const int32_t *skipped, int nskipped);
/* Raw filter results of the MSV and Viterbi samples -> scores in nats as the filters report them under the length model
 * of 200 residues: sc[2 * P7X_CAL_N], overflow[2 * P7X_CAL_N] (xJ < 0, xC = 32767).  The score of an overflowed sample is
 * +inf, as the filters report it; p7x_calibration_fit refuses a marked sample before it reads a score. */
int p7x_calibration_scores(const p7x_oprofile *om, const int32_t *xJ, const int32_t *xC, float *sc, uint8_t *overflow);
/* Test seam: the length model and the score units of the integer filters as every caller in the library takes them.  For
 * each target length L[l]: tjb[l] and xw_move[l], the N/C/J move cost in the MSV filter's bytes and the Viterbi filter's
 * words; usc[l * nJ + i] and vfsc[l * nC + i], the scores in nats of the raw filter results xJ[i] (negative: overflow, +inf)
 * and xC[i] (32767: overflow, +inf; -32768: -inf) under that length.  nJ / nC may be 0. */
int p7x_debug_score_units(const p7x_oprofile *om, const int32_t *L, size_t nL, int32_t *tjb, int32_t *xw_move,
                          const int32_t *xJ, size_t nJ, const int32_t *xC, size_t nC, float *usc, float *vfsc);
/* The fits (p7_Lambda, p7_MSVMu, p7_ViterbiMu, p7_Tau; esl_gumbel_FitCompleteLoc / FitComplete, tail mass 0.04), in double:
 * sc[3 * P7X_CAL_N] scores in nats (MSV, Viterbi, Forward; they enter as (sc - null1(L)) / ln 2), mh = M times the mean
 * match relative entropy in bits (p7x_oprofile_match_relent), out_evparam[6] in the order of P7X_MMU...  overflow
 * [2 * P7X_CAL_N] or NULL: a marked sample makes the call return P7X_ERANGE and fit nothing -- the model must be
 * calibrated on its own stream (p7x_calibration_redraw). */
int p7x_calibration_fit(const float *sc, const uint8_t *overflow, double mh, float *out_evparam);
/* M x p7_MeanMatchRelativeEntropy of the model a profile was made from (0: a pressed profile, which does not carry it) */
double p7x_oprofile_match_relent(const p7x_oprofile *om);
/* p7_Calibrate for a batch of profiles on the device: every profile against the 600 resident samples of its alphabet and
 * background and <seed> (generated once per device and kept; the builder's default seed is 42), one wavefront per (profile, sample), one launch per stage and tier of
 * nodes per lane, no host synchronisation before the one copy of the raw results; then the fits on the host.  A profile
 * with an overflowed sample is calibrated again, alone, on its own stream.  out_evparam[nq][6] is also stored in the
 * profiles.  out_scores (may be NULL): [nq][3][P7X_CAL_N] raw results, xJ and xC as integers, Forward in nats (float
 * bits).  M <= p7x_max_model_length.  P7X_ENODEVICE without a device; P7X_EINVAL for a profile without p7x_oprofile_match_relent. */
int p7x_calibrate_batch(p7x_oprofile *const *oms, size_t nq, int device, uint32_t seed, float *out_evparam, int32_t *out_scores);

/* ------------------------------------------------------------------ sampling: easel.Randomness, p7x_emit.cpp, p7x_emit.hip
 * Easel's generators as easel.Randomness holds them (easel.pyx:7006-7161): state[P7X_RNG_STATE_WORDS] = mt[624], mti, x of
 * ESL_RANDOMNESS.  seed: esl_randomness_Init for one generator (the caller replaces a seed of 0); draw: n calls of
 * esl_random, deviates x / 2^32 in [0, 1).  The unit the calibration stream draws from (p7x_rng.hpp). */
#define P7X_RNG_STATE_WORDS 626
int p7x_rng_seed(int generator, uint32_t seed, uint32_t *state);
int p7x_rng_draw(int generator, uint32_t *state, size_t n, double *out);

/* The cumulative tables (double) every emitter draws from, built once per core model: P7X_EINVAL for a model that
 * cannot be sampled (an insert state that is entered and never left; no residue ever emitted).  info: the expected
 * number of residues of one pass through the core model, and the slot capacity the block emitter starts with (twice
 * that, a multiple of four; debug option "emit_cap" overrides it). */
typedef struct p7x_emit_model p7x_emit_model;
int  p7x_emit_model_create(const p7x_hmm_view *hmm, p7x_emit_model **out);
void p7x_emit_model_destroy(p7x_emit_model *em);
int  p7x_emit_model_info(const p7x_emit_model *em, double *expected_length, int32_t *cap);
/* HMM.emit_sequence / emit_alignment (plan7.pyx:3141-3340; upstream p7_CoreEmit): one path through the core model from
 * node 0 on the generator in <state>, which advances; a path that emits nothing is drawn again.  dsq / st / node[cap]
 * (st, node may be NULL): residues, and the state (p7T_M 1, p7T_I 3) and node that emitted each.  *len residues were
 * emitted; when *len > cap the caller restores the state it had and calls again with room for them.
 * Profile.emit_sequence (plan7.pyx:8109-8194; upstream p7_ProfileEmit): a path through the local multihit profile
 * with length model L; counts[2] (may be NULL): residues emitted by core states, passes through the core.
 * What is claimed is the distribution, not upstream's draw-for-draw stream.  P7X_ERANGE: beyond 100,000 residues. */
int p7x_emit_core(const p7x_emit_model *em, int generator, uint32_t *state, uint8_t *dsq, int8_t *st, int32_t *node, size_t cap, int64_t *len);
int p7x_emit_profile(const p7x_emit_model *em, int32_t L, const float *bg_f, int generator, uint32_t *state, uint8_t *dsq, size_t cap,
                     int64_t *len, int32_t *counts);
/* HMM.emit_block (an extension): n core-model sequences emitted on the device, one lane per sequence, every (sequence,
 * attempt, step) with its own Philox-4x32-10 block keyed by <seed> -- sequence i does not depend on n, the grid or the
 * device.  The block is packed as p7x_seqdb_create takes it (255 x1..xL 255 ...).  p7x_emit_block_host is the host twin:
 * same tables, same generator, same loop, the same bytes; debug option "host_emit" = 1 makes p7x_emit_block call it.
 * P7X_ENODEVICE without a device, P7X_EINVAL for n < 0 or a model beyond p7x_max_model_length, P7X_EMEM when the slots of
 * n sequences do not fit the device's free memory, P7X_ERANGE for a sequence beyond 100,000 residues.
 * info: 0 n, 1 residues, 2 slot capacity of the first pass, 3 sequences drawn again into an exact slot, 4 emitted on the
 * device, 5 has traces, 6 microseconds of the emit kernel's launches (device events). copy: dsq[residues + n + 1], offsets / lengths / attempts[n] (the attempt whose path was kept),
 * with traces st / node[residues + n + 1] laid out as dsq. */
typedef struct p7x_emitted p7x_emitted;
int     p7x_emit_block(const p7x_emit_model *em, int device, int64_t n, uint64_t seed, int want_traces, p7x_emitted **out);
int     p7x_emit_block_host(const p7x_emit_model *em, int64_t n, uint64_t seed, int want_traces, int threads, p7x_emitted **out);
int64_t p7x_emitted_info(const p7x_emitted *b, int which);
int     p7x_emitted_copy(const p7x_emitted *b, uint8_t *dsq, int64_t *offsets, int32_t *lengths, int32_t *attempts, int8_t *st, int32_t *node);
void    p7x_emitted_destroy(p7x_emitted *b);
/* test seams: one Philox-4x32-10 block (key[2], counter[4] -> out[4]); the device bytes the first pass of n sequences
 * takes, P7X_EMEM when they exceed <budget> (negative: no budget) */
int p7x_debug_philox(const uint32_t *key2, const uint32_t *ctr4, uint32_t *out4);
int p7x_debug_emit_bytes(int64_t n, int64_t cap, int traces, int64_t budget, int64_t *bytes);

/* ------------------------------------------------------------------ translation: p7x_translate.cpp, p7x_translate.hip
 * Nucleotide codes ACGT-RYMKSWHBVDN*~ = 0..17 (RNA: U at 3), amino codes as everywhere; definitions: DESIGN.md 3.18.
 * p7x_gencode_table: genetic code <table> (NCBI id): aa64[64] amino codes in NCBI order (first base slowest, each base in
 * the order T, C, A, G), a description, and lut[18 * 18 * 18], indexed (c1 * 18 + c2) * 18 + c3: low seven bits the amino
 * acid (a degenerate codon whose expansions agree translates to what they give, else to X), bit 7 set when the codon holds
 * a gap, * or ~.  Any of the three may be NULL.  P7X_EINVAL for an unknown id.
 * p7x_translate_codons: seq[len] in frame into out[len / 3] on the host; P7X_EINVAL when len is no multiple of three
 * (*err_pos = -1) or a codon has bit 7 (*err_pos = its first base, from 0).
 * p7x_translate_block: the same for every sequence of a block packed as p7x_seqdb_create takes it (255 x1..xL 255 ...,
 * nres residues in all) on <device>: out_dsq[nres / 3 + n + 1] in the same packing, out_offsets / out_lengths[n].
 * P7X_EINVAL with *err_seq and *err_pos for the first sequence whose length is no multiple of three (*err_pos = -1), else
 * for the first codon that cannot be translated.  Debug option "host_translate" = 1 runs the host twin: the same bytes.
 * p7x_orfs_find: the open reading frames of at least min_length codons of both strands (strands: P7X_STRAND_*), in the
 * order sequence, watson before crick, first base along the translated strand.  The unit of work is a span of
 * "orf_chunk" (debug option; 3..384, default 196) positions of the packed array, whatever the sequences: the output does
 * not depend on it.  p7x_orfs_find_host is the twin ("host_translate" = 1 makes p7x_orfs_find call it); p7x_orfs_plan
 * gives the chunk length in force and the chunks a block of nres residues in nseq sequences takes per pass and strand.
 * P7X_ENODEVICE without a device, P7X_EMEM when workspace and output do not fit the device's free memory.
 * info: 0 ORFs, 1 residues, 2 chunks, 3 microseconds of the kernels (device events), 4 found on the device, 5 chunk length,
 * 6-9 microseconds of the passes (summaries, counts, heads, continuations), 10 of the host scans between them.
 * copy: dsq[residues + n + 1], offsets / lengths / source / frame / start / end[n]. */
typedef struct p7x_orfs p7x_orfs;
int     p7x_gencode_table(int32_t table, uint8_t *aa64, char *desc, size_t desc_cap, uint8_t *lut);
int     p7x_translate_codons(int32_t table, const uint8_t *seq, int64_t len, uint8_t *out, int64_t *err_pos);
int     p7x_translate_block(int32_t table, int device, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, size_t n, int64_t nres,
                            uint8_t *out_dsq, int64_t *out_offsets, int32_t *out_lengths, int64_t *err_seq, int64_t *err_pos);
int     p7x_orfs_find(int32_t table, int device, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, size_t n, int64_t nres,
                      int32_t min_length, int strands, p7x_orfs **out);
int     p7x_orfs_find_host(int32_t table, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, size_t n, int64_t nres,
                           int32_t min_length, int strands, int threads, p7x_orfs **out);
int     p7x_orfs_plan(int64_t nres, int64_t nseq, int32_t *orf_chunk, int64_t *chunks);
int64_t p7x_orfs_info(const p7x_orfs *b, int which);
int     p7x_orfs_copy(const p7x_orfs *b, uint8_t *dsq, int64_t *offsets, int32_t *lengths, int64_t *source, int8_t *frame, int64_t *start, int64_t *end);
void    p7x_orfs_destroy(p7x_orfs *b);

/* ------------------------------------------------------------------ decoy sequences: p7x_shuffle.cpp, p7x_shuffle.hip
 * DigitalSequenceBlock.shuffle (an extension; definitions: DESIGN.md 3.19): every sequence of a block packed as
 * p7x_seqdb_create takes it (255 x1..xL 255 ..., nbytes = residues + n + 1) shuffled on <device>, one lane per sequence, into
 * out_dsq[nbytes] in the same packing -- the offsets and lengths of the input hold for the output.  mode: P7X_SHUFFLE_MONO a
 * uniform permutation, _DI a uniform draw among the sequences with the same first residue, last residue and adjacent-pair
 * counts (sequences of fewer than three residues stay), _WINDOW a permutation within consecutive windows of <window>
 * residues, _REVERSE the sequence backwards.  Every digital code is a symbol; abc_type only bounds the codes of _DI.  The
 * draws are Philox-4x32-10 blocks keyed by <seed> with the counter (sequence index, attempt, step): sequence i depends on
 * nothing but itself, its index, the mode, the window and the seed.  p7x_shuffle_host is the twin: same procedure, the same
 * bytes; debug option "host_shuffle" = 1 makes p7x_shuffle_block call it.  A workgroup shuffles a run of consecutive
 * sequences whose span fits "shuffle_slab" (debug option; a multiple of 64 from 64 up, default 65,536; _DI: half of it) bytes
 * of LDS; a sequence that alone does not fit takes a second launch (the long path).  p7x_shuffle_plan gives the runs, the
 * long sequences and the slab in force for lengths[n] (offsets may be NULL).  The output does not depend on the slab.
 * P7X_ENODEVICE without a device (and without the seam); P7X_EINVAL for a block that is not packed as it says, an unknown
 * mode, window < 0, window = 0 with _WINDOW, a code outside the alphabet with _DI; P7X_EMEM when input and output do not
 * fit the device's free memory.
 * stats[5] (may be NULL): nanoseconds of the kernels (device events; wall clock for the twin), nanoseconds of the upload,
 * runs, long sequences, 1 when shuffled on the device. */
enum { P7X_SHUFFLE_MONO = 0, P7X_SHUFFLE_DI = 1, P7X_SHUFFLE_WINDOW = 2, P7X_SHUFFLE_REVERSE = 3 };
int p7x_shuffle_block(int32_t abc_type, int device, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, size_t n, int64_t nbytes,
                      int mode, int32_t window, uint32_t seed, uint8_t *out_dsq, int64_t *stats);
int p7x_shuffle_host(int32_t abc_type, const uint8_t *dsq, const int64_t *offsets, const int32_t *lengths, size_t n, int64_t nbytes, int mode,
                     int32_t window, uint32_t seed, int threads, uint8_t *out_dsq, int64_t *stats);
int p7x_shuffle_plan(const int64_t *offsets, const int32_t *lengths, size_t n, int mode, int64_t *runs, int64_t *long_sequences, int32_t *slab);

/* ------------------------------------------------------------------ Builder.build_msa: p7x_msabuild.cpp, p7x_msabuild.hip
 * A protein alignment as a query (hmmbuild).  ax[N * L]: the digital codes of the rows, one after the other (gap 20).
 * p7x_msa_checksum: Jenkins' one-at-a-time hash over them, the CKSUM of the model.
 * p7x_msa_counts: fragments (rows spanning less than fragthresh of the columns: the cells outside the span are missing
 * data), relative weights (weighting 1: position-based over the columns with a residue share of at least symfrac, or the
 * columns of rf_mask[L] when it is given; 0: none), consensus columns (weighted residue share of at least symfrac, or
 * rf_mask), and the weighted counts of the rows as paths through them.  The passes over the alignment run on <device>;
 * debug option "host_build" = 1 runs their host twin, which gives the same bits: every sum over the rows is a sum of
 * integers (weights in fixed point, unit 2^-40).  "build_rows" = n: rows per block of the kernels.
 * P7X_ERANGE: N > 2^20, L > 65,535, more consensus columns than p7x_max_model_length(); P7X_EINVAL: an empty alignment,
 * no consensus column, an alphabet other than amino; P7X_ENODEVICE without a device (and without the seam).
 * info: 0 N, 1 L, 2 M, 3 weighting columns, 4 counted on the device, 5 fragments, 6-9 nanoseconds of the four passes
 * (column counts, weights, weighted counts, transitions; device events, wall clock for the twin), 10 of the upload.
 * get: 0 uint32[L][32] rows holding each code per column, 1 uint64[N] weights, 2 uint64[L][32] weighted counts per column,
 * 3 int32[M] column of every node (from 0), 4 uint64[M+1][32] weighted counts of every code at every node, 5 uint64[M+1][8]
 * transition counts (MM MI MD IM II DM DD; node 0 is B): the I->I count, which can pass 2^64, is slot 4 (units 2^-40) plus
 * slot 7 (units 2^-20); 6 / 7 the counts as doubles ([M+1][20], degenerate residues
 * spread; [M+1][7]), 8 uint8[L] weighting columns, 9 uint8[N] fragments.
 * p7x_msa_parameterize: priors (0: the amino Dirichlets, 1: Laplace), the effective sequence number (eff_mode 0: N, 1:
 * entropy weighting to max(ere, (esigma + log2(M (M + 1) / 2)) / M) bits per node, ere <= 0: 0.59; 2: eff_value) and the
 * probabilities of the model: t[(M+1)*7], mat / ins[(M+1)*20], caller-allocated; the insert rows are the mean of hmmbuild's
 * insert prior, whatever bg_f holds.  t64 / mat64 (may be NULL): the same probabilities before they are
 * rounded to float.  Host code. */
typedef struct p7x_msacounts p7x_msacounts;
uint32_t p7x_msa_checksum(const uint8_t *ax, size_t n);
int      p7x_msa_counts(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, const uint8_t *rf_mask, int weighting, double symfrac,
                        double fragthresh, int device, p7x_msacounts **out);
int64_t  p7x_msacounts_info(const p7x_msacounts *c, int which);
int      p7x_msacounts_get(const p7x_msacounts *c, int which, void *out, size_t cap_bytes);
void     p7x_msacounts_destroy(p7x_msacounts *c);
int      p7x_msa_parameterize(const p7x_msacounts *c, const float *bg_f, int prior, int eff_mode, double eff_value, double ere, double esigma,
                              float *t, float *mat, float *ins, double *neff, double *t64, double *mat64);

/* ------------------------------------------------------------------ pairwise identity: p7x_msapair.cpp, p7x_msapair.hip
 * The all-pairs fractional identity of the rows of an alignment of any alphabet (ax[N * L] digital codes, as above), and the
 * two things built on it.  len_i: canonical residues of row i; idents_ij: columns where both rows hold the same canonical
 * residue; pid_ij = idents_ij / min(len_i, len_j), 0 when that is 0; two rows are linked when pid_ij >= (double)(float) maxid.
 * The counting runs on <device>; debug option "host_pairid" = 1 runs the host twin, which gives the same bytes: everything is
 * an integer, "linked" included (idents >= need[min len], a table built on the host).  "pairid_tile" = n (1..64): rows per
 * tile side of the kernel, and candidate blocks / bands of two tiles.  P7X_ENODEVICE without a device (and without the seam);
 * P7X_ERANGE beyond the limits; P7X_EINVAL for an empty alignment or a code outside the alphabet.
 * p7x_msa_pair_idents: idents[N][N] and len[N] (may be NULL); N <= 4,096.
 * p7x_msa_idfilter: the greedy identity filter.  Rows are visited in order[N] (a permutation); a row is kept unless it is
 *   linked to a row kept before it.  keep[N]: 1 for the rows kept.  N <= 2^20, L <= 65,535.
 * p7x_msa_linkage: single-linkage clusters of "linked".  cluster[N]: the smallest row index of every row's cluster;
 *   *nclusters (may be NULL).  N <= 2^18: N^2 / 16 bytes of link bits come back from the device (4 GiB at the limit).
 * stats[4] (may be NULL): pairs compared, nanoseconds of the kernels (device events; wall clock for the twin), nanoseconds
 *   of the upload, 1 when counted on the device.
 * p7x_debug_msa_pair_links (test seam): rows_a[na] against rows_b[nb] (row indices): bits[na][(nb + 63) / 64], bit j & 63 of
 *   word j / 64 set when rows_a[i] and rows_b[j] are linked, and any[na], 1 when the row is linked to any of rows_b; either
 *   may be NULL. */
int p7x_msa_pair_idents(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, int device, uint32_t *idents, uint32_t *len);
int p7x_msa_idfilter(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, const int64_t *order, double maxid, int device,
                     uint8_t *keep, int64_t *stats);
int p7x_msa_linkage(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, double maxid, int device, int32_t *cluster,
                    int64_t *nclusters, int64_t *stats);
int p7x_debug_msa_pair_links(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, double maxid, int device, const int32_t *rows_a,
                             int64_t na, const int32_t *rows_b, int64_t nb, uint64_t *bits, uint8_t *any);

const char *p7x_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* P7X_H */
