// p7x_translate.hpp -- nucleotide to protein: the genetic codes, the codon lookup that the host twin and the kernels both
// read, the in-frame translation of a packed block and the six-frame ORF finder (p7x_translate.cpp: tables and host twin;
// p7x_translate.hip: the kernels).  Definitions: DESIGN.md 3.18.
#pragma once
#include "p7x_internal.hpp"
#include <cstdint>
#include <string>
#include <vector>

namespace p7x {

constexpr int kNtKp = 18;                       // ACGT-RYMKSWHBVDN*~
constexpr int kCodonLut = kNtKp * kNtKp * kNtKp; // 5,832
constexpr uint8_t kAaX = 26, kAaStop = 27;      // amino codes of X and *
constexpr uint8_t kLutAmino = 0x7f;             // lut byte: the amino acid ...
constexpr uint8_t kLutUntranslatable = 0x80;    // ... and whether the codon holds a gap, * or ~ (translate refuses it; the ORF finder reads X)
constexpr int kOrfChunkDefault = 196;           // nucleotides per unit of work: 49 dwords, so the lanes of a wavefront walk 32 different LDS banks
constexpr int kOrfChunkMin = 3, kOrfChunkMax = 384;

struct GeneticCodeTable {
  int id = 0;
  std::string desc;
  uint8_t aa64[64];                             // NCBI order: first base slowest, each base in the order T, C, A, G
  uint8_t lut[kCodonLut];                       // [(c1 * 18 + c2) * 18 + c3] over Easel's nucleotide codes
};
// the table of a genetic code (built once per id, kept for the life of the process); nullptr and an error for an unknown id
const GeneticCodeTable *genetic_code(int id);
extern const uint8_t kNtComplement[kNtKp];      // A<->T C<->G R<->Y M<->K H<->D B<->V; S W N - * ~ stay

// In-frame translation of sequence <dsq[0..L)> (L a multiple of three): -1, or the index of the first codon base that
// cannot be translated.
int64_t translate_codons(const GeneticCodeTable &gc, const uint8_t *dsq, int64_t L, uint8_t *out);

// the units of work of the ORF finder over a packed block of <nres> residues in <nseq> sequences: option "orf_chunk"
// when set (clamped), else the default; chunks = ceil((nres + nseq + 1) / chunk)
void orf_plan(int64_t nres, int64_t nseq, int32_t *chunk, int64_t *chunks);

} // namespace p7x

struct p7x_orfs {                               // packed as easel.PackedBlock: 255 orf1 255 orf2 255 ...
  int64_t n = 0, nres = 0;
  int64_t chunks = 0;                           // units of work per pass and strand
  int32_t chunk = 0;
  int on_device = 0;
  double pass_us[4] = { 0, 0, 0, 0 };           // device time of the passes (summaries, counts, heads, continuations), both strands, from events
  double stitch_us = 0;                         // host time of the two scans between them
  std::vector<uint8_t> dsq;                     // [nres + n + 1]
  std::vector<int64_t> offsets, source, start, end;   // [n]
  std::vector<int32_t> lengths;                 // [n]
  std::vector<int8_t> frame;                    // [n] +1..+3 watson, -1..-3 crick
};

namespace p7x {

struct PackedView { const uint8_t *dsq; const int64_t *offsets; const int32_t *lengths; int64_t n; int64_t nres; };
// the packing is what it says it is: a sentinel before every sequence and after the last; P7X_EINVAL otherwise
int check_packing(const PackedView &in);
// host twins
int orfs_find_host(const GeneticCodeTable &gc, const PackedView &in, int32_t min_length, int strands, int threads, p7x_orfs &out);
int translate_block_host(const GeneticCodeTable &gc, const PackedView &in, uint8_t *out_dsq, int64_t *out_offsets, int32_t *out_lengths,
                         int64_t *err_seq, int64_t *err_pos);
// the checks of translate_block that need no residue: the first sequence whose length is no multiple of three
int translate_block_lengths(const PackedView &in, int64_t *err_seq, int64_t *err_pos);
// device paths (p7x_translate.hip)
int orfs_find_device(const GeneticCodeTable &gc, int device, const PackedView &in, int32_t min_length, int strands, p7x_orfs &out);
int translate_block_device(const GeneticCodeTable &gc, int device, const PackedView &in, uint8_t *out_dsq, int64_t *out_offsets,
                           int32_t *out_lengths, int64_t *err_seq, int64_t *err_pos);

} // namespace p7x
