// p7x_translate.cpp -- the genetic codes and the codon lookup, and the host twins of p7x_translate.hip: in-frame translation
// of a packed block and the six-frame ORF finder, in plain C++.  GeneticCode.translate and
// DigitalSequence.translate are served from here; option "host_translate" sends the block entry points here too.
#include "p7x_translate.hpp"
#include "p7x.h"
#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

namespace p7x {

// ------------------------------------------------------------------------------------------------ genetic codes
static const char kStandard[65] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
static const char kAminoSyms[30] = "ACDEFGHIKLMNPQRSTVWY-BJZOUX*~";

struct CodeDiff { int id; const char *desc; const char *changes; };      // changes: "AGA* AGG* ATAM ..." (codon, new letter)
static const CodeDiff kCodes[] = {
  { 1, "Standard", "" },
  { 2, "Vertebrate Mitochondrial", "AGA* AGG* ATAM TGAW" },
  { 3, "Yeast Mitochondrial", "ATAM CTTT CTCT CTAT CTGT TGAW" },
  { 4, "Mold, Protozoan and Coelenterate Mitochondrial; Mycoplasma and Spiroplasma", "TGAW" },
  { 5, "Invertebrate Mitochondrial", "AGAS AGGS ATAM TGAW" },
  { 6, "Ciliate, Dasycladacean and Hexamita Nuclear", "TAAQ TAGQ" },
  { 9, "Echinoderm and Flatworm Mitochondrial", "AAAN AGAS AGGS TGAW" },
  { 10, "Euplotid Nuclear", "TGAC" },
  { 11, "Bacterial, Archaeal and Plant Plastid", "" },
  { 12, "Alternative Yeast Nuclear", "CTGS" },
  { 13, "Ascidian Mitochondrial", "AGAG AGGG ATAM TGAW" },
  { 14, "Alternative Flatworm Mitochondrial", "AAAN AGAS AGGS TAAY TGAW" },
  { 16, "Chlorophycean Mitochondrial", "TAGL" },
  { 21, "Trematode Mitochondrial", "TGAW ATAM AGAS AGGS AAAN" },
  { 22, "Scenedesmus obliquus Mitochondrial", "TCA* TAGL" },
  { 23, "Thraustochytrium Mitochondrial", "TTA*" },
  { 24, "Pterobranchia Mitochondrial", "AGAS AGGK TGAW" },
  { 25, "Candidate Division SR1 and Gracilibacteria", "TGAG" },
};

const uint8_t kNtComplement[kNtKp] = { 3, 2, 1, 0, 4, 6, 5, 8, 7, 9, 10, 14, 13, 12, 11, 15, 16, 17 };

static int tcag_of_letter(char c) { return c == 'T' ? 0 : c == 'C' ? 1 : c == 'A' ? 2 : 3; }
static uint8_t amino_code(char c) { return (uint8_t) (std::strchr(kAminoSyms, c) - kAminoSyms); }

static void build_table(const CodeDiff &d, GeneticCodeTable &t)
{
  t.id = d.id; t.desc = d.desc;
  char letters[65];
  std::memcpy(letters, kStandard, 65);
  for (const char *p = d.changes; *p; ) {
    letters[16 * tcag_of_letter(p[0]) + 4 * tcag_of_letter(p[1]) + tcag_of_letter(p[2])] = p[3];
    p += 4;
    while (*p == ' ') ++p;
  }
  for (int i = 0; i < 64; ++i) t.aa64[i] = amino_code(letters[i]);
  // the bases a nucleotide code stands for, as a mask over Easel's A C G T = bits 0..3; 0: gap, * and ~
  static const uint8_t set_of[kNtKp] = { 1, 2, 4, 8, 0, 1 | 4, 2 | 8, 1 | 2, 4 | 8, 2 | 4, 1 | 8, 1 | 2 | 8, 2 | 4 | 8, 1 | 2 | 4, 1 | 4 | 8, 15, 0, 0 };
  static const int tcag_of_base[4] = { 2, 1, 3, 0 };
  for (int c1 = 0; c1 < kNtKp; ++c1)
    for (int c2 = 0; c2 < kNtKp; ++c2)
      for (int c3 = 0; c3 < kNtKp; ++c3) {
        uint8_t &cell = t.lut[(c1 * kNtKp + c2) * kNtKp + c3];
        if (!set_of[c1] || !set_of[c2] || !set_of[c3]) { cell = kAaX | kLutUntranslatable; continue; }
        int aa = -1;
        for (int b1 = 0; b1 < 4; ++b1) if (set_of[c1] >> b1 & 1)
          for (int b2 = 0; b2 < 4; ++b2) if (set_of[c2] >> b2 & 1)
            for (int b3 = 0; b3 < 4; ++b3) if (set_of[c3] >> b3 & 1) {
              const int a = t.aa64[16 * tcag_of_base[b1] + 4 * tcag_of_base[b2] + tcag_of_base[b3]];
              aa = aa < 0 ? a : (aa == a ? a : kAaX);
            }
        cell = (uint8_t) aa;
      }
}

const GeneticCodeTable *genetic_code(int id)
{
  static std::mutex mu;
  static std::map<int, std::unique_ptr<GeneticCodeTable>> *built = new std::map<int, std::unique_ptr<GeneticCodeTable>>();
  std::lock_guard<std::mutex> lk(mu);
  auto it = built->find(id);
  if (it != built->end()) return it->second.get();
  for (const CodeDiff &d : kCodes)
    if (d.id == id) {
      auto t = std::make_unique<GeneticCodeTable>();
      build_table(d, *t);
      return ((*built)[id] = std::move(t)).get();
    }
  set_error("unknown translation table " + std::to_string(id));
  return nullptr;
}

// ------------------------------------------------------------------------------------------------ in-frame translation
int64_t translate_codons(const GeneticCodeTable &gc, const uint8_t *dsq, int64_t L, uint8_t *out)
{
  for (int64_t k = 0; 3 * k + 2 < L; ++k) {
    const uint8_t a = dsq[3 * k], b = dsq[3 * k + 1], c = dsq[3 * k + 2];
    if (a >= kNtKp || b >= kNtKp || c >= kNtKp) return 3 * k;
    const uint8_t v = gc.lut[(a * kNtKp + b) * kNtKp + c];
    if (v & kLutUntranslatable) return 3 * k;
    out[k] = v;
  }
  return -1;
}

int check_packing(const PackedView &in)
{
  if (in.n < 0 || (in.n && (!in.offsets || !in.lengths)) || !in.dsq) { set_error("translate: bad packed block"); return P7X_EINVAL; }
  int64_t pos = 1;
  if (in.dsq[0] != 255) { set_error("translate: the packed block does not start with a sentinel"); return P7X_EINVAL; }
  for (int64_t s = 0; s < in.n; ++s) {
    if (in.lengths[s] < 0 || in.offsets[s] != pos || in.dsq[pos + in.lengths[s]] != 255) {
      set_error("translate: sequence " + std::to_string(s) + " is not packed as 255 x1..xL 255");
      return P7X_EINVAL;
    }
    pos += (int64_t) in.lengths[s] + 1;
  }
  if (pos != in.nres + in.n + 1) { set_error("translate: the lengths of the packed block do not add up"); return P7X_EINVAL; }
  return P7X_OK;
}

int translate_block_lengths(const PackedView &in, int64_t *err_seq, int64_t *err_pos)
{
  for (int64_t s = 0; s < in.n; ++s)
    if (in.lengths[s] % 3 != 0) {
      if (err_seq) *err_seq = s;
      if (err_pos) *err_pos = -1;
      set_error("Incomplete sequence of length " + std::to_string(in.lengths[s]) + " at index " + std::to_string(s));
      return P7X_EINVAL;
    }
  return P7X_OK;
}

int translate_block_host(const GeneticCodeTable &gc, const PackedView &in, uint8_t *out_dsq, int64_t *out_offsets, int32_t *out_lengths,
                         int64_t *err_seq, int64_t *err_pos)
{
  int st = translate_block_lengths(in, err_seq, err_pos);
  if (st != P7X_OK) return st;
  int64_t pos = 1;
  out_dsq[0] = 255;
  for (int64_t s = 0; s < in.n; ++s) {
    const int64_t L = in.lengths[s];
    const int64_t bad = translate_codons(gc, in.dsq + in.offsets[s], L, out_dsq + pos);
    if (bad >= 0) {
      if (err_seq) *err_seq = s;
      if (err_pos) *err_pos = bad;
      set_error("Failed to translate codon at index " + std::to_string(bad) + " of sequence " + std::to_string(s));
      return P7X_EINVAL;
    }
    out_offsets[s] = pos; out_lengths[s] = (int32_t) (L / 3);
    pos += L / 3;
    out_dsq[pos++] = 255;
  }
  return P7X_OK;
}

// ------------------------------------------------------------------------------------------------ ORF finder, host twin
void orf_plan(int64_t nres, int64_t nseq, int32_t *chunk, int64_t *chunks)
{
  int c = debug_opt(OPT_ORF_CHUNK);
  if (c <= 0) c = kOrfChunkDefault;
  c = std::min(std::max(c, kOrfChunkMin), kOrfChunkMax);
  if (chunk) *chunk = c;
  if (chunks) *chunks = (nres + nseq + 1 + c - 1) / c;
}

namespace {

struct OrfPiece {                 // the ORFs of a range of sequences, in output order
  std::vector<uint8_t> res;       // orf1 255 orf2 255 ...
  std::vector<int64_t> source, start, end;
  std::vector<int32_t> lengths;
  std::vector<int8_t> frame;
};

struct Run { int64_t head; int64_t len; };

// the ORFs of one strand of one sequence: s[0..L) is the translated strand
void strand_orfs(const GeneticCodeTable &gc, const uint8_t *s, int64_t L, int32_t min_length, std::vector<Run> &runs, std::vector<uint8_t> &aa)
{
  runs.clear();
  aa.assign((size_t) std::max<int64_t>(L - 2, 0), kAaStop);
  for (int64_t t = 0; t + 2 < L; ++t) {
    const uint8_t a = s[t], b = s[t + 1], c = s[t + 2];
    aa[t] = (a >= kNtKp || b >= kNtKp || c >= kNtKp) ? kAaStop : (uint8_t) (gc.lut[(a * kNtKp + b) * kNtKp + c] & kLutAmino);
  }
  for (int f = 0; f < 3; ++f) {
    int64_t head = -1;
    for (int64_t t = f; ; t += 3) {
      const bool stop = t + 2 >= L || aa[t] == kAaStop;
      if (!stop) { if (head < 0) head = t; continue; }
      if (head >= 0 && (t - head) / 3 >= min_length) runs.push_back({ head, (t - head) / 3 });
      head = -1;
      if (t + 2 >= L) break;
    }
  }
  std::sort(runs.begin(), runs.end(), [](const Run &x, const Run &y) { return x.head < y.head; });
}

void range_orfs(const GeneticCodeTable &gc, const PackedView &in, int64_t s0, int64_t s1, int32_t min_length, int strands, OrfPiece &out)
{
  std::vector<Run> runs;
  std::vector<uint8_t> aa, rc;
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t L = in.lengths[s];
    const uint8_t *x = in.dsq + in.offsets[s];
    for (int crick = 0; crick < 2; ++crick) {
      if (strands == (crick ? P7X_STRAND_TOPONLY : P7X_STRAND_BOTTOMONLY)) continue;
      const uint8_t *str = x;
      if (crick) {
        rc.resize((size_t) L);
        for (int64_t i = 0; i < L; ++i) { const uint8_t v = x[L - 1 - i]; rc[i] = v < kNtKp ? kNtComplement[v] : v; }
        str = rc.data();
      }
      strand_orfs(gc, str, L, min_length, runs, aa);
      for (const Run &r : runs) {
        for (int64_t k = 0; k < r.len; ++k) out.res.push_back(aa[r.head + 3 * k]);
        out.res.push_back(255);
        const int f = (int) (r.head % 3) + 1;
        out.source.push_back(s); out.lengths.push_back((int32_t) r.len);
        out.frame.push_back((int8_t) (crick ? -f : f));
        if (!crick) { out.start.push_back(r.head + 1); out.end.push_back(r.head + 3 * r.len); }
        else { out.start.push_back(L - r.head); out.end.push_back(L - r.head - 3 * r.len + 1); }
      }
    }
  }
}

} // namespace

int orfs_find_host(const GeneticCodeTable &gc, const PackedView &in, int32_t min_length, int strands, int threads, p7x_orfs &out)
{
  out = p7x_orfs();
  orf_plan(in.nres, in.n, &out.chunk, &out.chunks);
  // ranges of whole sequences of about equal residues, several per worker; a single contig is one range
  if (threads <= 0) threads = (int) std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
  const int64_t per = std::max<int64_t>(1 << 16, (in.nres + in.n) / (4 * (int64_t) threads) + 1);
  std::vector<int64_t> cut{ 0 };
  for (int64_t s = 0, acc = 0; s < in.n; ++s) {
    acc += (int64_t) in.lengths[s] + 1;
    if (acc >= per && s + 1 < in.n) { cut.push_back(s + 1); acc = 0; }
  }
  cut.push_back(in.n);
  const size_t nr = cut.size() - 1;
  std::vector<OrfPiece> pieces(nr);
  std::atomic<size_t> next{ 0 };
  auto work = [&] { for (size_t r; (r = next.fetch_add(1)) < nr; ) range_orfs(gc, in, cut[r], cut[r + 1], min_length, strands, pieces[r]); };
  const int nw = (int) std::min<size_t>((size_t) threads, nr);
  std::vector<std::thread> pool;
  for (int w = 1; w < nw; ++w) pool.emplace_back(work);
  work();
  for (auto &t : pool) t.join();
  size_t n = 0, bytes = 1;
  for (const OrfPiece &p : pieces) { n += p.source.size(); bytes += p.res.size(); }
  out.n = (int64_t) n; out.nres = (int64_t) (bytes - 1 - n);
  out.dsq.reserve(bytes); out.dsq.push_back(255);
  out.offsets.reserve(n); out.source.reserve(n); out.start.reserve(n); out.end.reserve(n); out.lengths.reserve(n); out.frame.reserve(n);
  for (const OrfPiece &p : pieces) {
    int64_t pos = (int64_t) out.dsq.size();
    for (int32_t len : p.lengths) { out.offsets.push_back(pos); pos += (int64_t) len + 1; }
    out.dsq.insert(out.dsq.end(), p.res.begin(), p.res.end());
    out.source.insert(out.source.end(), p.source.begin(), p.source.end());
    out.start.insert(out.start.end(), p.start.begin(), p.start.end());
    out.end.insert(out.end.end(), p.end.begin(), p.end.end());
    out.lengths.insert(out.lengths.end(), p.lengths.begin(), p.lengths.end());
    out.frame.insert(out.frame.end(), p.frame.begin(), p.frame.end());
  }
  return P7X_OK;
}

} // namespace p7x

using namespace p7x;

extern "C" {

int p7x_gencode_table(int32_t id, uint8_t *aa64, char *desc, size_t desc_cap, uint8_t *lut)
{
  const GeneticCodeTable *gc = genetic_code(id);
  if (!gc) return P7X_EINVAL;
  if (aa64) std::memcpy(aa64, gc->aa64, 64);
  if (lut) std::memcpy(lut, gc->lut, kCodonLut);
  if (desc && desc_cap) { std::strncpy(desc, gc->desc.c_str(), desc_cap - 1); desc[desc_cap - 1] = 0; }
  return P7X_OK;
}

int p7x_translate_codons(int32_t id, const uint8_t *seq, int64_t len, uint8_t *out, int64_t *err_pos)
{
  const GeneticCodeTable *gc = genetic_code(id);
  if (!gc) return P7X_EINVAL;
  if (len < 0 || (len && (!seq || !out))) { set_error("p7x_translate_codons: bad arguments"); return P7X_EINVAL; }
  if (err_pos) *err_pos = -1;
  if (len % 3 != 0) { set_error("Invalid sequence of length " + std::to_string(len)); return P7X_EINVAL; }
  const int64_t bad = translate_codons(*gc, seq, len, out);
  if (bad >= 0) {
    if (err_pos) *err_pos = bad;
    set_error("Failed to translate codon at index " + std::to_string(bad));
    return P7X_EINVAL;
  }
  return P7X_OK;
}

int p7x_orfs_plan(int64_t nres, int64_t nseq, int32_t *orf_chunk, int64_t *chunks)
{
  if (nres < 0 || nseq < 0) { set_error("p7x_orfs_plan: bad arguments"); return P7X_EINVAL; }
  orf_plan(nres, nseq, orf_chunk, chunks);
  return P7X_OK;
}

int64_t p7x_orfs_info(const p7x_orfs *b, int which)
{
  if (!b) return -1;
  switch (which) {
    case 0: return b->n;
    case 1: return b->nres;
    case 2: return b->chunks;
    case 3: return (int64_t) (b->pass_us[0] + b->pass_us[1] + b->pass_us[2] + b->pass_us[3]);
    case 4: return b->on_device;
    case 5: return b->chunk;
    case 6: case 7: case 8: case 9: return (int64_t) b->pass_us[which - 6];
    case 10: return (int64_t) b->stitch_us;
    default: return -1;
  }
}

int p7x_orfs_copy(const p7x_orfs *b, uint8_t *dsq, int64_t *offsets, int32_t *lengths, int64_t *source, int8_t *frame, int64_t *start, int64_t *end)
{
  if (!b || !dsq) { set_error("p7x_orfs_copy: bad arguments"); return P7X_EINVAL; }
  std::memcpy(dsq, b->dsq.data(), b->dsq.size());
  const size_t n = (size_t) b->n;
  if (n) {
    if (offsets) std::memcpy(offsets, b->offsets.data(), n * sizeof(int64_t));
    if (lengths) std::memcpy(lengths, b->lengths.data(), n * sizeof(int32_t));
    if (source) std::memcpy(source, b->source.data(), n * sizeof(int64_t));
    if (frame) std::memcpy(frame, b->frame.data(), n * sizeof(int8_t));
    if (start) std::memcpy(start, b->start.data(), n * sizeof(int64_t));
    if (end) std::memcpy(end, b->end.data(), n * sizeof(int64_t));
  }
  return P7X_OK;
}

void p7x_orfs_destroy(p7x_orfs *b) { delete b; }

} // extern "C"
