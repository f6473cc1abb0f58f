// p7x_msapair.cpp -- pairwise identity of the rows of an alignment: identity filter and single-linkage clusters.
//
// Host code.  Restated from the published behaviour of Easel's esl_dst_XPairId, esl_msaweight_IDFilter and
// esl_msaweight_BLOSUM: pid_ij = identical canonical residues / min(len_i, len_j); two rows are linked
// when pid_ij >= the threshold as a C float.  The N^2 / 2 x L part runs on the device (p7x_msapair.hip); what is here is
// the two byte images and the table need[] that turn "linked" into an integer comparison, the drivers -- the filter's
// sequential greedy over candidate blocks, the clusters' union-find over streamed link bits -- and the host twin of the
// kernel (debug option "host_pairid" = 1), which is used for nothing else.
#include "p7x_msapair.hpp"
#include "p7x_host.hpp"
#include <algorithm>
#include <chrono>
#include <cstring>

namespace p7x {

static int pair_images(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, int64_t max_rows, const char *what, PairImages &img)
{
  if (abc_type != P7X_AMINO && abc_type != P7X_DNA && abc_type != P7X_RNA) { set_error("pairwise identity: unknown alphabet"); return P7X_EINVAL; }
  if (!ax || N < 1 || L < 1) { set_error("the alignment is empty"); return P7X_EINVAL; }
  if (N > max_rows) { set_error(std::string(what) + ": the alignment has " + std::to_string(N) + " rows, more than " + std::to_string(max_rows)); return P7X_ERANGE; }
  if (L > kPairMaxCols) { set_error("the alignment has " + std::to_string(L) + " columns, more than 65,535"); return P7X_ERANGE; }
  const Alphabet &abc = Alphabet::get(abc_type);
  const unsigned K = (unsigned) abc.K, Kp = (unsigned) abc.Kp;
  img.N = N; img.L = L; img.Lp = (L + 3) / 4 * 4;
  img.a.assign((size_t) N * img.Lp, kPairOtherA);
  img.b.assign((size_t) N * img.Lp, kPairOtherB);
  img.len.assign((size_t) N, 0);
  bool bad = false;
  for (int64_t i = 0; i < N; ++i) {
    const uint8_t *src = ax + (size_t) i * L;
    uint8_t *da = img.a.data() + (size_t) i * img.Lp, *db = img.b.data() + (size_t) i * img.Lp;
    uint32_t len = 0;
    for (int c = 0; c < L; ++c) {
      const unsigned a = src[c];
      bad |= a >= Kp;
      da[c] = pair_code_a(a, K); db[c] = pair_code_b(a, K);
      len += pair_is_canonical(a, K);
    }
    img.len[(size_t) i] = len;
  }
  if (bad) { set_error("the alignment holds a code outside the alphabet"); return P7X_EINVAL; }
  return P7X_OK;
}

// ---------------------------------------------------------------- the host twin of pair_tile_kernel
static uint32_t twin_idents(const PairImages &img, int64_t i, int64_t j)
{
  const uint32_t *a = reinterpret_cast<const uint32_t *>(img.a.data() + (size_t) i * img.Lp);
  const uint32_t *b = reinterpret_cast<const uint32_t *>(img.b.data() + (size_t) j * img.Lp);
  uint32_t diff = 0;
  for (int k = 0; k < img.Lp / 4; ++k) diff = pair_dword_diff(diff, a[k], b[k]);
  return (uint32_t) img.Lp - diff;
}

static void twin_run(const PairImages &img, const std::vector<uint32_t> &need, const PairJob &job, PairStats &st)
{
  const int64_t words = (job.nb + 63) / 64;
  if (job.bits) std::memset(job.bits, 0, (size_t) job.na * (size_t) words * sizeof(uint64_t));
  if (job.any) std::memset(job.any, 0, (size_t) job.na);
  if (job.idents) std::memset(job.idents, 0, (size_t) job.na * (size_t) job.nb * sizeof(uint32_t));
  for (int64_t i = 0; i < job.na; ++i) {
    const int64_t ri = job.rows_a ? job.rows_a[i] : job.base_a + i;
    for (int64_t j = 0; j < job.nb; ++j) {
      if (job.lower && job.base_b + j > job.base_a + i) break;
      const int64_t rj = job.rows_b ? job.rows_b[j] : job.base_b + j;
      const uint32_t idents = twin_idents(img, ri, rj);
      ++st.pairs;
      if (job.idents) job.idents[i * job.nb + j] = idents;
      if (pair_linked(idents, img.len[(size_t) ri], img.len[(size_t) rj], need.data())) {
        if (job.bits) job.bits[i * words + (j >> 6)] |= (uint64_t) 1 << (j & 63);
        if (job.any) job.any[i] = 1;
      }
    }
  }
}

// ---------------------------------------------------------------- one engine for the drivers: the device, or the twin
struct PairEngine {
  PairImages img;
  std::vector<uint32_t> need;
  PairDevice *dev = nullptr;
  bool host = false;
  int tile = kPairTileMax;
  bool seam_tile = false;
  PairStats st;
  ~PairEngine() { if (dev) pair_device_close(dev); }

  int open(int device, double maxid)
  {
    pair_need_table((double) (float) maxid, img.L, need);
    host = debug_opt(OPT_HOST_PAIRID) > 0;
    const int t = debug_opt(OPT_PAIRID_TILE);
    if (t > 0) { tile = std::min(t, kPairTileMax); seam_tile = true; }
    return host ? P7X_OK : pair_device_open(device, img, need, tile, st, &dev);
  }
  int run(const PairJob &job)
  {
    if (!host) return pair_device_run(dev, job, st);
    const auto t0 = std::chrono::steady_clock::now();
    twin_run(img, need, job, st);
    st.kernel_ns += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    return P7X_OK;
  }
  void report(int64_t *stats) const
  {
    if (!stats) return;
    stats[0] = st.pairs; stats[1] = (int64_t) st.kernel_ns; stats[2] = (int64_t) st.upload_ns; stats[3] = st.on_device;
  }
};

// ---------------------------------------------------------------- the identity filter: the sequential greedy
// Candidates in the order of the preference, a block at a time: against everything kept so far only "linked to any" comes
// back, against each other the block's link bits; the host then walks the block in order.
static int idfilter(PairEngine &e, const int64_t *order, uint8_t *keep)
{
  const int64_t N = e.img.N;
  std::vector<uint8_t> seen((size_t) N, 0);
  for (int64_t c = 0; c < N; ++c) {
    if (order[c] < 0 || order[c] >= N || seen[(size_t) order[c]]) { set_error("identity filter: the order is no permutation of the rows"); return P7X_EINVAL; }
    seen[(size_t) order[c]] = 1;
  }
  std::memset(keep, 0, (size_t) N);
  const int64_t block = (int64_t) e.tile * (e.seam_tile ? 2 : kPairBlockTiles);
  std::vector<int32_t> kept, cand;
  std::vector<uint8_t> any;
  std::vector<uint64_t> bits, mask;
  for (int64_t c0 = 0; c0 < N; c0 += block) {
    const int64_t nb = std::min(block, N - c0), words = (nb + 63) / 64;
    cand.resize((size_t) nb);
    for (int64_t c = 0; c < nb; ++c) cand[(size_t) c] = (int32_t) order[c0 + c];
    any.assign((size_t) nb, 0);
    bits.assign((size_t) nb * (size_t) words, 0);
    int rc;
    if (!kept.empty()) {
      PairJob j; j.rows_a = cand.data(); j.na = nb; j.rows_b = kept.data(); j.nb = (int64_t) kept.size(); j.any = any.data();
      if ((rc = e.run(j)) != P7X_OK) return rc;
    }
    {
      PairJob j; j.rows_a = cand.data(); j.na = nb; j.rows_b = cand.data(); j.nb = nb; j.lower = true; j.bits = bits.data();
      if ((rc = e.run(j)) != P7X_OK) return rc;
    }
    mask.assign((size_t) words, 0);                 // the rows of this block that were kept
    for (int64_t c = 0; c < nb; ++c) {
      bool linked = any[(size_t) c] != 0;
      for (int64_t w = 0; !linked && w <= c / 64; ++w) {
        uint64_t m = bits[(size_t) (c * words + w)] & mask[(size_t) w];
        if (w == c / 64) m &= ((uint64_t) 1 << (c & 63)) - 1;      // rows before this one
        linked = m != 0;
      }
      if (linked) continue;
      mask[(size_t) (c / 64)] |= (uint64_t) 1 << (c & 63);
      kept.push_back(cand[(size_t) c]);
      keep[cand[(size_t) c]] = 1;
    }
  }
  return P7X_OK;
}

// ---------------------------------------------------------------- single-linkage clusters: union-find over the link bits
struct UnionFind {
  std::vector<int32_t> parent;
  explicit UnionFind(int64_t n) : parent((size_t) n) { for (int64_t i = 0; i < n; ++i) parent[(size_t) i] = (int32_t) i; }
  int32_t find(int32_t x)
  {
    while (parent[(size_t) x] != x) { parent[(size_t) x] = parent[(size_t) parent[(size_t) x]]; x = parent[(size_t) x]; }
    return x;
  }
  // the root is the smaller index, so a cluster's root is its smallest row
  void unite(int32_t a, int32_t b)
  {
    a = find(a); b = find(b);
    if (a == b) return;
    if (a < b) parent[(size_t) b] = a; else parent[(size_t) a] = b;
  }
};

static void visit_band(void *user, int64_t i0, int64_t i1, int64_t words, const uint64_t *bits)
{
  UnionFind &uf = *static_cast<UnionFind *>(user);
  for (int64_t i = i0; i < i1; ++i) {
    const uint64_t *row = bits + (size_t) (i - i0) * (size_t) words;
    for (int64_t w = 0; w <= i / 64; ++w) {
      uint64_t m = row[w];
      if (w == i / 64) m &= ((uint64_t) 1 << (i & 63)) - 1;
      while (m) { const int b = __builtin_ctzll(m); m &= m - 1; uf.unite((int32_t) i, (int32_t) (w * 64 + b)); }
    }
  }
}

static int linkage(PairEngine &e, int32_t *cluster, int64_t *nclusters)
{
  const int64_t N = e.img.N;
  UnionFind uf(N);
  if (!e.host) {
    const int rc = pair_device_bands(e.dev, N, visit_band, &uf, e.st);
    if (rc != P7X_OK) return rc;
  } else {
    // the twin: the same bands, one tile of rows at a time
    std::vector<uint64_t> bits;
    const int64_t band = e.tile;
    for (int64_t i0 = 0; i0 < N; i0 += band) {
      const int64_t i1 = std::min(N, i0 + band), words = (i1 + 63) / 64;
      bits.assign((size_t) (i1 - i0) * (size_t) words, 0);
      PairJob j; j.base_a = i0; j.na = i1 - i0; j.base_b = 0; j.nb = i1; j.lower = true; j.bits = bits.data();
      const int rc = e.run(j);
      if (rc != P7X_OK) return rc;
      visit_band(&uf, i0, i1, words, bits.data());
    }
  }
  int64_t n = 0;
  for (int64_t i = 0; i < N; ++i) { cluster[i] = uf.find((int32_t) i); n += cluster[i] == i; }
  if (nclusters) *nclusters = n;
  return P7X_OK;
}

} // namespace p7x

using namespace p7x;

extern "C" {

int p7x_msa_pair_idents(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, int device, uint32_t *idents, uint32_t *len)
{
  if (!idents) { set_error("p7x_msa_pair_idents: bad arguments"); return P7X_EINVAL; }
  PairEngine e;
  int rc = pair_images(abc_type, ax, N, L, kPairMaxIdentRows, "pairwise identity counts", e.img);
  if (rc != P7X_OK) return rc;
  if ((rc = e.open(device, 2.0)) != P7X_OK) return rc;
  PairJob j; j.na = N; j.nb = N; j.lower = true; j.idents = idents;
  if ((rc = e.run(j)) != P7X_OK) return rc;
  for (int64_t i = 0; i < N; ++i)
    for (int64_t k = i + 1; k < N; ++k) idents[i * N + k] = idents[k * N + i];      // the count is symmetric
  if (len) std::memcpy(len, e.img.len.data(), (size_t) N * sizeof(uint32_t));
  return P7X_OK;
}

int p7x_msa_idfilter(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, const int64_t *order, double maxid, int device,
                     uint8_t *keep, int64_t *stats)
{
  if (!order || !keep) { set_error("p7x_msa_idfilter: bad arguments"); return P7X_EINVAL; }
  PairEngine e;
  int rc = pair_images(abc_type, ax, N, L, kPairMaxRows, "identity filter", e.img);
  if (rc != P7X_OK) return rc;
  if ((rc = e.open(device, maxid)) != P7X_OK) return rc;
  rc = idfilter(e, order, keep);
  e.report(stats);
  return rc;
}

int p7x_msa_linkage(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, double maxid, int device, int32_t *cluster,
                    int64_t *nclusters, int64_t *stats)
{
  if (!cluster) { set_error("p7x_msa_linkage: bad arguments"); return P7X_EINVAL; }
  PairEngine e;
  int rc = pair_images(abc_type, ax, N, L, kPairMaxLinkRows, "single-linkage clusters", e.img);
  if (rc != P7X_OK) return rc;
  if ((rc = e.open(device, maxid)) != P7X_OK) return rc;
  rc = linkage(e, cluster, nclusters);
  e.report(stats);
  return rc;
}

int p7x_debug_msa_pair_links(int32_t abc_type, const uint8_t *ax, int64_t N, int32_t L, double maxid, int device, const int32_t *rows_a,
                             int64_t na, const int32_t *rows_b, int64_t nb, uint64_t *bits, uint8_t *any)
{
  if (!rows_a || !rows_b || na < 1 || nb < 1 || (!bits && !any)) { set_error("p7x_debug_msa_pair_links: bad arguments"); return P7X_EINVAL; }
  PairEngine e;
  int rc = pair_images(abc_type, ax, N, L, kPairMaxRows, "link bits", e.img);
  if (rc != P7X_OK) return rc;
  for (int64_t i = 0; i < na; ++i) if (rows_a[i] < 0 || rows_a[i] >= N) { set_error("p7x_debug_msa_pair_links: a row index is out of range"); return P7X_EINVAL; }
  for (int64_t i = 0; i < nb; ++i) if (rows_b[i] < 0 || rows_b[i] >= N) { set_error("p7x_debug_msa_pair_links: a row index is out of range"); return P7X_EINVAL; }
  if ((rc = e.open(device, maxid)) != P7X_OK) return rc;
  PairJob j; j.rows_a = rows_a; j.na = na; j.rows_b = rows_b; j.nb = nb; j.bits = bits; j.any = any;
  return e.run(j);
}

} // extern "C"
