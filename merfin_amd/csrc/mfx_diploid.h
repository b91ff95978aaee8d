// mfx_diploid.h -- the rule of mfx_db_diploid (mfx_db_join.cpp; kernels: mfx_diploid.hip): two haplotype assemblies against the reads in one sorted
// join.  Which class a k-mer of the union of the three databases belongs to, what it adds to the two images, to the counters and to the
// completeness piece sums.  Written once for the host and the device (MFX_MERGE_HD), no HIP call, no library state: the kernels,
// mfx_db_diploid_host and tools/native/diploid_sanitize.cpp run this text.
//
// For a k-mer of the union: r its raw read count (0: absent), rf = r where minV <= r <= maxV and else 0, c1 / c2 its counts in hap1 / hap2,
// cb = min(c1 + c2, 2^32 - 1) -- the count mfx_db_merge writes with MFX_MERGE_SUM.
//   class image   4 rows of max_mult + 1 cells, column min(rf, max_mult): row 0 read-only (c1 == c2 == 0), 1 hap1-only, 2 hap2-only, 3 shared;
//                 rf == 0 and cb == 0: no entry
//   cn image      what mfx_db_join_spectrum(reads, M) gives for M = mfx_db_merge([hap1, hap2], SUM): row min(cb, copies + 1), the same column
//   counters      per X in hap1, hap2, both (cX = c1, c2, cb): distinct (cX > 0), total (the sum of cX), only_distinct / only_total (cX > 0
//                 and r == 0 -- the RAW count: -min / -max do not apply), found (cX > 0 and rf > 0); solid (rf > 0), n_read (r > 0),
//                 n_shared (c1 > 0 and c2 > 0)
//   piece sums    mfx_join_completeness' (mfx_join.hip; merfin-completeness.C:70-117) for hap1, hap2 and M: the total is the same for the
//                 three (it sums readK over the read k-mers), so one tot[64] and three und[64]
// QV per X is mfx_histoQV (merfin-histogram.C:22-31) with kval = only_total and ktot = total.  This follows Merqury's QV and k-mer
// completeness in spirit; it is UNVALIDATED against Merqury.  Both the distinct and the total counts are kept, so that a reader can apply
// the other convention.
//
// HOW THE TWO ASSEMBLIES BECOME ONE RUN.  The k-mers of hap1 and hap2 take their role into the key's two low bits (mfx_trio_tag, roles 0 and 1),
// mfx_merge_pairs_kernel merges the tagged runs as it is, and every head position of the merged run (mfx_trio_head) becomes one record of the
// PAIR RUN: the k-mer without its tag, and both counts in one 64-bit word (mfx_dip_pack).  The read run is then joined against the pair run by
// mfx_join_kernel's walk (mfx_join.h) with a 64-bit asm value; it is read once and never rewritten.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mfx_join.h"
#include "mfx_trio.h"                                          // mfx_trio_tag / _kmer / _role / _head

constexpr uint32_t MFX_DIP_HAP1 = 0, MFX_DIP_HAP2 = 1;         // the roles of the two assemblies in a tagged key
constexpr uint32_t MFX_DIP_ROWS = 4;                           // the class image: read-only, hap1-only, hap2-only, shared
constexpr uint32_t MFX_DIP_READ_ONLY = 0, MFX_DIP_HAP1_ONLY = 1, MFX_DIP_HAP2_ONLY = 2, MFX_DIP_SHARED = 3;

// the counters: five per X (X * MFX_DIP_PER_X + ...), then three of the call
enum { MFX_DIP_DISTINCT, MFX_DIP_TOTAL, MFX_DIP_ONLY_DISTINCT, MFX_DIP_ONLY_TOTAL, MFX_DIP_FOUND, MFX_DIP_PER_X };
constexpr uint32_t MFX_DIP_SOLID = 3 * MFX_DIP_PER_X, MFX_DIP_N_READ = MFX_DIP_SOLID + 1, MFX_DIP_N_SHARED = MFX_DIP_SOLID + 2, MFX_DIP_NSTATS = MFX_DIP_SOLID + 3;
// The join kernel's counters on the device: MFX_DIP_STAT_SHARDS copies of two 128-byte lines each, a workgroup adding to copy
// blockIdx % SHARDS, the host adding the copies up (as MFX_TRIO_STAT_SHARDS, mfx_trio.h).
constexpr uint32_t MFX_DIP_STAT_SHARDS = 64, MFX_DIP_STAT_STRIDE = 32, MFX_DIP_STAT_WORDS = MFX_DIP_STAT_SHARDS * MFX_DIP_STAT_STRIDE;
static_assert(MFX_DIP_NSTATS <= MFX_DIP_STAT_STRIDE, "a shard holds every counter");

// Both images are counted in one array of 32-bit LDS bins (mfx_spectrum.h's, twice: the class image's 4 rows in front of the cn image's
// copies + 2): columns m < L of every row in LDS, the others straight in the image.  L is a power of two, 1024 for up to 8 rows and 512 for
// up to 12, and never more than a row has columns.
constexpr uint32_t MFX_DIP_LDS_WORDS = 8192;
inline uint32_t mfx_dip_lds_cols(uint32_t copies, uint32_t max_mult) {
  uint32_t L = 2048;
  while ((MFX_DIP_ROWS + copies + 2u) * L > MFX_DIP_LDS_WORDS) L >>= 1;
  return L < max_mult + 1u ? L : max_mult + 1u;
}

MFX_MERGE_HD uint64_t mfx_dip_pack(uint32_t c1, uint32_t c2) { return (uint64_t)c1 | ((uint64_t)c2 << 32); }

// The pair-run record of the head position i of the tagged merged run of hap1 and hap2 (n records): at most two records hold the k-mer.
MFX_MERGE_HD uint64_t mfx_dip_gather(const uint64_t *keys, const uint32_t *vals, uint64_t n, uint64_t i) {
  uint32_t c[2] = {0u, 0u};
  const uint64_t kmer = mfx_trio_kmer(keys[i]);
  for (uint64_t j = i; j < n && j < i + 2 && mfx_trio_kmer(keys[j]) == kmer; ++j) {
    const uint32_t role = mfx_trio_role(keys[j]);
    if (role < 2u) c[role] = vals[j];
  }
  return mfx_dip_pack(c[0], c[1]);
}

struct mfx_dip_class {
  uint32_t rf, c1, c2, cb;
  uint32_t row;                                                // of the class image
  bool entry;                                                  // of both images: rf != 0 or cb != 0
};

// r: the raw read count; packed: the pair-run word, 0 where neither assembly holds the k-mer
MFX_MERGE_HD mfx_dip_class mfx_dip_rule(uint32_t r, uint64_t packed, uint64_t minV, uint64_t maxV) {
  mfx_dip_class k;
  k.rf = ((uint64_t)r < minV || (uint64_t)r > maxV) ? 0u : r;  // -min / -max (merfin.C:199-200)
  k.c1 = (uint32_t)packed;
  k.c2 = (uint32_t)(packed >> 32);
  const uint64_t sum = (uint64_t)k.c1 + (uint64_t)k.c2;
  k.cb = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
  k.row = k.c1 ? (k.c2 ? MFX_DIP_SHARED : MFX_DIP_HAP1_ONLY) : (k.c2 ? MFX_DIP_HAP2_ONLY : MFX_DIP_READ_ONLY);
  k.entry = (k.rf | k.cb) != 0u;
  return k;
}

// one k-mer into the counters
MFX_MERGE_HD void mfx_dip_count(uint64_t st[MFX_DIP_NSTATS], uint32_t r, const mfx_dip_class &k) {
  const uint32_t cx[3] = {k.c1, k.c2, k.cb};
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t x = 0; x < 3u; ++x) {
    const bool in = cx[x] != 0u, only = in && r == 0u;
    uint64_t *s = st + x * MFX_DIP_PER_X;
    s[MFX_DIP_DISTINCT] += in ? 1u : 0u;
    s[MFX_DIP_TOTAL] += cx[x];
    s[MFX_DIP_ONLY_DISTINCT] += only ? 1u : 0u;
    s[MFX_DIP_ONLY_TOTAL] += only ? cx[x] : 0u;
    s[MFX_DIP_FOUND] += (in && k.rf != 0u) ? 1u : 0u;
  }
  st[MFX_DIP_SOLID] += k.rf != 0u ? 1u : 0u;
  st[MFX_DIP_N_READ] += r != 0u ? 1u : 0u;
  st[MFX_DIP_N_SHARED] += (k.c1 != 0u && k.c2 != 0u) ? 1u : 0u;
}

// the piece of a k-mer (the top 6 bits of its 2k bits) and what it leaves of readK over an assembly count
MFX_MERGE_HD int mfx_dip_pshift(int k) { return 2 * k >= 6 ? 2 * k - 6 : 0; }
MFX_MERGE_HD double mfx_dip_under(double readK, uint32_t c) {
  const double asmK = (double)c;
  return readK > asmK ? readK - asmK : 0.0;                    // merfin-completeness.C:115-116
}

// ---- the host's restatement of the device path: tag, merge, head compaction, the tiled lane walk, the rule
struct mfx_dip_host_result {
  std::vector<uint64_t> pk, pv;                                // the pair run
  std::vector<uint64_t> asm_img, cn_img;                       // 4 and copies + 2 rows of max_mult + 1 cells
  uint64_t n_entries = 0;
  uint64_t stats[MFX_DIP_NSTATS];
  double tot[64], und[3][64];
};

// the pair run of two strictly ascending runs: the tagged keys merged with hap1's record in front, then every head position
inline void mfx_dip_pair_run_host(const uint64_t *k1, const uint32_t *v1, uint64_t n1, const uint64_t *k2, const uint32_t *v2, uint64_t n2, std::vector<uint64_t> &pk,
                                  std::vector<uint64_t> &pv) {
  const uint64_t total = n1 + n2;
  std::vector<uint64_t> mk(total);
  std::vector<uint32_t> mv(total);
  uint64_t i = 0, j = 0;
  for (uint64_t o = 0; o < total; ++o) {                       // (tagged keys never tie)
    const bool a = i < n1 && (j >= n2 || mfx_trio_tag(k1[i], MFX_DIP_HAP1) < mfx_trio_tag(k2[j], MFX_DIP_HAP2));
    mk[o] = a ? mfx_trio_tag(k1[i], MFX_DIP_HAP1) : mfx_trio_tag(k2[j], MFX_DIP_HAP2);
    mv[o] = a ? v1[i++] : v2[j++];
  }
  pk.clear(); pv.clear();
  for (uint64_t p = 0; p < total; ++p) {
    if (!mfx_trio_head(mk.data(), p)) continue;
    pk.push_back(mfx_trio_kmer(mk[p]));
    pv.push_back(mfx_dip_gather(mk.data(), mv.data(), total, p));
  }
}

// readK(rv): a callable (the host has no LDS table to look it up in); null_peak: no piece sums.  each(key, r, c1, c2) per k-mer in walk order.
template <class ReadK, class Each>
inline void mfx_dip_host(const uint64_t *rk, const uint32_t *rv, uint64_t nr, const uint64_t *k1, const uint32_t *v1, uint64_t n1, const uint64_t *k2, const uint32_t *v2,
                         uint64_t n2, int k, uint64_t minV, uint64_t maxV, uint32_t copies, uint32_t max_mult, bool pieces, ReadK &&readK, Each &&each,
                         mfx_dip_host_result &R) {
  mfx_dip_pair_run_host(k1, v1, n1, k2, v2, n2, R.pk, R.pv);
  const uint64_t W = (uint64_t)max_mult + 1;
  R.asm_img.assign(MFX_DIP_ROWS * W, 0);
  R.cn_img.assign((uint64_t)(copies + 2u) * W, 0);
  R.n_entries = 0;
  for (uint32_t s = 0; s < MFX_DIP_NSTATS; ++s) R.stats[s] = 0;
  for (int p = 0; p < 64; ++p) { R.tot[p] = 0.0; R.und[0][p] = R.und[1][p] = R.und[2][p] = 0.0; }
  const int pshift = mfx_dip_pshift(k);
  mfx_join_host<uint64_t>(rk, rv, nr, R.pk.data(), R.pv.data(), R.pk.size(), [&](bool have, uint64_t key, uint32_t r, uint64_t packed) {
    if (!have) return;
    const mfx_dip_class c = mfx_dip_rule(r, packed, minV, maxV);
    each(key, r, c.c1, c.c2);
    mfx_dip_count(R.stats, r, c);
    if (c.entry) {
      const uint64_t col = c.rf < max_mult ? c.rf : max_mult;
      ++R.asm_img[c.row * W + col];
      ++R.cn_img[(uint64_t)(c.cb <= copies ? c.cb : copies + 1u) * W + col];
      ++R.n_entries;
    }
    if (pieces && r != 0u) {
      const double K = readK(r);
      const uint32_t piece = (uint32_t)(key >> pshift) & 63u;
      R.tot[piece] += K;
      R.und[0][piece] += mfx_dip_under(K, c.c1);
      R.und[1][piece] += mfx_dip_under(K, c.c2);
      R.und[2][piece] += mfx_dip_under(K, c.cb);
    }
  });
}
