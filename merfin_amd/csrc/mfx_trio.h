// mfx_trio.h -- the class rule of mfx_db_trio (mfx_db_trio.cpp; kernels: mfx_trio.hip): which hap-mer set a k-mer of the parents' and the child's
// databases belongs to, the count written for it, and what it adds to the three histogram rows.  Written once for the host and the device
// (MFX_MERGE_HD), no HIP call, no library state: the kernels, mfx_db_trio_host and tools/native/trio_sanitize.cpp run this text.
//
// The rule is this project's own, in the spirit of Merqury's hapmers.sh (parent-specific k-mers above an error cutoff, kept where the child
// holds them); it is UNVALIDATED against Merqury.
//
// HOW THE ROLE TRAVELS.  mfx_db_merge's kernels merge (k-mer, count) records and keep no word of which input a record came from.  A k-mer of
// k <= 31 takes 2k <= 62 bits, so every record's key is shifted up by two bits and the input's role stands in the two bits below it
// (mfx_trio_tag): the tagged keys of one input still ascend strictly, keys of different inputs are never equal, and the merged run has the
// at most three records of one k-mer side by side in the order mat, pat, child.  At k = 31 the tagged key uses all 64 bits.
#pragma once
#include <stdint.h>

#include <vector>

#include "mfx_merge.h"                                         // MFX_MERGE_HD

constexpr uint32_t MFX_TRIO_MAT = 0, MFX_TRIO_PAT = 1, MFX_TRIO_CHILD = 2;      // the roles, and the histogram rows of their k-mers
constexpr uint32_t MFX_TRIO_NONE = 0, MFX_TRIO_A = 1, MFX_TRIO_B = 2;           // the set a k-mer goes to
constexpr uint32_t MFX_TRIO_NOROW = 3;                         // mfx_trio_class::prow: the k-mer adds to neither parent's row

MFX_MERGE_HD uint64_t mfx_trio_tag(uint64_t kmer, uint32_t role) { return (kmer << 2) | (uint64_t)role; }
MFX_MERGE_HD uint64_t mfx_trio_kmer(uint64_t tagged) { return tagged >> 2; }
MFX_MERGE_HD uint32_t mfx_trio_role(uint64_t tagged) { return (uint32_t)(tagged & 3u); }

struct mfx_trio_cuts { uint32_t tm, tp, tc; bool has_child; };      // the cutoffs, each >= 1 (tc is not read without a child)

struct mfx_trio_class {
  uint32_t set;                                                // MFX_TRIO_NONE / _A / _B
  uint32_t count;                                              // the count written: min(parent, child) with a child, the parent's without
  uint32_t prow;                                               // MFX_TRIO_MAT: cp == 0, binned by cm; MFX_TRIO_PAT: cm == 0, by cp; else MFX_TRIO_NOROW
  bool both, mat_only, pat_only;                               // held by both parents / by one of them alone
  bool mat_cut, pat_cut;                                       // ... alone, and at or above its cutoff
  bool child_cut;                                              // the child holds it at or above tc
};

// cm, cp, cc: the k-mer's counts in the three databases, 0 where absent (not all three 0)
MFX_MERGE_HD mfx_trio_class mfx_trio_rule(uint32_t cm, uint32_t cp, uint32_t cc, const mfx_trio_cuts &t) {
  mfx_trio_class r;
  r.both = cm != 0u && cp != 0u;
  r.mat_only = cm != 0u && cp == 0u;
  r.pat_only = cp != 0u && cm == 0u;
  r.mat_cut = r.mat_only && cm >= t.tm;
  r.pat_cut = r.pat_only && cp >= t.tp;
  r.child_cut = t.has_child && cc != 0u && cc >= t.tc;
  r.prow = r.mat_only ? MFX_TRIO_MAT : r.pat_only ? MFX_TRIO_PAT : MFX_TRIO_NOROW;
  const bool child_ok = !t.has_child || r.child_cut;
  r.set = (r.mat_cut && child_ok) ? MFX_TRIO_A : (r.pat_cut && child_ok) ? MFX_TRIO_B : MFX_TRIO_NONE;
  const uint32_t pc = r.set == MFX_TRIO_A ? cm : cp;
  r.count = r.set == MFX_TRIO_NONE ? 0u : (t.has_child && cc < pc) ? cc : pc;
  return r;
}

// Is position i of the tagged merged run the first record of its k-mer?
MFX_MERGE_HD bool mfx_trio_head(const uint64_t *keys, uint64_t i) { return i == 0 || mfx_trio_kmer(keys[i - 1]) != mfx_trio_kmer(keys[i]); }

// The counts of the k-mer whose first record stands at the head position i: c[role], 0 where the role holds no record.  At most three records.
MFX_MERGE_HD void mfx_trio_gather(const uint64_t *keys, const uint32_t *vals, uint64_t n, uint64_t i, uint32_t c[3]) {
  const uint64_t kmer = mfx_trio_kmer(keys[i]);
  c[0] = c[1] = c[2] = 0u;
  for (uint64_t j = i; j < n && j < i + 3 && mfx_trio_kmer(keys[j]) == kmer; ++j) {
    const uint32_t role = mfx_trio_role(keys[j]);
    if (role < 3u) c[role] = vals[j];
  }
}

// the column of a count in a histogram row of max_mult + 1 cells
MFX_MERGE_HD uint32_t mfx_trio_col(uint32_t count, uint32_t max_mult) { return count < max_mult ? count : max_mult; }

// what mfx_db_trio counts, summed over the k-mers (the order of mfx_db_trio_stats' counters behind n_child: include/merfin_amd.h)
enum { MFX_TRIO_S_BOTH, MFX_TRIO_S_MAT_ONLY, MFX_TRIO_S_PAT_ONLY, MFX_TRIO_S_MAT_CUT, MFX_TRIO_S_PAT_CUT, MFX_TRIO_S_CHILD_CUT, MFX_TRIO_NSTATS };
// The classify kernel's counters on the device: MFX_TRIO_STAT_SHARDS copies, one 128-byte line each, a workgroup adding to copy blockIdx % SHARDS;
// the host adds the copies up.  (Nearly every workgroup has something to add to nearly every counter: adds to one line from every wave of
// every tile took 0.39 s of a 1.5 s call at 2.9 G records, profiles/trio_rate.txt.)
constexpr uint32_t MFX_TRIO_STAT_SHARDS = 64, MFX_TRIO_STAT_STRIDE = 16, MFX_TRIO_STAT_WORDS = MFX_TRIO_STAT_SHARDS * MFX_TRIO_STAT_STRIDE;

struct mfx_trio_host_result {
  std::vector<uint64_t> ak, bk;                                // the two sets, ascending
  std::vector<uint32_t> av, bv;
  std::vector<uint64_t> img;                                   // 3 rows of max_mult + 1 cells
  uint64_t stats[MFX_TRIO_NSTATS] = {0, 0, 0, 0, 0, 0};
};

// The whole of mfx_db_trio on the host over three strictly ascending runs (role i: keys[i], vals[i], n[i]; the child's n is 0 without one):
// tag, merge with the earlier role in front, then every head position through mfx_trio_gather and mfx_trio_rule, as the kernels do.
inline void mfx_trio_host(const uint64_t *const keys[3], const uint32_t *const vals[3], const uint64_t n[3], const mfx_trio_cuts &t, uint32_t max_mult,
                          mfx_trio_host_result &R) {
  const uint64_t total = n[0] + n[1] + n[2];
  std::vector<uint64_t> mk(total);
  std::vector<uint32_t> mv(total);
  uint64_t at[3] = {0, 0, 0};
  for (uint64_t o = 0; o < total; ++o) {                       // (tagged keys never tie: the smallest of the three fronts)
    int best = -1;
    uint64_t bt = 0;
    for (int r = 0; r < 3; ++r) {
      if (at[r] >= n[r]) continue;
      const uint64_t x = mfx_trio_tag(keys[r][at[r]], (uint32_t)r);
      if (best < 0 || x < bt) { best = r; bt = x; }
    }
    mk[o] = bt;
    mv[o] = vals[best][at[best]++];
  }
  const uint64_t W = (uint64_t)max_mult + 1;
  R.img.assign(3 * W, 0);
  for (uint64_t i = 0; i < total; ++i) {
    if (!mfx_trio_head(mk.data(), i)) continue;
    uint32_t c[3];
    mfx_trio_gather(mk.data(), mv.data(), total, i, c);
    const mfx_trio_class r = mfx_trio_rule(c[0], c[1], c[2], t);
    if (r.prow != MFX_TRIO_NOROW) ++R.img[r.prow * W + mfx_trio_col(c[r.prow], max_mult)];
    if (c[2]) ++R.img[MFX_TRIO_CHILD * W + mfx_trio_col(c[2], max_mult)];
    R.stats[MFX_TRIO_S_BOTH] += r.both; R.stats[MFX_TRIO_S_MAT_ONLY] += r.mat_only; R.stats[MFX_TRIO_S_PAT_ONLY] += r.pat_only;
    R.stats[MFX_TRIO_S_MAT_CUT] += r.mat_cut; R.stats[MFX_TRIO_S_PAT_CUT] += r.pat_cut; R.stats[MFX_TRIO_S_CHILD_CUT] += r.child_cut;
    if (r.set == MFX_TRIO_A) { R.ak.push_back(mfx_trio_kmer(mk[i])); R.av.push_back(r.count); }
    else if (r.set == MFX_TRIO_B) { R.bk.push_back(mfx_trio_kmer(mk[i])); R.bv.push_back(r.count); }
  }
}
