// mfx_merge.h -- the plain host arithmetic of mfx_db_merge (mfx_db_merge.cpp): the key windows the sorted inputs are merged by, and the slice of
// an input's escape list that belongs to a window.  No HIP, no library state: tools/native/db_merge_sanitize.cpp drives it under the
// sanitizers, tests/test_merge_plan_cpu.py through mfx_db_merge_plan.
//
// An input is a delta-coded flat database (mfx_db.cpp FLAT_DELTA): blocks of MFX_DELTA_BLOCK ascending k-mers whose first k-mers stand in the
// file's directory.  Block b of an input holds k-mers in [first[b], first[b + 1]) -- the last one up to the end of the key space -- and that
// is all the host knows of it.  The key space [0, 2^2k) is cut into half-open windows [lo, hi); per window and input the blocks that MAY
// hold a k-mer of the window are decoded, and what they hold outside the window is dropped, so every copy of a key lands in one window.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

constexpr uint64_t MFX_MERGE_BLOCK = 4096;                     // (MFX_DELTA_BLOCK, mfx_delta.h: checked where both are seen, mfx_db_windows.cpp)
constexpr uint64_t MFX_MERGE_RANGE_DEFAULT = 1ull << 26;       // pairs decoded per window, summed over the inputs
constexpr uint32_t MFX_MERGE_MAX_INPUTS = 64;

// first[b * stride]: the first k-mer of block b (stride 2: a file's directory as it is read), strictly ascending; n k-mers in
// nblocks = ceil(n / 4096) blocks
struct mfx_merge_input { const uint64_t *first; uint32_t stride; uint64_t nblocks, n; };
struct mfx_merge_window { uint64_t lo, hi, pairs; };            // pairs: what the window's blocks hold, summed over the inputs

#if defined(__HIPCC__)
#define MFX_MERGE_HD __host__ __device__ inline __attribute__((always_inline))      // (no HIP header needed)
#else
#define MFX_MERGE_HD inline
#endif

// merge path: how many of the first d pairs of two ascending runs merged come from a (la of them) -- with equal k-mers a's first.  The merge
// kernel and the join kernel (mfx_merge.hip, mfx_join.hip) cut their tiles and their lanes' shares with it, mfx_join.h restates both on the host.
template <class I>
MFX_MERGE_HD I mfx_merge_cut(const uint64_t *a, I la, const uint64_t *b, I lb, I d) {
  I x = d > lb ? d - lb : 0, y = d < la ? d : la;
  while (x < y) {
    const I m = x + (y - x) / 2;
    if (a[m] <= b[d - 1 - m]) x = m + 1; else y = m;
  }
  return x;
}

inline uint64_t mfx_merge_end(int k) { return 1ull << (2 * k); }      // k <= 31: one past the largest k-mer

// the blocks [b0, b1) of an input that may hold a k-mer of [lo, hi): from the last block that starts at or below lo (its k-mers reach up to
// the next block's first) to the last block that starts below hi
inline void mfx_merge_blocks(const mfx_merge_input &in, uint64_t lo, uint64_t hi, uint64_t *b0, uint64_t *b1) {
  uint64_t a = 0, b = in.nblocks;                              // the first block that starts above lo
  while (a < b) { const uint64_t m = a + (b - a) / 2; if (in.first[m * in.stride] <= lo) a = m + 1; else b = m; }
  const uint64_t begin = a ? a - 1 : 0;
  a = begin; b = in.nblocks;                                   // the first block that starts at or above hi
  while (a < b) { const uint64_t m = a + (b - a) / 2; if (in.first[m * in.stride] < hi) a = m + 1; else b = m; }
  *b0 = begin;
  *b1 = a > begin ? a : begin;
}
inline uint64_t mfx_merge_block_pairs(const mfx_merge_input &in, uint64_t b0, uint64_t b1) {
  if (b1 <= b0) return 0;
  return std::min(in.n, b1 * MFX_MERGE_BLOCK) - b0 * MFX_MERGE_BLOCK;
}
inline uint64_t mfx_merge_cost(const mfx_merge_input *in, uint32_t n_in, uint64_t lo, uint64_t hi) {
  uint64_t sum = 0;
  for (uint32_t i = 0; i < n_in; ++i) {
    uint64_t b0, b1;
    mfx_merge_blocks(in[i], lo, hi, &b0, &b1);
    sum += mfx_merge_block_pairs(in[i], b0, b1);
  }
  return sum;
}

// The windows: ascending, half-open, together [0, 2^2k).  Every boundary but the two ends is the first k-mer of a block of some input.  A window
// takes the largest such boundary that keeps its blocks at R pairs or below; where even the next boundary does not, it takes that one -- no
// block starts inside such a window, so it holds one block per input at the most.  blk[2 * (w * n_in + i)], [.. + 1]: the blocks [b0, b1) of
// input i in window w.
inline void mfx_merge_plan(const mfx_merge_input *in, uint32_t n_in, int k, uint64_t R, std::vector<mfx_merge_window> &win, std::vector<uint64_t> &blk) {
  win.clear();
  blk.clear();
  if (R == 0) R = 1;
  const uint64_t END = mfx_merge_end(k);
  std::vector<uint64_t> cand;                                  // the candidate boundaries: every block's first k-mer, once
  for (uint32_t i = 0; i < n_in; ++i)
    for (uint64_t b = 0; b < in[i].nblocks; ++b) cand.push_back(in[i].first[b * in[i].stride]);
  std::sort(cand.begin(), cand.end());
  cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
  uint64_t lo = 0;
  size_t ci = 0;
  while (true) {
    while (ci < cand.size() && cand[ci] <= lo) ++ci;
    uint64_t hi = END;
    if (ci < cand.size() && mfx_merge_cost(in, n_in, lo, END) > R) {
      size_t a = ci, b = cand.size();                          // the first candidate whose window is above R (the cost grows with hi)
      while (a < b) { const size_t m = a + (b - a) / 2; if (mfx_merge_cost(in, n_in, lo, cand[m]) <= R) a = m + 1; else b = m; }
      const size_t j = a > ci ? a - 1 : ci;
      hi = cand[j];
      ci = j + 1;
    }
    mfx_merge_window w{lo, hi, 0};
    for (uint32_t i = 0; i < n_in; ++i) {
      uint64_t b0, b1;
      mfx_merge_blocks(in[i], lo, hi, &b0, &b1);
      blk.push_back(b0);
      blk.push_back(b1);
      w.pairs += mfx_merge_block_pairs(in[i], b0, b1);
    }
    win.push_back(w);
    if (hi == END) break;
    lo = hi;
  }
}

// the escapes [e0, e1) of an ascending escape list whose k-mers lie in [lo, hi)
inline void mfx_merge_escape_slice(const uint64_t *ek, uint64_t n, uint64_t lo, uint64_t hi, uint64_t *e0, uint64_t *e1) {
  *e0 = (uint64_t)(std::lower_bound(ek, ek + n, lo) - ek);
  *e1 = (uint64_t)(std::lower_bound(ek + *e0, ek + n, hi) - ek);
}
