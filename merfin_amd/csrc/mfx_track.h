// mfx_track.h -- device code of -track, shared by the kernel files (mfx_kernels.hip: mfx_track_kernel, k <= 31;
// mfx_wide.hip: mfx_w_track_kernel, 32 <= k <= 64): K* of a k-mer (merfin-dump.C:44-67, through mfx_getK_core /
// mfx_kmetric) folded into the record of the fixed window its start position lies in (include/merfin_amd.h:
// mfx_track_window).  Include from .hip files only.
//
// Every field of a record is an integer sum, a minimum or a maximum, so a record does not depend on which lane,
// wave, block or launch saw a k-mer.  That holds for the sum of K* too -- it is exact:
//   - a finite non-zero K* is +-(q - 1) with q = hi / lo >= 1 a double (mfx_kmetric);
//   - q - 1 is then exact and a multiple of ulp(q) >= 2^-52: every K* is an integer number of 2^-52 units;
//   - its magnitude is below 2^32 (counts are uint32), so that integer fits in 84 bits;
//   - 2^32 of them (a window's k-mers are counted in a uint32) fit in the signed 128 bits of sum_kstar_hi:lo.
//
// The reduction.  In a round of a tile consecutive lanes hold consecutive positions, so the lanes of a wave lie in
// windows that do not decrease with the lane number, and a window's lanes are neighbours:
//   lane   : sums what it evaluates in registers for as long as its positions stay in one window (W >= 256: rounds);
//   wave   : when a lane's window changes, the wave reduces by segments (6 shuffle steps) -- one head lane per
//            (wave, window) holds the segment's share;
//   tile   : the heads add their shares to the tile's records in LDS (ds atomics without return: nothing waits for
//            them) when the tile touches at most MFX_TRK_LDS_WINDOWS windows (W >= ~65), and after the tile's last
//            round one lane per (tile, window) sends the record on;
//   global : commutative integer atomics -- packed pairs of the counters and the two sums as u64 adds, the 128-bit
//            sum as a low-word add whose carry (seen in the returned old value) goes into the high-word add, min and
//            max as u64 maxima of a monotone key.  A tile of more windows than the LDS table (small W: few lanes per
//            window, little to combine) sends its heads' shares straight there.
#pragma once
#include "mfx_device.h"
#include "mfx_kstar.h"

constexpr uint32_t MFX_TRK_LDS_WINDOWS = 64;
constexpr uint32_t MFX_TRK_LDS_WORDS = 10;      // c01, c23, c45, sum_readK, sum_asmK, three limbs of the K* sum, min, max

// the share of one window a lane (then: a segment's head lane) holds
struct mfx_trk_acc {
  uint64_t cnt;            // five 12-bit counters (a lane evaluates 16 k-mers of a tile, a wave 1024): k-mers | missing << 12 | non-finite << 24 | K* > 0 << 36 | K* < 0 << 48
  uint64_t sr, sa;         // sums of readK and asmK over the scored k-mers
  uint64_t lo, hi;         // sum of K* in units of 2^-52, two's complement
  uint64_t mn, mx;         // ~key of the smallest and key of the largest K* (mfx_trk_key); 0: none
};

__device__ __forceinline__ void mfx_trk_clear(mfx_trk_acc &A) { A.cnt = A.sr = A.sa = A.lo = A.hi = A.mn = A.mx = 0ull; }

// monotone double -> u64: x < y <=> key(x) < key(y) for finite x, y; never 0 and never ~0 for a finite x
__device__ __forceinline__ uint64_t mfx_trk_key(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double mfx_trk_unkey(uint64_t key) {
  const uint64_t b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  return __longlong_as_double((long long)b);
}

// one valid k-mer with its summed counts (merfin-dump.C:48-66); true: it is missing from the reads
__device__ __forceinline__ bool mfx_trk_add(mfx_trk_acc &A, double peak, uint32_t n_prob, const uint32_t *probK, const double *probP,
                                            uint32_t rv, uint32_t av) {
  double readK, prob;
  mfx_getK_core(peak, n_prob, probK, probP, rv, readK, prob);
  A.cnt += 1ull;                                              // kasm, :48
  if (readK == 0) { A.cnt += 1ull << 12; return true; }           // missing, :56-58 (K* is 0 by definition; not scored)
  if (av == 0) { A.cnt += 1ull << 24; return false; }             // readK / 0: not finite
  const double asmK = (double)av;                             // merfin-globals.C:81
  const double x = mfx_kmetric(readK, asmK);
  A.sr += (uint64_t)readK;                                    // (integer-valued: 1, round(), probK[])
  A.sa += (uint64_t)av;
  // |x| = ip + fr exactly, fr a multiple of 2^-52 below 1: the integer is ip << 52 | fr * 2^52
  const double ax = fabs(x);
  const uint64_t ip = (uint64_t)ax;
  const double fr = ax - (double)ip;
  const uint64_t ff = (uint64_t)(fr * 4503599627370496.0);
  uint64_t lo = (ip << 52) | ff, hi = ip >> 12;
  if (x < 0) { lo = ~lo + 1ull; hi = ~hi + (lo == 0ull ? 1ull : 0ull); A.cnt += 1ull << 48; }
  else if (x > 0) A.cnt += 1ull << 36;
  A.lo += lo;
  A.hi += hi + (A.lo < lo ? 1ull : 0ull);
  const uint64_t key = mfx_trk_key(x);
  A.mn = A.mn > ~key ? A.mn : ~key;
  A.mx = A.mx > key ? A.mx : key;
  return false;
}

__device__ __forceinline__ void mfx_trk_merge(mfx_trk_acc &A, const mfx_trk_acc &B) {
  A.cnt += B.cnt; A.sr += B.sr; A.sa += B.sa;
  A.lo += B.lo;
  A.hi += B.hi + (A.lo < B.lo ? 1ull : 0ull);
  A.mn = A.mn > B.mn ? A.mn : B.mn;
  A.mx = A.mx > B.mx ? A.mx : B.mx;
}

// Segmented reduction over the wave: `win` does not decrease with the lane number; afterwards the FIRST lane of every
// run of equal `win` holds the run's total (lane i holds the total of the lanes i .. end of its run).  Returns
// whether this lane is such a head.
__device__ __forceinline__ bool mfx_trk_wave_reduce(mfx_trk_acc &A, uint32_t win) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const uint32_t ow = (uint32_t)__shfl_down((int)win, off, 64);
    mfx_trk_acc B;
    B.cnt = __shfl_down(A.cnt, off, 64); B.sr = __shfl_down(A.sr, off, 64); B.sa = __shfl_down(A.sa, off, 64);
    B.lo = __shfl_down(A.lo, off, 64);   B.hi = __shfl_down(A.hi, off, 64);
    B.mn = __shfl_down(A.mn, off, 64);   B.mx = __shfl_down(A.mx, off, 64);
    if (lane + off < 64u && ow == win) mfx_trk_merge(A, B);
  }
  const uint32_t pw = (uint32_t)__shfl_up((int)win, 1, 64);
  return lane == 0u || pw != win;
}

// the counters of a share as the record's three packed words: n_kmers | n_missing << 32, n_scored | n_pos << 32, n_neg | n_nonfinite << 32
__device__ __forceinline__ void mfx_trk_counts(uint64_t cnt, uint64_t &c01, uint64_t &c23, uint64_t &c45) {
  const uint64_t nk = cnt & 0xfffull, nm = (cnt >> 12) & 0xfffull, nf = (cnt >> 24) & 0xfffull, np = (cnt >> 36) & 0xfffull, nn = (cnt >> 48) & 0xfffull;
  c01 = nk | (nm << 32);
  c23 = (nk - nm - nf) | (np << 32);             // scored: has a read count and a finite K*
  c45 = nn | (nf << 32);
}

// A share into its record of the device image (the 9 words of mfx_track_window; while the kernel runs word 7 holds the
// largest ~key and word 8 the largest key, 0 = none: mfx_track_finish_kernel turns them into min_kstar / max_kstar).
// The packed counter pairs cannot carry into each other: a window's totals are below 2^32 (mfx_track_run checks).
__device__ __forceinline__ void mfx_trk_emit_global(uint64_t *rec, uint64_t c01, uint64_t c23, uint64_t c45, uint64_t sr, uint64_t sa,
                                                    uint64_t lo, uint64_t hi, uint64_t mn, uint64_t mx) {
  unsigned long long *r = reinterpret_cast<unsigned long long *>(rec);
  (void)__hip_atomic_fetch_add(r + 0, (unsigned long long)c01, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (c23) (void)__hip_atomic_fetch_add(r + 1, (unsigned long long)c23, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (c45) (void)__hip_atomic_fetch_add(r + 2, (unsigned long long)c45, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (sr) (void)__hip_atomic_fetch_add(r + 3, (unsigned long long)sr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (sa) (void)__hip_atomic_fetch_add(r + 4, (unsigned long long)sa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (lo | hi) {
    // 128-bit add in two commutative halves: this add's carry out of the low word is known from the value it replaced
    uint64_t carry = 0;
    if (lo) {
      const uint64_t old = __hip_atomic_fetch_add(r + 5, (unsigned long long)lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      carry = old + lo < old ? 1ull : 0ull;
    }
    if (hi + carry) (void)__hip_atomic_fetch_add(r + 6, (unsigned long long)(hi + carry), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (mn) (void)__hip_atomic_fetch_max(r + 7, (unsigned long long)mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (mx) (void)__hip_atomic_fetch_max(r + 8, (unsigned long long)mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the records of the windows one tile touches, in LDS.  The K* sum is kept as three limbs (bits 0-31, 32-63, 64-127 of the
// two's complement value, each summed in 64 bits: at most 64 shares per window and tile) so that no add needs its result.
struct mfx_trk_lds {
  uint64_t w[MFX_TRK_LDS_WINDOWS][MFX_TRK_LDS_WORDS];
};

__device__ __forceinline__ void mfx_trk_lds_clear(mfx_trk_lds &T) {
  for (uint32_t i = threadIdx.x; i < MFX_TRK_LDS_WINDOWS * MFX_TRK_LDS_WORDS; i += MFX_BLOCK) (&T.w[0][0])[i] = 0ull;
}

__device__ __forceinline__ void mfx_trk_emit_lds(mfx_trk_lds &T, uint32_t win, const mfx_trk_acc &A) {
  uint64_t c01, c23, c45;
  mfx_trk_counts(A.cnt, c01, c23, c45);
  unsigned long long *r = reinterpret_cast<unsigned long long *>(T.w[win]);
  (void)__hip_atomic_fetch_add(r + 0, (unsigned long long)c01, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (c23) (void)__hip_atomic_fetch_add(r + 1, (unsigned long long)c23, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (c45) (void)__hip_atomic_fetch_add(r + 2, (unsigned long long)c45, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (A.sr) (void)__hip_atomic_fetch_add(r + 3, (unsigned long long)A.sr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (A.sa) (void)__hip_atomic_fetch_add(r + 4, (unsigned long long)A.sa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (A.lo | A.hi) {
    (void)__hip_atomic_fetch_add(r + 5, (unsigned long long)(A.lo & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    (void)__hip_atomic_fetch_add(r + 6, (unsigned long long)(A.lo >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    (void)__hip_atomic_fetch_add(r + 7, (unsigned long long)A.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  if (A.mn) (void)__hip_atomic_fetch_max(r + 8, (unsigned long long)A.mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (A.mx) (void)__hip_atomic_fetch_max(r + 9, (unsigned long long)A.mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// What a tile needs to know about its windows (block-uniform), and the per-lane state of the reduction.
struct mfx_trk_tile {
  uint64_t *rec0;          // the record of the tile's first window
  uint64_t  window;
  uint32_t  rem0;          // offset of the tile's first position inside that window (window < 2^31; else unused)
  uint64_t  rem0_64;
  bool      use_lds;
};

// contig `c`'s tile at position pos0 with n positions; first_rec: the contig's first record
__device__ __forceinline__ mfx_trk_tile mfx_trk_tile_begin(uint64_t *recs, uint64_t first_rec, uint64_t window, uint64_t pos0, uint32_t n) {
  mfx_trk_tile t;
  const uint64_t w0 = pos0 / window, rem = pos0 - w0 * window;
  t.rec0 = recs + (first_rec + w0) * 9ull;
  t.window = window;
  t.rem0_64 = rem;
  t.rem0 = (uint32_t)rem;
  const uint64_t nwin = n ? (rem + n - 1ull) / window + 1ull : 0ull;
  t.use_lds = nwin <= MFX_TRK_LDS_WINDOWS;
  return t;
}

// window of the tile's position p, counted from the tile's first window
__device__ __forceinline__ uint32_t mfx_trk_window_of(const mfx_trk_tile &t, uint32_t p) {
  if (t.window >= (1ull << 31)) return t.rem0_64 + p >= t.window ? 1u : 0u;
  return (t.rem0 + p) / (uint32_t)t.window;
}

// The wave sends what its lanes hold for their windows `win` (wave-wide call; lanes holding nothing take part with empty shares)
__device__ __forceinline__ void mfx_trk_flush(const mfx_trk_tile &t, mfx_trk_lds &T, mfx_trk_acc &A, uint32_t win) {
  const bool head = mfx_trk_wave_reduce(A, win);
  if (head && (A.cnt & 0xfffull)) {
    if (t.use_lds) mfx_trk_emit_lds(T, win, A);
    else {
      uint64_t c01, c23, c45;
      mfx_trk_counts(A.cnt, c01, c23, c45);
      mfx_trk_emit_global(t.rec0 + 9ull * win, c01, c23, c45, A.sr, A.sa, A.lo, A.hi, A.mn, A.mx);
    }
  }
  mfx_trk_clear(A);
}

// One position of a round: the lane's window may have changed (its position moved on by MFX_BLOCK); a lane that holds
// a share of another window makes the whole wave flush first.  After the call every lane's `cur` is the window of the
// position it just visited -- non-decreasing with the lane number, which is what mfx_trk_wave_reduce needs.  True: a
// valid k-mer that is missing from the reads.
__device__ __forceinline__ bool mfx_trk_visit(const mfx_trk_tile &t, mfx_trk_lds &T, mfx_trk_acc &A, uint32_t &cur, uint32_t p, bool ok,
                                              double peak, uint32_t n_prob, const uint32_t *probK, const double *probP, uint32_t rv, uint32_t av) {
  const uint32_t win = mfx_trk_window_of(t, p);
  if (__any(A.cnt != 0ull && win != cur)) mfx_trk_flush(t, T, A, cur);
  cur = win;
  return ok && mfx_trk_add(A, peak, n_prob, probK, probP, rv, av);
}

// after the tile's last round, behind a barrier: one lane per window of the tile sends the LDS record on and clears it
__device__ __forceinline__ void mfx_trk_tile_end(const mfx_trk_tile &t, mfx_trk_lds &T) {
  if (!t.use_lds || threadIdx.x >= MFX_TRK_LDS_WINDOWS) return;
  uint64_t *w = T.w[threadIdx.x];
  if (w[0] == 0ull) return;                                   // no k-mer of this tile in that window: nothing was added
  const uint64_t l0 = w[5], l1 = w[6], l2 = w[7];
  // limbs -> 128 bits: l0 + (l1 << 32) + (l2 << 64), modulo 2^128
  const uint64_t a = l1 << 32, lo = l0 + a;
  const uint64_t hi = l2 + (l1 >> 32) + (lo < a ? 1ull : 0ull);
  mfx_trk_emit_global(t.rec0 + 9ull * threadIdx.x, w[0], w[1], w[2], w[3], w[4], lo, hi, w[8], w[9]);
#pragma unroll
  for (uint32_t i = 0; i < MFX_TRK_LDS_WORDS; ++i) w[i] = 0ull;
}
