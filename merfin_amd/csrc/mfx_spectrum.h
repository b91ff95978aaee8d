// mfx_spectrum.h -- the copy-number spectrum of an index: the 2-D histogram of the (read count, assembly count) pairs of
// its entries (what assembly evaluators call spectra-cn).  No reference counterpart: merfin takes its -peak from a k-mer
// histogram of the read database made elsewhere.  Shared by the two streaming kernels (mfx_spectrum_kernel in
// mfx_kernels.hip, mfx_w_spectrum_kernel in mfx_wide.hip) and the host side (mfx_spectrum.cpp).
#pragma once
#include "mfx_internal.h"

// Image: (copies + 2) rows of max_mult + 1 uint64 cells, row-major; one more word behind it counts the entries the
// kernels counted (mfx_spectrum_run checks it against the sum of the cells).
//   row r <= copies: assembly count r; row copies + 1: assembly count > copies
//   column m < max_mult: read count m (after -min / -max); column max_mult: read count >= max_mult
constexpr uint32_t MFX_SPEC_MIN_COPIES = 1, MFX_SPEC_MAX_COPIES = 6;
constexpr uint32_t MFX_SPEC_MIN_MULT = 4, MFX_SPEC_MAX_MULT = 65536;
// Columns m < L of every row are counted in uint32 bins in LDS (rows * L * 4 <= 32 KB), the others straight in the image.
// L is a power of two between 1024 (7 or 8 rows) and 2048 (3 or 4 rows), and never more than the row has columns.
constexpr uint32_t MFX_SPEC_LDS_WORDS = 8192;
constexpr uint32_t MFX_SPEC_MAX_L = 2048;
// A block adds at most one to one bin per slot it reads, and the launchers give a block fewer than MFX_SPEC_BLOCK_SLOTS
// slots (they raise the grid until that holds): no LDS bin can wrap.
constexpr uint64_t MFX_SPEC_BLOCK_SLOTS = 1ull << 32;
#ifndef MFX_SPEC_AGG_DEFAULT
#define MFX_SPEC_AGG_DEFAULT 0       // the plain LDS atomics (mfx_spectrum_args::aggregate; MFX_SPECTRUM_AGG overrides per call)
#endif

static inline uint32_t mfx_spec_lds_cols(uint32_t copies, uint32_t max_mult) {
  uint32_t L = MFX_SPEC_MAX_L;
  while ((copies + 2u) * L > MFX_SPEC_LDS_WORDS) L >>= 1;
  return L < max_mult + 1u ? L : max_mult + 1u;
}

struct mfx_spectrum_args {
  mfx_table_view t;
  uint32_t       copies, max_mult;
  uint32_t       lds_cols;             // L (mfx_spec_lds_cols)
  int            aggregate;            // 1: lanes of a wave that hit the same LDS bin add once (A/B: docs/KNOBS.md, MFX_SPECTRUM_AGG)
  uint64_t      *img;                  // the image + the counter word, zero at launch
};

// grid: blocks the device holds at once (the kernels are persistent: grid-stride over the table); raised where a block's share
// of slots would reach MFX_SPEC_BLOCK_SLOTS
hipError_t mfx_k_spectrum(const mfx_spectrum_args &a, int grid, hipStream_t st);       // k <= 31, every layout
hipError_t mfx_kw_spectrum(const mfx_spectrum_args &a, int grid, hipStream_t st);      // 32 <= k <= 64 (mfx_wide.hip)

static inline unsigned mfx_spec_grid(uint64_t nslots, uint32_t per_lane, int grid) {
  const uint64_t per_block = (uint64_t)MFX_BLOCK * per_lane;
  uint64_t g = (nslots + per_block - 1) / per_block;
  if (g > (uint64_t)(grid > 0 ? grid : 1)) g = (uint64_t)(grid > 0 ? grid : 1);
  if (g < 1) g = 1;
  while ((nslots / g) + per_block >= MFX_SPEC_BLOCK_SLOTS) g *= 2;                      // a block's share of slots stays below 2^32
  return (unsigned)g;
}

#ifdef __HIPCC__
// One entry into the block's bins.  `have` lanes carry a pair; every lane of the wave must call (the aggregated form votes).
// Returns 1 when the entry was counted.
template <bool AGG>
__device__ __forceinline__ uint32_t mfx_spec_count(const mfx_spectrum_args &a, uint32_t *s_bins, bool have, uint32_t rv, uint32_t av) {
  have = have && (rv | av) != 0u;                              // both counts 0 after the filter: no entry of the spectrum
  const uint32_t row = av <= a.copies ? av : a.copies + 1u;
  const uint32_t col = rv < a.max_mult ? rv : a.max_mult;
  if (have && col >= a.lds_cols)
    atomicAdd(reinterpret_cast<unsigned long long *>(a.img) + (uint64_t)row * (a.max_mult + 1u) + col, 1ull);
  bool lds = have && col < a.lds_cols;
  const uint32_t bin = row * a.lds_cols + col;
  if (AGG) {
    // real spectra are skewed (half of a joint table is (0, 1)): same-address LDS atomics serialise inside a wave, so the
    // lanes sharing the first pending lane's bin add once, for two rounds; what is left takes the plain atomic
    unsigned long long todo = __ballot(lds);
#pragma unroll 1
    for (int r = 0; r < 2 && todo; ++r) {
      const int leader = __ffsll(todo) - 1;
      const uint32_t b0 = __shfl(bin, leader, 64);
      const bool same = lds && bin == b0;
      const unsigned long long m = __ballot(same);
      if ((int)(threadIdx.x & 63u) == leader) atomicAdd(&s_bins[b0], (uint32_t)__popcll(m));
      todo &= ~m;
      if (same) lds = false;
    }
  }
  if (lds) atomicAdd(&s_bins[bin], 1u);
  return have ? 1u : 0u;
}

__device__ __forceinline__ void mfx_spec_begin(const mfx_spectrum_args &a, uint32_t *s_bins) {
  for (uint32_t i = threadIdx.x; i < (a.copies + 2u) * a.lds_cols; i += blockDim.x) s_bins[i] = 0u;
  __syncthreads();
}

// the block's LDS bins and its entry count into the image (64-bit global atomics)
__device__ __forceinline__ void mfx_spec_end(const mfx_spectrum_args &a, uint32_t *s_bins, uint64_t counted) {
  __syncthreads();
  unsigned long long *img = reinterpret_cast<unsigned long long *>(a.img);
  const uint32_t W = a.max_mult + 1u;
  for (uint32_t i = threadIdx.x; i < (a.copies + 2u) * a.lds_cols; i += blockDim.x) {
    const uint32_t v = s_bins[i];
    if (v) atomicAdd(img + (uint64_t)(i / a.lds_cols) * W + (i % a.lds_cols), (unsigned long long)v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) counted += __shfl_down(counted, o, 64);
  if ((threadIdx.x & 63u) == 0 && counted) atomicAdd(img + (uint64_t)(a.copies + 2u) * W, (unsigned long long)counted);
}
#endif
