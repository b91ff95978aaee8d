// mfx_delta.h -- the block rule of the delta-coded flat database (mfx_db.cpp FLAT_DELTA), as arithmetic shared by host and device code.
//
// A block is at most MFX_DELTA_BLOCK strictly ascending k-mers with their counts: cnt - 1 differences of kb bits, then -- from the next
// word boundary -- cnt count fields of vb bits, both LSB-first in little-endian uint64 words.  kb is the bit length of the largest
// difference.  A count fits vb bits iff bit_length(count + 1) <= vb (the field of all ones means "escape": the count stands in the file's
// escape list, 96 bits); vb is what makes block + escapes smallest, the smallest such vb on a tie.  The host writer (mfx_db.cpp:
// plan_delta_block) and the encoder kernels of the streamed writer (mfx_sort.hip) both call what stands here, so they agree by construction.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MFX_DHD __host__ __device__ __forceinline__
#else
#define MFX_DHD inline
#endif

constexpr uint32_t MFX_DELTA_BLOCK = 4096;     // k-mers per delta-coded block of a sorted flat database
constexpr int      MFX_DELTA_MAX_VBITS = 22;   // widest count field of a block; larger counts are escapes
constexpr int      MFX_DELTA_VBINS = 34;       // bit_length(count + 1) of a 32-bit count: 1 .. 33

MFX_DHD uint32_t mfx_bit_length(uint64_t x) { return x ? 64u - (uint32_t)__builtin_clzll(x) : 0u; }

// the histogram bin of a count (count + 1 of 2^32 - 1 takes 33 bits: 64-bit arithmetic on either side)
MFX_DHD uint32_t mfx_delta_vbin(uint32_t value) { return mfx_bit_length((uint64_t)value + 1ull); }

// vb and the escapes it leaves, from hist[b] = the counts of the block with mfx_delta_vbin == b
MFX_DHD void mfx_delta_vbits(const uint32_t *hist /* [MFX_DELTA_VBINS] */, uint32_t cnt, uint32_t &vb, uint32_t &nesc) {
  uint64_t best = ~0ull;
  uint32_t above = 0;                                         // values that need more than v bits
  vb = 2u;
  nesc = 0u;
  for (int v = MFX_DELTA_VBINS - 1; v >= 2; --v) {
    if (v <= MFX_DELTA_MAX_VBITS) {
      const uint64_t cost = (uint64_t)cnt * (uint64_t)v + 96ull * above;
      if (cost <= best) { best = cost; vb = (uint32_t)v; nesc = above; }
    }
    above += hist[v];
  }
}

// the words of a block's two parts, and its bytes
MFX_DHD uint64_t mfx_delta_kwords(uint32_t cnt, uint32_t kb) { return ((uint64_t)(cnt - 1u) * kb + 63u) / 64u; }
MFX_DHD uint64_t mfx_delta_vwords(uint32_t cnt, uint32_t vb) { return ((uint64_t)cnt * vb + 63u) / 64u; }
MFX_DHD uint64_t mfx_delta_bytes(uint32_t cnt, uint32_t kb, uint32_t vb) { return (mfx_delta_kwords(cnt, kb) + mfx_delta_vwords(cnt, vb)) * 8u; }
