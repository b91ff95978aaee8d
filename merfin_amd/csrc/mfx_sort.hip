// mfx_sort.hip -- what is built on hipCUB (rocPRIM): the stable radix sort of (owner rank -> position index) pairs for the
// sharded-index query exchange (8-bit keys, one pass), and the device part of mfx_index_write_db (below).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "mfx_internal.h"
#include "mfx_kernels.h"

int mfx_sort_by_owner(void *tmp, size_t &tmp_bytes, const uint8_t *kin, uint8_t *kout, const uint32_t *vin, uint32_t *vout,
                      uint64_t n, hipStream_t st) {
  // hipCUB counts its items in an int; the values sorted here are 32-bit position indexes of one routed chunk
  // (mfx_route_tiles: max_tiles * MFX_TILE positions), so a chunk beyond 2^31 - 1 keys is refused, never truncated
  if (n > (uint64_t)INT32_MAX) return mfx_fail(MFX_E_INVAL, "mfx_sort_by_owner: %lu keys in one routed chunk (at most %d)", (unsigned long)n, INT32_MAX);
  if (tmp == nullptr) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint8_t *)nullptr, (uint8_t *)nullptr, (const uint32_t *)nullptr,
                                       (uint32_t *)nullptr, (int)n, 0, 8, st);
    tmp_bytes = b;
    return MFX_OK;
  }
  if (n == 0) return MFX_OK;
  size_t b = tmp_bytes;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(tmp, b, kin, kout, vin, vout, (int)n, 0, 8, st);
  if (e != hipSuccess) return mfx_fail(MFX_E_HIP, "radix sort failed: %s", hipGetErrorString(e));
  return MFX_OK;
}

// ---------------------------------------------------------------------------
// mfx_index_write_db (mfx_db.cpp): the entries of a full table of 16-byte slots as a sorted database.  One streaming pass counts the
// entries per bin of their top key bits; per range of bins the entries are compacted out of the table and sorted here.
// ---------------------------------------------------------------------------
constexpr uint32_t MFX_DB_BINS_MAX = 4096;                   // (mfx_db.cpp: MFX_DB_BIN_BITS = 12)

__global__ __launch_bounds__(MFX_BLOCK) void mfx_db_bins_kernel(mfx_table_view t, int side, int shift, uint32_t nbins, unsigned long long *bins) {
  __shared__ uint32_t s_bins[MFX_DB_BINS_MAX];               // per block: a table has at most 2^35 slots and a large one 4096 blocks, 2^23 slots each
  for (uint32_t j = threadIdx.x; j < nbins; j += MFX_BLOCK) s_bins[j] = 0u;
  __syncthreads();
  const uint64_t nslots = t.nlines * MFX_SLOTS_LINE, stride = (uint64_t)gridDim.x * MFX_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * MFX_BLOCK + threadIdx.x; i < nslots; i += stride) {
    const uint4 s = *reinterpret_cast<const uint4 *>(t.slots + i);
    const uint64_t key = (uint64_t)s.x | ((uint64_t)s.y << 32);
#ifdef MFX_V_DB_EXPORT_ALL
    if (key == MFX_EMPTY) continue;
#else
    if (key == MFX_EMPTY || (side ? s.w : s.z) == 0u) continue;
#endif
    const uint64_t b = key >> shift;
    if (b < nbins) atomicAdd(&s_bins[(uint32_t)b], 1u);      // (a key wider than 2k bits is never in a table: mfx_table_add_kernel refuses it)
  }
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < nbins; j += MFX_BLOCK)
    if (s_bins[j]) atomicAdd(&bins[j], (unsigned long long)s_bins[j]);
}

// the entries of the bins [bin_lo, bin_hi) with a non-zero count on `side`: one reservation per wave, nothing is written beyond cap
__global__ __launch_bounds__(MFX_BLOCK) void mfx_db_export_kernel(mfx_table_view t, int side, int shift, uint32_t bin_lo, uint32_t bin_hi, uint64_t *keys,
                                                                  uint32_t *vals, uint64_t cap, unsigned long long *count) {
  const uint64_t nslots = t.nlines * MFX_SLOTS_LINE, stride = (uint64_t)gridDim.x * MFX_BLOCK;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t base = (uint64_t)blockIdx.x * MFX_BLOCK; base < nslots; base += stride) {          // wave-uniform trip count
    const uint64_t i = base + threadIdx.x;
    uint64_t key = MFX_EMPTY;
    uint32_t v = 0u;
    if (i < nslots) {
      const uint4 s = *reinterpret_cast<const uint4 *>(t.slots + i);
      key = (uint64_t)s.x | ((uint64_t)s.y << 32);
      v = side ? s.w : s.z;
    }
    const uint64_t b = key >> shift;
#ifdef MFX_V_DB_EXPORT_ALL                                   // A/B build only: entries without a count on this side are written too (tests/test_gpu_count.py must FAIL on it)
    const bool take = key != MFX_EMPTY && b >= bin_lo && b < bin_hi;
#else
    const bool take = key != MFX_EMPTY && v != 0u && b >= bin_lo && b < bin_hi;
#endif
    const unsigned long long m = __ballot(take);
    if (m == 0ull) continue;
    unsigned long long w0 = 0;
    if (lane == 0) w0 = atomicAdd(count, (unsigned long long)__popcll(m));
    w0 = __shfl(w0, 0, 64);
    if (take) {
      const unsigned long long w = w0 + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
      if (w < cap) { keys[w] = key; vals[w] = v; }
    }
  }
}

static unsigned mfx_db_grid(uint64_t nslots) {
  const uint64_t blocks = (nslots + MFX_BLOCK - 1) / MFX_BLOCK;
  return (unsigned)(blocks < 4096 ? blocks : 4096);
}

hipError_t mfx_k_db_bins(mfx_table_view t, int side, int shift, uint32_t nbins, uint64_t *bins, hipStream_t st) {
  if (nbins > MFX_DB_BINS_MAX) return hipErrorInvalidValue;
  mfx_db_bins_kernel<<<mfx_db_grid(t.nlines * MFX_SLOTS_LINE), MFX_BLOCK, 0, st>>>(t, side, shift, nbins, reinterpret_cast<unsigned long long *>(bins));
  return hipGetLastError();
}

hipError_t mfx_k_db_export(mfx_table_view t, int side, int shift, uint32_t bin_lo, uint32_t bin_hi, uint64_t *keys, uint32_t *vals, uint64_t cap,
                           unsigned long long *count, hipStream_t st) {
  mfx_db_export_kernel<<<mfx_db_grid(t.nlines * MFX_SLOTS_LINE), MFX_BLOCK, 0, st>>>(t, side, shift, bin_lo, bin_hi, keys, vals, cap, count);
  return hipGetLastError();
}

int mfx_sort_db_pairs(void *tmp, size_t &tmp_bytes, const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, uint64_t n, int key_bits,
                      hipStream_t st) {
  // (hipCUB counts its items in an int: a range beyond 2^31 - 1 entries is refused, never truncated)
  if (n > (uint64_t)INT32_MAX) return mfx_fail(MFX_E_INVAL, "mfx_index_write_db: %lu k-mers in one key range (at most %d)", (unsigned long)n, INT32_MAX);
  if (tmp == nullptr) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (int)n, 0, key_bits, st);
    tmp_bytes = b;
    return MFX_OK;
  }
  if (n == 0) return MFX_OK;
  size_t b = tmp_bytes;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(tmp, b, kin, kout, vin, vout, (int)n, 0, key_bits, st);
  if (e != hipSuccess) return mfx_fail(MFX_E_HIP, "radix sort failed: %s", hipGetErrorString(e));
  return MFX_OK;
}
