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

// the entries of the bins [bin_lo, bin_hi) with a non-zero count on `side`; nothing is written beyond cap.  One reservation per workgroup and
// MFX_DB_EXPORT_SLOTS slots a lane: every reservation is a returning atomic on ONE address, and those are served one after the other -- at one
// per wave and 64 slots they, not the table's bytes, set the time of a scan (0.75 s over a table of 68.7 GB; profiles/count_stream.txt)
constexpr uint32_t MFX_DB_EXPORT_SLOTS = 4;

__global__ __launch_bounds__(MFX_BLOCK) void mfx_db_export_kernel(mfx_table_view t, int side, int shift, uint32_t bin_lo, uint32_t bin_hi, uint64_t *keys,
                                                                  uint32_t *vals, uint64_t cap, unsigned long long *count) {
  __shared__ uint32_t s_wave[MFX_BLOCK / 64];
  __shared__ unsigned long long s_base;
  const uint64_t nslots = t.nlines * MFX_SLOTS_LINE, per = (uint64_t)MFX_BLOCK * MFX_DB_EXPORT_SLOTS, stride = (uint64_t)gridDim.x * per;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t base = (uint64_t)blockIdx.x * per; base < nslots; base += stride) {                 // workgroup-uniform trip count
    uint64_t key[MFX_DB_EXPORT_SLOTS];
    uint32_t v[MFX_DB_EXPORT_SLOTS];
    unsigned long long m[MFX_DB_EXPORT_SLOTS];
    uint32_t mine = 0;                                         // the wave's entries
#pragma unroll
    for (uint32_t u = 0; u < MFX_DB_EXPORT_SLOTS; ++u) {
      const uint64_t i = base + (uint64_t)u * MFX_BLOCK + threadIdx.x;
      key[u] = MFX_EMPTY;
      v[u] = 0u;
      if (i < nslots) {
        const uint4 s = *reinterpret_cast<const uint4 *>(t.slots + i);
        key[u] = (uint64_t)s.x | ((uint64_t)s.y << 32);
        v[u] = side ? s.w : s.z;
      }
      const uint64_t b = key[u] >> shift;
#ifdef MFX_V_DB_EXPORT_ALL                                   // A/B build only: entries without a count on this side are written too (tests/test_gpu_count.py must FAIL on it)
      const bool take = key[u] != MFX_EMPTY && b >= bin_lo && b < bin_hi;
#else
      const bool take = key[u] != MFX_EMPTY && v[u] != 0u && b >= bin_lo && b < bin_hi;
#endif
      m[u] = __ballot(take);
      mine += (uint32_t)__popcll(m[u]);
    }
    if (lane == 0) s_wave[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t all = 0;
      for (uint32_t w = 0; w < MFX_BLOCK / 64; ++w) all += s_wave[w];
      s_base = all ? atomicAdd(count, (unsigned long long)all) : 0ull;
    }
    __syncthreads();
    unsigned long long w0 = s_base;
    for (uint32_t w = 0; w < wave; ++w) w0 += s_wave[w];
#pragma unroll
    for (uint32_t u = 0; u < MFX_DB_EXPORT_SLOTS; ++u) {
      if ((m[u] >> lane) & 1ull) {
        const unsigned long long w = w0 + (unsigned long long)__popcll(m[u] & ((1ull << lane) - 1ull));
        if (w < cap) { keys[w] = key[u]; vals[w] = v[u]; }
      }
      w0 += (unsigned long long)__popcll(m[u]);
    }
    __syncthreads();                                           // (s_wave and s_base are written again in the next round)
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

// ---------------------------------------------------------------------------
// The encoder of the streamed database writer (mfx_db.cpp: mfx_db_writer_open_streamed): the sorted pairs of a key range, the writer's
// carry in front of them, as the delta-coded blocks mfx_db_write_flat makes of them.  Only FULL blocks of MFX_DELTA_BLOCK k-mers are
// encoded here (what stays behind the last of them is the next carry; the file's last, partial block is packed on the host at close), so a
// block is 4095 differences and 4096 counts.  One workgroup per block, twice: the plan kernel finds the widths by the rule of mfx_delta.h,
// the host scans the sizes into offsets (at most 2^16 blocks a range), the pack kernel writes the words and the escapes.
// ---------------------------------------------------------------------------
static_assert(MFX_DELTA_BLOCK % MFX_BLOCK == 0 && MFX_BLOCK % 64 == 0, "a block is whole rounds of the workgroup's waves");
constexpr uint32_t MFX_ENC_WAVES = MFX_BLOCK / 64;

__global__ __launch_bounds__(MFX_BLOCK) void mfx_delta_plan_kernel(const uint64_t *keys, const uint32_t *vals, uint32_t nblocks, mfx_delta_plan *plan) {
  __shared__ uint32_t s_hist[MFX_ENC_WAVES][MFX_DELTA_VBINS];   // per wave: bit_length(count + 1)
  __shared__ uint64_t s_or[MFX_ENC_WAVES];
  const uint32_t b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  if (b >= nblocks) return;                                    // (uniform)
  for (uint32_t j = tid; j < MFX_ENC_WAVES * MFX_DELTA_VBINS; j += MFX_BLOCK) (&s_hist[0][0])[j] = 0u;
  __syncthreads();
  const uint64_t *k = keys + (uint64_t)b * MFX_DELTA_BLOCK;
  const uint32_t *v = vals + (uint64_t)b * MFX_DELTA_BLOCK;
  uint64_t ord = 0;                                            // the OR of the differences has the bit length of the largest
  for (uint32_t i = tid; i < MFX_DELTA_BLOCK; i += MFX_BLOCK) {
    if (i) ord |= k[i] - k[i - 1];
    atomicAdd(&s_hist[wave][mfx_delta_vbin(v[i])], 1u);
  }
  for (int o = 32; o; o >>= 1) ord |= __shfl_xor(ord, o, 64);
  if (lane == 0) s_or[wave] = ord;
  __syncthreads();
  if (tid < MFX_DELTA_VBINS) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < MFX_ENC_WAVES; ++w) s += s_hist[w][tid];
    s_hist[0][tid] = s;                                        // (lane tid alone reads and writes column tid)
  }
  __syncthreads();
  if (tid == 0) {
    uint64_t all = 0;
    for (uint32_t w = 0; w < MFX_ENC_WAVES; ++w) all |= s_or[w];
    uint32_t vb, nesc;
    mfx_delta_vbits(s_hist[0], MFX_DELTA_BLOCK, vb, nesc);
    mfx_delta_plan p;
    p.first = k[0];
    p.widths = mfx_bit_length(all) | (vb << 8);
    p.nesc = nesc;
    plan[b] = p;
  }
}

// the 64 bits [64 w, 64 w + 64) of a stream of n fields of `bits` bits each, field i = f(i): every field that overlaps the word, shifted into place
template <class F>
__device__ __forceinline__ uint64_t mfx_delta_word(uint32_t w, uint32_t bits, uint32_t n, F &&f) {
  const int32_t bit0 = (int32_t)(w * 64u);                    // (a block's part has at most 4095 x 62 bits)
  uint64_t word = 0;
  for (uint32_t i = (uint32_t)bit0 / bits; i < n && (int32_t)(i * bits) < bit0 + 64; ++i) {
    const int32_t pos = (int32_t)(i * bits) - bit0;            // > -bits
    const uint64_t x = f(i);
    word |= pos >= 0 ? x << pos : x >> -pos;
  }
  return word;
}

__global__ __launch_bounds__(MFX_BLOCK) void mfx_delta_pack_kernel(const uint64_t *keys, const uint32_t *vals, uint32_t nblocks, const mfx_delta_plan *plan,
                                                                   const uint64_t *word_off, const uint32_t *esc_off, uint64_t *out, uint64_t *esc_keys,
                                                                   uint32_t *esc_vals) {
  __shared__ uint64_t s_k[MFX_DELTA_BLOCK];                    // the block's k-mers; then, in its first half, the count fields
  __shared__ uint32_t s_cnt[MFX_ENC_WAVES];
  const uint32_t b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  if (b >= nblocks) return;                                    // (uniform)
  const uint64_t *k = keys + (uint64_t)b * MFX_DELTA_BLOCK;
  const uint32_t *v = vals + (uint64_t)b * MFX_DELTA_BLOCK;
  const uint32_t kb = plan[b].widths & 0xffu, vb = plan[b].widths >> 8, nesc = plan[b].nesc;
  uint64_t *o = out + word_off[b];
  for (uint32_t i = tid; i < MFX_DELTA_BLOCK; i += MFX_BLOCK) s_k[i] = k[i];
  __syncthreads();
  const uint32_t kwords = (uint32_t)mfx_delta_kwords(MFX_DELTA_BLOCK, kb), vwords = (uint32_t)mfx_delta_vwords(MFX_DELTA_BLOCK, vb);
  for (uint32_t w = tid; w < kwords; w += MFX_BLOCK)           // (kb == 0: no word)
    o[w] = mfx_delta_word(w, kb, MFX_DELTA_BLOCK - 1u, [&](uint32_t i) { return s_k[i + 1] - s_k[i]; });
  __syncthreads();
  uint32_t *s_v = reinterpret_cast<uint32_t *>(s_k);
  const uint32_t esc = (1u << vb) - 1u;
  for (uint32_t i = tid; i < MFX_DELTA_BLOCK; i += MFX_BLOCK) { const uint32_t x = v[i]; s_v[i] = x >= esc ? esc : x; }
  __syncthreads();
  for (uint32_t w = tid; w < vwords; w += MFX_BLOCK)
    o[kwords + w] = mfx_delta_word(w, vb, MFX_DELTA_BLOCK, [&](uint32_t i) { return (uint64_t)s_v[i]; });
  if (nesc == 0u) return;                                      // (uniform)
  // the escapes in index order: per round of MFX_BLOCK fields a ballot per wave and the waves' counts in front of it
  uint32_t base = esc_off[b];
  for (uint32_t r = 0; r < MFX_DELTA_BLOCK; r += MFX_BLOCK) {
    const uint32_t i = r + tid;
    const bool take = s_v[i] == esc;
    const unsigned long long m = __ballot(take);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < MFX_ENC_WAVES; ++w) { const uint32_t c = s_cnt[w]; total += c; if (w < wave) before += c; }
    if (take) {
      const uint32_t at = base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (at < esc_off[b] + nesc) { esc_keys[at] = k[i]; esc_vals[at] = v[i]; }      // (never beyond what the plan counted)
    }
    base += total;
    __syncthreads();
  }
}

hipError_t mfx_k_delta_plan(const uint64_t *keys, const uint32_t *vals, uint32_t nblocks, mfx_delta_plan *plan, hipStream_t st) {
  if (nblocks == 0) return hipSuccess;
  mfx_delta_plan_kernel<<<nblocks, MFX_BLOCK, 0, st>>>(keys, vals, nblocks, plan);
  return hipGetLastError();
}

hipError_t mfx_k_delta_pack(const uint64_t *keys, const uint32_t *vals, uint32_t nblocks, const mfx_delta_plan *plan, const uint64_t *word_off,
                            const uint32_t *esc_off, uint64_t *out, uint64_t *esc_keys, uint32_t *esc_vals, hipStream_t st) {
  if (nblocks == 0) return hipSuccess;
  mfx_delta_pack_kernel<<<nblocks, MFX_BLOCK, 0, st>>>(keys, vals, nblocks, plan, word_off, esc_off, out, esc_keys, esc_vals);
  return hipGetLastError();
}
