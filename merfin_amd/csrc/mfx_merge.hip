// mfx_merge.hip -- the device part of mfx_db_merge (mfx_db.cpp): the blocks of sorted, delta-coded databases decoded into ascending
// (k-mer, count) runs, the runs merged pairwise, equal k-mers combined and filtered.  What leaves the last kernel is ascending and dense:
// the streamed database writer's encoder (mfx_sort.hip) takes it as it takes a sorted key range of a table.  No hash table, no sort.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfx_device.h"
#include "mfx_merge.h"                                         // mfx_merge_cut

// ---------------------------------------------------------------------------
// mfx_delta_decode_kernel: one workgroup per (input, block) of a window; the decode is mfx_table_add_delta_kernel's (mfx_device.h).  The
// block's records go to keys / vals from t.out on, all of them: the records of an input's blocks outside the window [lo, hi) are a prefix
// of its first block and a suffix of its last, so the host only needs their numbers (below / above, per block) to know the dense run.
// A count field of all ones is an escape: the count stands in the input's escape list, whose slice for this window [esc_lo, esc_hi) is
// ascending.  What no writer makes is reported in err[input] and nothing of the window is written to the output file: k-mers that do not ascend
// strictly or reach the next block's first (MFX_MERGE_ERR_ORDER), an escape that is not in the list (.._ESCAPE), a count of zero (.._ZERO).
// The inputs from zero_from on are decoded and checked like the others and then leave with a count of 0: the mark of a k-mer to subtract.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mfx_delta_decode_kernel(const mfx_merge_task *tasks, uint32_t ntasks, const uint64_t *payload, const uint64_t *esc_keys,
                                                               const uint32_t *esc_vals, uint64_t lo, uint64_t hi, uint64_t *keys, uint32_t *vals,
                                                               uint32_t *below, uint32_t *above, uint32_t *err, uint32_t zero_from) {
  __shared__ uint64_t wsum[4];
  __shared__ uint32_t s_cnt[4][2];
  if (blockIdx.x >= ntasks) return;                            // (uniform)
  const mfx_merge_task t = tasks[blockIdx.x];
  const uint32_t tid = threadIdx.x, wv = tid >> 6, ln = tid & 63u, e0 = tid * MFX_DELTA_PER_LANE;
  const mfx_delta_blk B = mfx_delta_blk_open(payload + t.word_off, t.first, t.kb, t.vb, t.cnt);
  const uint32_t esc = (1u << B.vb) - 1u;
  uint64_t run = mfx_delta_lane_start(B, wsum);
  uint32_t bad = 0u, nb = 0u, na = 0u;
#pragma unroll 4
  for (uint32_t i = 0; i < MFX_DELTA_PER_LANE; ++i) {
    const uint32_t e = e0 + i;
    if (e >= B.cnt) break;
    if (e > 0u) {
      const uint64_t prev = run;
      if (B.kb) run += mfx_delta_diff(B, e);
      if (!(run > prev)) bad |= MFX_MERGE_ERR_ORDER;           // (a sum that wrapped is below the k-mer before it)
    }
    if (run >= t.limit) bad |= MFX_MERGE_ERR_ORDER;
    uint32_t v = mfx_delta_field(B, e);
    if (v == esc && run >= lo && run < hi) {                   // (a record outside the window is dropped: its escape is not in the slice)
      uint32_t a = t.esc_lo, b = t.esc_hi;                     // the first escape at or above this k-mer
      while (a < b) { const uint32_t m = a + (b - a) / 2u; if (esc_keys[m] < run) a = m + 1u; else b = m; }
      if (a < t.esc_hi && esc_keys[a] == run) v = esc_vals[a];
      else bad |= MFX_MERGE_ERR_ESCAPE;
    }
    if (v == 0u) bad |= MFX_MERGE_ERR_ZERO;
    if (t.input >= zero_from) v = 0u;                          // an input that is subtracted (mfx_db_merge_except): its k-mers, whatever their counts
    nb += run < lo ? 1u : 0u;
    na += run >= hi ? 1u : 0u;
    keys[t.out + e] = run;
    vals[t.out + e] = v;
  }
  for (int o = 32; o; o >>= 1) { nb += __shfl_xor(nb, o, 64); na += __shfl_xor(na, o, 64); bad |= __shfl_xor(bad, o, 64); }
  if (ln == 0u) {
    s_cnt[wv][0] = nb;
    s_cnt[wv][1] = na;
    if (bad) atomicOr(err + t.input, bad);
  }
  __syncthreads();
  if (tid == 0u) {
    below[blockIdx.x] = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
    above[blockIdx.x] = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
  }
}

// ---------------------------------------------------------------------------
// mfx_merge_pairs_kernel: two ascending runs into one, by merge path.  A workgroup makes MFX_MERGE_TILE consecutive pairs of the output: it
// finds where its first and its last diagonal cut the two runs (binary searches in global memory), stages its two pieces in LDS (24 KB: the
// k-mers and the counts of a tile), every lane finds its own diagonal's cut in LDS and merges MFX_MERGE_PER pairs into registers, the pairs go
// back to LDS in output order and leave in one contiguous, coalesced piece.  Equal k-mers stay, the first run's in front.  24 bytes move per
// pair and level.  (24 KB a workgroup of 256 lanes: six of them in the 160 KB of a CU, beside the pack kernel's 32 KB and five.)
// ---------------------------------------------------------------------------
constexpr uint32_t MFX_MERGE_PER = 8;
constexpr uint32_t MFX_MERGE_TILE = 256u * MFX_MERGE_PER;

__global__ __launch_bounds__(256) void mfx_merge_pairs_kernel(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *kb, const uint32_t *vb,
                                                              uint64_t lb, uint64_t *ko, uint32_t *vo) {
  __shared__ uint64_t s_k[MFX_MERGE_TILE];
  __shared__ uint32_t s_v[MFX_MERGE_TILE];
  __shared__ uint64_t s_cut[2];
  const uint32_t tid = threadIdx.x;
  const uint64_t total = la + lb, d0 = (uint64_t)blockIdx.x * MFX_MERGE_TILE;
  if (d0 >= total) return;                                     // (uniform)
  const uint64_t d1 = d0 + MFX_MERGE_TILE < total ? d0 + MFX_MERGE_TILE : total;
  if (tid < 2u) s_cut[tid] = mfx_merge_cut<uint64_t>(ka, la, kb, lb, tid ? d1 : d0);
  __syncthreads();
  const uint64_t a0 = s_cut[0], b0 = d0 - a0;
  const uint32_t na = (uint32_t)(s_cut[1] - a0), n = (uint32_t)(d1 - d0), nb = n - na;
  for (uint32_t i = tid; i < n; i += 256u) {
    s_k[i] = i < na ? ka[a0 + i] : kb[b0 + (i - na)];
    s_v[i] = i < na ? va[a0 + i] : vb[b0 + (i - na)];
  }
  __syncthreads();
  const uint32_t t0 = tid * MFX_MERGE_PER < n ? tid * MFX_MERGE_PER : n, t1 = t0 + MFX_MERGE_PER < n ? t0 + MFX_MERGE_PER : n;
  uint64_t rk[MFX_MERGE_PER];
  uint32_t rv[MFX_MERGE_PER];
  {
    uint32_t i = mfx_merge_cut<uint32_t>(s_k, na, s_k + na, nb, t0), j = t0 - i;
#pragma unroll
    for (uint32_t r = 0; r < MFX_MERGE_PER; ++r) {
      rk[r] = 0; rv[r] = 0u;
      if (t0 + r < t1) {
        const bool from_a = j >= nb || (i < na && s_k[i] <= s_k[na + j]);
        const uint32_t at = from_a ? i : na + j;
        rk[r] = s_k[at]; rv[r] = s_v[at];
        if (from_a) ++i; else ++j;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < MFX_MERGE_PER; ++r)
    if (t0 + r < t1) { s_k[t0 + r] = rk[r]; s_v[t0 + r] = rv[r]; }
  __syncthreads();
  for (uint32_t i = tid; i < n; i += 256u) { ko[d0 + i] = s_k[i]; vo[d0 + i] = s_v[i]; }
}

// ---------------------------------------------------------------------------
// mfx_combine_kernel: the merged run, equal k-mers side by side, into one record per k-mer.  A position whose k-mer differs from the one
// before it is a head; it walks its equal k-mers (one per input at the most) and applies the operation, then the filter on the combined
// count.  The survivors are compacted in order without an atomic that could reorder them: the kernel runs twice over tiles of MFX_COMB_TILE
// positions -- the first run leaves every tile's number of survivors, a one-workgroup scan turns them into offsets, the second run computes
// the same again and stores.  Within a tile: rounds of 256 positions, a ballot per wave and the waves' counts in front of it.
// stats (second run): [0] sums clamped to 2^32 - 1, [1] k-mers the operation yields and the filter drops, [2] k-mers the operation yields and a
// subtracted input holds.  n_in: the inputs of the operation, the subtracted ones not counted.
// ---------------------------------------------------------------------------
constexpr uint32_t MFX_COMB_ROUNDS = 8;
constexpr uint32_t MFX_COMB_TILE = 256u * MFX_COMB_ROUNDS;

template <bool SCATTER>
__global__ __launch_bounds__(256) void mfx_combine_kernel(const uint64_t *keys, const uint32_t *vals, uint64_t n, uint32_t n_in, int op, uint64_t minV, uint64_t maxV,
                                                          uint64_t *tile_off, uint64_t *out_keys, uint32_t *out_vals, unsigned long long *stats) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t tid = threadIdx.x, wv = tid >> 6, ln = tid & 63u;
  uint64_t base = SCATTER ? tile_off[blockIdx.x] : 0ull;
  uint32_t nsat = 0u, nfilt = 0u, nbar = 0u;
  for (uint32_t r = 0; r < MFX_COMB_ROUNDS; ++r) {             // (uniform)
    const uint64_t i = (uint64_t)blockIdx.x * MFX_COMB_TILE + (uint64_t)r * 256u + tid;
    bool take = false;
    uint64_t key = 0;
    uint32_t c = 0u;
    if (i < n) {
      key = keys[i];
      if (i == 0 || keys[i - 1] != key) {
        // (a count of 0 is a subtracted input's: it is no member of the operation, and its k-mer is not written)
        uint32_t v = vals[i], mn = v ? v : 0xffffffffu, mx = v, len = v ? 1u : 0u;
        uint64_t sum = v;
        bool barred = v == 0u;
        for (uint64_t j = i + 1; j < n && keys[j] == key; ++j) {
          v = vals[j];
          if (v == 0u) { barred = true; continue; }
          sum += v;
          mn = v < mn ? v : mn;
          mx = v > mx ? v : mx;
          ++len;
        }
        bool yields = len != 0u;
        if (op == MFX_MERGE_SUM) {
          if (sum > 0xffffffffull) { sum = 0xffffffffull; ++nsat; }
          c = (uint32_t)sum;
        } else if (op == MFX_MERGE_MAX) c = mx;
        else {
          c = mn;
          if (op == MFX_MERGE_INTERSECT) yields = len == n_in;
        }
        if (yields && barred) { yields = false; ++nbar; }
        if (yields) {
          take = (uint64_t)c >= minV && (uint64_t)c <= maxV;
          if (!take) ++nfilt;
        }
      }
    }
    const unsigned long long m = __ballot(take);
    if (ln == 0u) s_cnt[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0u, total = 0u;
    for (uint32_t w = 0; w < 4u; ++w) { const uint32_t x = s_cnt[w]; total += x; if (w < wv) before += x; }
    if (SCATTER && take) {
      const uint64_t at = base + before + (uint32_t)__popcll(m & ((1ull << ln) - 1ull));
      out_keys[at] = key;
      out_vals[at] = c;
    }
    base += total;
    __syncthreads();                                           // (s_cnt is written again in the next round)
  }
  if (!SCATTER) {
    if (tid == 0u) tile_off[blockIdx.x] = base;
    return;
  }
  for (int o = 32; o; o >>= 1) { nsat += __shfl_xor(nsat, o, 64); nfilt += __shfl_xor(nfilt, o, 64); nbar += __shfl_xor(nbar, o, 64); }
  if (ln == 0u) {
    if (nsat) atomicAdd(&stats[0], (unsigned long long)nsat);
    if (nfilt) atomicAdd(&stats[1], (unsigned long long)nfilt);
    if (nbar) atomicAdd(&stats[2], (unsigned long long)nbar);
  }
}

// t[0 .. n) -> their exclusive prefix sums, t[n] = the total; one workgroup
__global__ __launch_bounds__(256) void mfx_tile_scan_kernel(uint64_t *t, uint32_t n) {
  __shared__ uint64_t s_w[4];
  __shared__ uint64_t s_carry;
  const uint32_t tid = threadIdx.x, wv = tid >> 6, ln = tid & 63u;
  if (tid == 0u) s_carry = 0ull;
  __syncthreads();
  for (uint32_t b = 0; b < n; b += 256u) {                     // (uniform)
    const uint32_t i = b + tid;
    const uint64_t x = i < n ? t[i] : 0ull;
    uint64_t inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint64_t u = __shfl_up(inc, o, 64); if ((int)ln >= o) inc += u; }
    if (ln == 63u) s_w[wv] = inc;
    __syncthreads();
    uint64_t pre = s_carry;
    for (uint32_t w = 0; w < wv; ++w) pre += s_w[w];
    if (i < n) t[i] = pre + inc - x;
    __syncthreads();                                           // (s_carry and s_w are read by now)
    if (tid == 255u) s_carry = pre + inc;
    __syncthreads();
  }
  if (tid == 0u) t[n] = s_carry;
}

hipError_t mfx_k_delta_decode(const mfx_merge_task *tasks, uint32_t ntasks, const uint64_t *payload, const uint64_t *esc_keys, const uint32_t *esc_vals, uint64_t lo,
                              uint64_t hi, uint64_t *keys, uint32_t *vals, uint32_t *below, uint32_t *above, uint32_t *err, hipStream_t st, uint32_t zero_from) {
  if (ntasks == 0) return hipSuccess;
  mfx_delta_decode_kernel<<<ntasks, 256, 0, st>>>(tasks, ntasks, payload, esc_keys, esc_vals, lo, hi, keys, vals, below, above, err, zero_from);
  return hipGetLastError();
}

hipError_t mfx_k_merge_pairs(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *kb, const uint32_t *vb, uint64_t lb, uint64_t *ko, uint32_t *vo,
                             hipStream_t st) {
  const uint64_t tiles = (la + lb + MFX_MERGE_TILE - 1) / MFX_MERGE_TILE;
  if (tiles == 0) return hipSuccess;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  mfx_merge_pairs_kernel<<<(unsigned)tiles, 256, 0, st>>>(ka, va, la, kb, vb, lb, ko, vo);
  return hipGetLastError();
}

uint64_t mfx_combine_tiles(uint64_t n) { return (n + MFX_COMB_TILE - 1) / MFX_COMB_TILE; }

// tile_off: mfx_combine_tiles(n) + 1 words; the number of survivors is its last word when the stream has run
hipError_t mfx_k_combine(const uint64_t *keys, const uint32_t *vals, uint64_t n, uint32_t n_in, int op, uint64_t minV, uint64_t maxV, uint64_t *tile_off,
                         uint64_t *out_keys, uint32_t *out_vals, uint64_t *stats, hipStream_t st) {
  const uint64_t tiles = mfx_combine_tiles(n);
  if (tiles == 0) return hipSuccess;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  unsigned long long *s = reinterpret_cast<unsigned long long *>(stats);
  mfx_combine_kernel<false><<<(unsigned)tiles, 256, 0, st>>>(keys, vals, n, n_in, op, minV, maxV, tile_off, out_keys, out_vals, s);
  mfx_tile_scan_kernel<<<1, 256, 0, st>>>(tile_off, (uint32_t)tiles);
  mfx_combine_kernel<true><<<(unsigned)tiles, 256, 0, st>>>(keys, vals, n, n_in, op, minV, maxV, tile_off, out_keys, out_vals, s);
  return hipGetLastError();
}
