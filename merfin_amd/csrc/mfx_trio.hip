// mfx_trio.hip -- the device part of mfx_db_trio, mfx_db_trio_hist and mfx_db_histogram (mfx_db.cpp).  The windows, the block decode and the
// pairwise merge are mfx_db_merge's (mfx_merge.hip), unchanged; what is new is that the merged run knows which input a record came from
// (the role in the two low bits of the key, mfx_trio.h), a histogram pass over it and a classify pass that compacts TWO outputs at once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfx_device.h"
#include "mfx_kernels.h"
#include "mfx_spectrum.h"
#include "mfx_trio.h"

// ---------------------------------------------------------------------------
// mfx_trio_tag_kernel: keys[i] -> mfx_trio_tag(keys[i], role), in place, over one input's decoded run (ascending before and after).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mfx_trio_tag_kernel(uint64_t *keys, uint64_t n, uint32_t role) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) keys[i] = mfx_trio_tag(keys[i], role);
}

// ---------------------------------------------------------------------------
// mfx_trio_hist_kernel (pass 1): the three histogram rows of a tagged merged run.  A head position gathers its k-mer's at most three records
// and adds one to row 0 or row 1 where the rule says so (mfx_trio_rule: prow) and one to row 2 where the child holds the k-mer.  The bins are
// mfx_spectrum.h's as they are, with copies = 1: an image of copies + 2 = 3 rows, the row chosen through the "assembly count" argument, the
// column through the "read count" -- 32-bit LDS bins for the low columns, flushed per workgroup, 64-bit global atomics beyond, the counter
// word behind the image.  Exact integer adds: the order takes no part.  The workgroups are persistent (24 KB of bins set up and flushed once
// each); every lane of a wave calls mfx_spec_count in every turn (its aggregated form votes).  A workgroup adds at most two to a bin per
// position and n < 2^31 (mfx_k_trio_hist): no LDS bin wraps.  With the child's role alone in the run this is `meryl histogram`: every k-mer
// goes to row 2.
// ---------------------------------------------------------------------------
template <bool AGG>
__global__ __launch_bounds__(256) void mfx_trio_hist_kernel(const uint64_t *keys, const uint32_t *vals, uint64_t n, mfx_spectrum_args a) {
  __shared__ uint32_t s_bins[MFX_SPEC_LDS_WORDS];
  mfx_spec_begin(a, s_bins);
  uint64_t counted = 0;
  const mfx_trio_cuts none{1u, 1u, 1u, true};
  for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < n; base += (uint64_t)gridDim.x * 256u) {      // (uniform)
    const uint64_t i = base + threadIdx.x;
    uint32_t c[3] = {0u, 0u, 0u}, prow = MFX_TRIO_NOROW;
    if (i < n && mfx_trio_head(keys, i)) {
      mfx_trio_gather(keys, vals, n, i, c);
      prow = mfx_trio_rule(c[0], c[1], c[2], none).prow;
    }
    const bool par = prow != MFX_TRIO_NOROW;
    counted += mfx_spec_count<AGG>(a, s_bins, par, par ? c[prow] : 0u, par ? prow : 0u);
    counted += mfx_spec_count<AGG>(a, s_bins, c[2] != 0u, c[2], MFX_TRIO_CHILD);
  }
  mfx_spec_end(a, s_bins, counted);
}

// ---------------------------------------------------------------------------
// mfx_trio_classify_kernel (pass 2): mfx_combine_kernel's shape -- tiles of MFX_TRIO_TILE positions of the merged run, a count run, one scan,
// a scatter run that computes the same again and stores -- with two compactions at once.  Per round of 256 positions a ballot for "goes to
// A" and a ballot for "goes to B", the waves' counts of both in LDS; per tile both survivor numbers (tile_off[2 t], [2 t + 1]), which
// mfx_tile_scan2_kernel turns into the offsets of both outputs in one launch.  Both outputs leave ascending and dense, the role bits taken
// off again; no atomic orders anything, so a second run gives the same bytes.  stats (scatter run; MFX_TRIO_S_*): summed in registers, reduced
// per wave and then per workgroup in LDS, one 64-bit add per workgroup and statistic, into the workgroup's copy of the counters
// (MFX_TRIO_STAT_SHARDS copies, mfx_trio.h).
// ---------------------------------------------------------------------------
constexpr uint32_t MFX_TRIO_ROUNDS = 8;
constexpr uint32_t MFX_TRIO_TILE = 256u * MFX_TRIO_ROUNDS;

template <bool SCATTER>
__global__ __launch_bounds__(256) void mfx_trio_classify_kernel(const uint64_t *keys, const uint32_t *vals, uint64_t n, mfx_trio_cuts cuts, uint64_t *tile_off,
                                                                uint64_t *a_keys, uint32_t *a_vals, uint64_t *b_keys, uint32_t *b_vals, unsigned long long *stats) {
  __shared__ uint32_t s_cnt[4][2];
  __shared__ uint32_t s_st[4][MFX_TRIO_NSTATS];
  const uint32_t tid = threadIdx.x, wv = tid >> 6, ln = tid & 63u;
  uint64_t base_a = SCATTER ? tile_off[2ull * blockIdx.x] : 0ull, base_b = SCATTER ? tile_off[2ull * blockIdx.x + 1] : 0ull;
  uint32_t st[MFX_TRIO_NSTATS] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (uint32_t r = 0; r < MFX_TRIO_ROUNDS; ++r) {             // (uniform)
    const uint64_t i = (uint64_t)blockIdx.x * MFX_TRIO_TILE + (uint64_t)r * 256u + tid;
    uint32_t set = MFX_TRIO_NONE, cnt = 0u;
    uint64_t kmer = 0;
    if (i < n && mfx_trio_head(keys, i)) {
      uint32_t c[3];
      mfx_trio_gather(keys, vals, n, i, c);
      const mfx_trio_class k = mfx_trio_rule(c[0], c[1], c[2], cuts);
      set = k.set; cnt = k.count; kmer = mfx_trio_kmer(keys[i]);
      if (SCATTER) {
        st[MFX_TRIO_S_BOTH] += k.both; st[MFX_TRIO_S_MAT_ONLY] += k.mat_only; st[MFX_TRIO_S_PAT_ONLY] += k.pat_only;
        st[MFX_TRIO_S_MAT_CUT] += k.mat_cut; st[MFX_TRIO_S_PAT_CUT] += k.pat_cut; st[MFX_TRIO_S_CHILD_CUT] += k.child_cut;
      }
    }
    const unsigned long long ma = __ballot(set == MFX_TRIO_A), mb = __ballot(set == MFX_TRIO_B);
    if (ln == 0u) { s_cnt[wv][0] = (uint32_t)__popcll(ma); s_cnt[wv][1] = (uint32_t)__popcll(mb); }
    __syncthreads();
    uint32_t before_a = 0u, total_a = 0u, before_b = 0u, total_b = 0u;
    for (uint32_t w = 0; w < 4u; ++w) {
      const uint32_t xa = s_cnt[w][0], xb = s_cnt[w][1];
      total_a += xa; total_b += xb;
      if (w < wv) { before_a += xa; before_b += xb; }
    }
    if (SCATTER) {
      const unsigned long long below = (1ull << ln) - 1ull;
      if (set == MFX_TRIO_A) {
        const uint64_t at = base_a + before_a + (uint32_t)__popcll(ma & below);
        a_keys[at] = kmer; a_vals[at] = cnt;
      } else if (set == MFX_TRIO_B) {
        const uint64_t at = base_b + before_b + (uint32_t)__popcll(mb & below);
        b_keys[at] = kmer; b_vals[at] = cnt;
      }
    }
    base_a += total_a; base_b += total_b;
    __syncthreads();                                           // (s_cnt is written again in the next round)
  }
  if (!SCATTER) {
    if (tid == 0u) { tile_off[2ull * blockIdx.x] = base_a; tile_off[2ull * blockIdx.x + 1] = base_b; }
    return;
  }
#pragma unroll
  for (uint32_t s = 0; s < (uint32_t)MFX_TRIO_NSTATS; ++s) {
    uint32_t x = st[s];
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
    if (ln == 0u) s_st[wv][s] = x;
  }
  __syncthreads();
  if (tid < (uint32_t)MFX_TRIO_NSTATS) {
    const uint32_t x = s_st[0][tid] + s_st[1][tid] + s_st[2][tid] + s_st[3][tid];      // (a tile holds 2048 positions: no wrap)
    if (x) atomicAdd(&stats[(blockIdx.x % MFX_TRIO_STAT_SHARDS) * MFX_TRIO_STAT_STRIDE + tid], (unsigned long long)x);
  }
}

// t[2 i], t[2 i + 1], i < n -> the exclusive prefix sums of the even and of the odd words, t[2 n], t[2 n + 1] = the two totals; one workgroup
// (mfx_tile_scan_kernel, mfx_merge.hip, over two words per tile)
__global__ __launch_bounds__(256) void mfx_tile_scan2_kernel(uint64_t *t, uint32_t n) {
  __shared__ uint64_t s_w[4][2];
  __shared__ uint64_t s_carry[2];
  const uint32_t tid = threadIdx.x, wv = tid >> 6, ln = tid & 63u;
  if (tid < 2u) s_carry[tid] = 0ull;
  __syncthreads();
  for (uint32_t b = 0; b < n; b += 256u) {                     // (uniform)
    const uint32_t i = b + tid;
    const uint64_t x0 = i < n ? t[2ull * i] : 0ull, x1 = i < n ? t[2ull * i + 1] : 0ull;
    uint64_t i0 = x0, i1 = x1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t u0 = __shfl_up(i0, o, 64), u1 = __shfl_up(i1, o, 64);
      if ((int)ln >= o) { i0 += u0; i1 += u1; }
    }
    if (ln == 63u) { s_w[wv][0] = i0; s_w[wv][1] = i1; }
    __syncthreads();
    uint64_t p0 = s_carry[0], p1 = s_carry[1];
    for (uint32_t w = 0; w < wv; ++w) { p0 += s_w[w][0]; p1 += s_w[w][1]; }
    if (i < n) { t[2ull * i] = p0 + i0 - x0; t[2ull * i + 1] = p1 + i1 - x1; }
    __syncthreads();                                           // (s_carry and s_w are read by now)
    if (tid == 255u) { s_carry[0] = p0 + i0; s_carry[1] = p1 + i1; }
    __syncthreads();
  }
  if (tid < 2u) t[2ull * n + tid] = s_carry[tid];
}

hipError_t mfx_k_trio_tag(uint64_t *keys, uint64_t n, uint32_t role, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + 255u) / 256u;
  mfx_trio_tag_kernel<<<(unsigned)(blocks < 4096u ? blocks : 4096u), 256, 0, st>>>(keys, n, role);
  return hipGetLastError();
}

// a.copies == 1, a.img: 3 rows of a.max_mult + 1 cells and the counter word; grid: the workgroups the device holds at once
hipError_t mfx_k_trio_hist(const uint64_t *keys, const uint32_t *vals, uint64_t n, const mfx_spectrum_args &a, int grid, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n > 0x7fffffffull || a.copies != 1u) return hipErrorInvalidValue;
  const uint64_t blocks = (n + 255u) / 256u, g = blocks < (uint64_t)(grid > 0 ? grid : 1) ? blocks : (uint64_t)(grid > 0 ? grid : 1);
  if (a.aggregate) mfx_trio_hist_kernel<true><<<(unsigned)g, 256, 0, st>>>(keys, vals, n, a);
  else mfx_trio_hist_kernel<false><<<(unsigned)g, 256, 0, st>>>(keys, vals, n, a);
  return hipGetLastError();
}

uint64_t mfx_trio_tiles(uint64_t n) { return (n + MFX_TRIO_TILE - 1) / MFX_TRIO_TILE; }

// tile_off: 2 * (mfx_trio_tiles(n) + 1) words; the survivors of A and of B are its last two words when the stream has run.  stats:
// MFX_TRIO_STAT_WORDS words
hipError_t mfx_k_trio_classify(const uint64_t *keys, const uint32_t *vals, uint64_t n, const mfx_trio_cuts &cuts, uint64_t *tile_off, uint64_t *a_keys, uint32_t *a_vals,
                               uint64_t *b_keys, uint32_t *b_vals, uint64_t *stats, hipStream_t st) {
  const uint64_t tiles = mfx_trio_tiles(n);
  if (tiles == 0) return hipSuccess;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  unsigned long long *s = reinterpret_cast<unsigned long long *>(stats);
  mfx_trio_classify_kernel<false><<<(unsigned)tiles, 256, 0, st>>>(keys, vals, n, cuts, tile_off, a_keys, a_vals, b_keys, b_vals, s);
  mfx_tile_scan2_kernel<<<1, 256, 0, st>>>(tile_off, (uint32_t)tiles);
  mfx_trio_classify_kernel<true><<<(unsigned)tiles, 256, 0, st>>>(keys, vals, n, cuts, tile_off, a_keys, a_vals, b_keys, b_vals, s);
  return hipGetLastError();
}
