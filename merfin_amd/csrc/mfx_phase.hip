// mfx_phase.hip -- pass 2 of -phase (csrc/mfx_phase.h): the two haplotype planes -> runs of one haplotype -> phase blocks.  Counted, scanned
// and scattered in the style of mfx_regions.hip; no atomic orders anything, so the records come out the same on every run:
//   tile     one wave per tile, lane = word: the tile's markers and its last marker (position, haplotype), flagged at a contig's first tile
//   scan     exclusive sums of the markers (their ranks); the carry scan (mfx_ph_join: the last marker of the contig in front of each tile)
//   count    the same waves: a word's run starts, given the marker in front of it (the lanes in front, else the tile's carry)
//   scatter  every run's contig, haplotype, first marker and rank; the marker in front of a start ends the run in front of it, a contig's last
//            marker ends the contig's last run
//   runs     a run's markers (a difference of ranks), long or short, its A and B markers; the carry scan over the runs (the haplotype of the
//            nearest earlier long run), two exclusive sums
//   heads    a run opens a block by mfx_ph_head; scan; bounds (mfx_k_rg_bounds); emit
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "mfx_internal.h"
#include "mfx_kernels.h"
#include "mfx_phase.h"

static_assert(MFX_RG_TILE == MFX_TILE && MFX_RG_WORDS == 64, "mfx_phase.h: a tile's words are one wave, lane = word");

namespace {
constexpr uint32_t WAVES = MFX_BLOCK / 64;

struct JoinOp {
  __host__ __device__ __forceinline__ uint64_t operator()(const uint64_t &a, const uint64_t &b) const { return mfx_ph_join(a, b); }
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return __shfl(x, 0, 64);                                    // every lane holds the wave's sum
}
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t x) {      // sum of the lanes in front
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t s = x;
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)s, off, 64);
    if (lane >= off) s += y;
  }
  return s - x;
}
// the last non-empty value of the lanes up to and including this one (no lane of a tile is a contig's first but lane 0: no reset inside)
__device__ __forceinline__ uint64_t wave_last_inclusive(uint64_t x) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const uint64_t y = __shfl_up(x, off, 64);
    if (lane >= off) x = mfx_ph_join(y, x);
  }
  return x;
}
// the marker in front of this lane's word: the lanes in front, else the tile's carry
__device__ __forceinline__ uint64_t wave_prev(uint64_t own_last, uint64_t tile_in) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t incl = wave_last_inclusive(own_last);
  const uint64_t up = __shfl_up(incl, 1, 64);
  return mfx_ph_join(tile_in, lane == 0u ? 0ull : up);
}
__device__ __forceinline__ bool first_tile(const uint32_t *tile_contig, uint64_t t) { return t == 0 || tile_contig[t - 1] != tile_contig[t]; }
__device__ __forceinline__ uint64_t tile_carry_in(const uint32_t *tile_contig, const uint64_t *car, uint64_t t) {
  return first_tile(tile_contig, t) ? 0ull : mfx_ph_value(car[t - 1]);
}

__global__ __launch_bounds__(MFX_BLOCK) void mfx_ph_tile_kernel(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig,
                                                                uint64_t *cnt, uint64_t *car) {
  const uint64_t nw = ntiles * MFX_RG_WORDS;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t t = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t <= ntiles; t += (uint64_t)gridDim.x * WAVES) {      // wave-uniform
    if (t == ntiles) { if (lane == 0u) cnt[t] = 0ull; continue; }      // the scan's last entry: the total
    const uint64_t i = t * MFX_RG_WORDS + lane;
    const uint64_t h = planes[nw + i], m = planes[i] | h;
    const uint64_t n = wave_sum((uint64_t)__popcll(m));
    const uint64_t last = wave_last_inclusive(mfx_ph_word_last(m, h, mfx_rg_position(tile_start, tile_contig[t], i, 0)));
    if (lane == 63u) {
      cnt[t] = n;
      car[t] = (first_tile(tile_contig, t) ? MFX_PH_RESET : 0ull) | last;
    }
  }
}

__global__ __launch_bounds__(MFX_BLOCK) void mfx_ph_count_kernel(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig,
                                                                 const uint64_t *car, uint64_t *cnt_run) {
  const uint64_t nw = ntiles * MFX_RG_WORDS;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t t = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t <= ntiles; t += (uint64_t)gridDim.x * WAVES) {
    if (t == ntiles) { if (lane == 0u) cnt_run[t] = 0ull; continue; }
    const uint64_t i = t * MFX_RG_WORDS + lane;
    const uint64_t h = planes[nw + i], m = planes[i] | h;
    const uint64_t prev = wave_prev(mfx_ph_word_last(m, h, mfx_rg_position(tile_start, tile_contig[t], i, 0)), tile_carry_in(tile_contig, car, t));
    const uint64_t n = wave_sum((uint64_t)__popcll(mfx_ph_starts(m, h, prev)));
    if (lane == 0u) cnt_run[t] = n;
  }
}

__global__ __launch_bounds__(MFX_BLOCK) void mfx_ph_scatter_kernel(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig,
                                                                   const uint64_t *car, const uint64_t *rank0, const uint64_t *off, uint32_t *run_contig,
                                                                   uint32_t *run_hap, uint64_t *run_start, uint64_t *run_end, uint64_t *run_rank) {
  const uint64_t nw = ntiles * MFX_RG_WORDS;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t t = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < ntiles; t += (uint64_t)gridDim.x * WAVES) {
    const uint32_t c = tile_contig[t];
    const uint64_t i = t * MFX_RG_WORDS + lane;
    const uint64_t h = planes[nw + i], m = planes[i] | h;
    const uint64_t pos0 = mfx_rg_position(tile_start, c, i, 0);
    const uint64_t prev = wave_prev(mfx_ph_word_last(m, h, pos0), tile_carry_in(tile_contig, car, t));
    uint64_t s = mfx_ph_starts(m, h, prev);
    uint64_t at = off[t] + wave_exclusive((uint32_t)__popcll(s));
    const uint64_t rank = rank0[t] + wave_exclusive((uint32_t)__popcll(m));
    while (s) {
      const uint32_t b = mfx_rg_pop_bit(s);
      run_contig[at] = c;
      run_hap[at] = (uint32_t)((h >> b) & 1ull);
      run_start[at] = pos0 + b;
      run_rank[at] = rank + mfx_ph_below(m, b);
      const uint64_t before = mfx_ph_before(m, h, b, pos0, prev);
      if (before) run_end[at - 1] = mfx_ph_mark_pos(before) + 1ull;      // (a marker in front of it in this contig: a run is listed in front of this one)
      ++at;
    }
    const bool last_tile = t + 1 == ntiles || tile_contig[t + 1] != c;
    if (lane == 0u && last_tile && mfx_ph_value(car[t])) run_end[off[t + 1] - 1ull] = mfx_ph_mark_pos(mfx_ph_value(car[t])) + 1ull;
  }
}

__global__ __launch_bounds__(MFX_BLOCK) void mfx_ph_runs_kernel(const uint32_t *run_contig, const uint32_t *run_hap, const uint64_t *run_start, const uint64_t *run_end,
                                                                const uint64_t *run_rank, uint64_t nruns, uint64_t nmarkers, uint64_t k, uint64_t S, uint64_t R,
                                                                uint64_t *lng, uint64_t *cnt_a, uint64_t *cnt_b) {
  const uint64_t stride = (uint64_t)gridDim.x * MFX_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * MFX_BLOCK + threadIdx.x; i <= nruns; i += stride) {
    if (i == nruns) { cnt_a[i] = 0ull; cnt_b[i] = 0ull; continue; }      // the scans' last entry: the totals
    const uint64_t n = (i + 1 < nruns ? run_rank[i + 1] : nmarkers) - run_rank[i];
    const bool first = i == 0 || run_contig[i - 1] != run_contig[i];
    const bool is_long = mfx_ph_long(n, run_start[i], run_end[i], k, S, R);
    lng[i] = (first ? MFX_PH_RESET : 0ull) | (is_long ? (uint64_t)run_hap[i] + 1ull : 0ull);
    cnt_a[i] = run_hap[i] == 0u ? n : 0ull;
    cnt_b[i] = run_hap[i] == 1u ? n : 0ull;
  }
}

// lng: a run's own element; lng_x: the inclusive carry scan of them
__global__ __launch_bounds__(MFX_BLOCK) void mfx_ph_heads_kernel(const uint32_t *run_contig, const uint32_t *run_hap, const uint64_t *lng, const uint64_t *lng_x,
                                                                 uint64_t nruns, uint64_t *head) {
  const uint64_t stride = (uint64_t)gridDim.x * MFX_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * MFX_BLOCK + threadIdx.x; i <= nruns; i += stride) {
    if (i == nruns) { head[i] = 0ull; continue; }
    const bool first = i == 0 || run_contig[i - 1] != run_contig[i];
    head[i] = mfx_ph_head(first, mfx_ph_value(lng[i]) != 0ull, run_hap[i], first ? 0ull : mfx_ph_value(lng_x[i - 1])) ? 1ull : 0ull;
  }
}

__global__ __launch_bounds__(MFX_BLOCK) void mfx_ph_emit_kernel(const uint64_t *blk_first, const uint64_t *blk_last, uint64_t nblocks, const uint32_t *run_contig,
                                                                const uint32_t *run_hap, const uint64_t *run_start, const uint64_t *run_end, const uint64_t *lng_x,
                                                                const uint64_t *a_x, const uint64_t *b_x, uint64_t *recs) {
  const uint64_t stride = (uint64_t)gridDim.x * MFX_BLOCK;
  for (uint64_t r = (uint64_t)blockIdx.x * MFX_BLOCK + threadIdx.x; r < nblocks; r += stride) {
    const uint64_t f = blk_first[r], l = blk_last[r];
    const uint64_t nA = a_x[l + 1] - a_x[f], nB = b_x[l + 1] - b_x[f];
    const uint32_t hap = mfx_ph_block_hap(mfx_ph_value(lng_x[l]), nA, nB);
    uint64_t *o = recs + r * MFX_PH_REC_WORDS;
    o[0] = (uint64_t)run_contig[f] | ((uint64_t)hap << 32);
    o[1] = run_start[f];
    o[2] = run_end[l];
    o[3] = hap ? nB : nA;
    o[4] = hap ? nA : nB;
    o[5] = mfx_ph_other_runs(l - f + 1ull, run_hap[f], hap);
  }
}

unsigned grid_for(uint64_t items, uint64_t per_block) {
  const uint64_t b = (items + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : b < 8192 ? b : 8192);
}
}  // namespace

// the carry scan works in the caller's temporary storage (mfx_k_ph_temp_bytes of the largest n it will pass) and waits for nothing
size_t mfx_k_ph_temp_bytes(uint64_t n) {
  size_t a = 0;
  uint64_t *x = nullptr;
  (void)hipcub::DeviceScan::InclusiveScan(nullptr, a, x, x, JoinOp(), (size_t)(n ? n : 1), (hipStream_t) nullptr);
  const size_t b = mfx_k_rg_temp_bytes(n);
  return (a > b ? a : b) + 256;
}
hipError_t mfx_k_ph_join_scan(const uint64_t *in, uint64_t *out, uint64_t n, void *tmp, size_t tmp_bytes, hipStream_t st) {
  if (n == 0) return hipSuccess;
  size_t bytes = 0;
  hipError_t e = hipcub::DeviceScan::InclusiveScan(nullptr, bytes, in, out, JoinOp(), (size_t)n, st);
  if (e != hipSuccess) return e;
  if (bytes > tmp_bytes) return hipErrorInvalidValue;
  return hipcub::DeviceScan::InclusiveScan(tmp, bytes, in, out, JoinOp(), (size_t)n, st);
}
hipError_t mfx_k_ph_tile(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig, uint64_t *cnt, uint64_t *car, hipStream_t st) {
  mfx_ph_tile_kernel<<<grid_for(ntiles + 1, WAVES), MFX_BLOCK, 0, st>>>(planes, ntiles, tile_start, tile_contig, cnt, car);
  return hipGetLastError();
}
hipError_t mfx_k_ph_count(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig, const uint64_t *car, uint64_t *cnt_run,
                          hipStream_t st) {
  mfx_ph_count_kernel<<<grid_for(ntiles + 1, WAVES), MFX_BLOCK, 0, st>>>(planes, ntiles, tile_start, tile_contig, car, cnt_run);
  return hipGetLastError();
}
hipError_t mfx_k_ph_scatter(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig, const uint64_t *car, const uint64_t *rank0,
                            const uint64_t *off, uint32_t *run_contig, uint32_t *run_hap, uint64_t *run_start, uint64_t *run_end, uint64_t *run_rank, hipStream_t st) {
  if (ntiles == 0) return hipSuccess;
  mfx_ph_scatter_kernel<<<grid_for(ntiles, WAVES), MFX_BLOCK, 0, st>>>(planes, ntiles, tile_start, tile_contig, car, rank0, off, run_contig, run_hap, run_start, run_end,
                                                                       run_rank);
  return hipGetLastError();
}
hipError_t mfx_k_ph_runs(const uint32_t *run_contig, const uint32_t *run_hap, const uint64_t *run_start, const uint64_t *run_end, const uint64_t *run_rank, uint64_t nruns,
                         uint64_t nmarkers, uint64_t k, uint64_t S, uint64_t R, uint64_t *lng, uint64_t *cnt_a, uint64_t *cnt_b, hipStream_t st) {
  mfx_ph_runs_kernel<<<grid_for(nruns + 1, MFX_BLOCK), MFX_BLOCK, 0, st>>>(run_contig, run_hap, run_start, run_end, run_rank, nruns, nmarkers, k, S, R, lng, cnt_a, cnt_b);
  return hipGetLastError();
}
hipError_t mfx_k_ph_heads(const uint32_t *run_contig, const uint32_t *run_hap, const uint64_t *lng, const uint64_t *lng_x, uint64_t nruns, uint64_t *head, hipStream_t st) {
  mfx_ph_heads_kernel<<<grid_for(nruns + 1, MFX_BLOCK), MFX_BLOCK, 0, st>>>(run_contig, run_hap, lng, lng_x, nruns, head);
  return hipGetLastError();
}
hipError_t mfx_k_ph_emit(const uint64_t *blk_first, const uint64_t *blk_last, uint64_t nblocks, const uint32_t *run_contig, const uint32_t *run_hap,
                         const uint64_t *run_start, const uint64_t *run_end, const uint64_t *lng_x, const uint64_t *a_x, const uint64_t *b_x, uint64_t *recs, hipStream_t st) {
  if (nblocks == 0) return hipSuccess;
  mfx_ph_emit_kernel<<<grid_for(nblocks, MFX_BLOCK), MFX_BLOCK, 0, st>>>(blk_first, blk_last, nblocks, run_contig, run_hap, run_start, run_end, lng_x, a_x, b_x, recs);
  return hipGetLastError();
}
