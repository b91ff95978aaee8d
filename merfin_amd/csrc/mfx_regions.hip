// mfx_regions.hip -- the steps of -regions between its two evaluation passes (csrc/mfx_regions.h): class planes -> elementary runs ->
// regions.  Everything is counted, scanned and scattered; no atomic orders anything, so the lists come out the same on every run:
//   count    one wave per (class, tile): its 64 words' run starts and run ends (mfx_rg_starts / mfx_rg_ends), added over the wave
//   scan     exclusive sums of the counts (hipCUB, in the caller's temporary storage): where each (class, tile) writes, and how many runs
//            there are; the totals the host needs are picked into one small array and copied once a stage
//   scatter  the same waves again: every start and every end to its place -- runs in (class, contig, start) order, the i-th start
//            pairing with the i-th end
//   heads    a run opens a region by mfx_rg_head; scan: the region of every run
//   bounds   first and last run of every region; keep: its k-mers (a difference of the scanned run lengths) against -minrun; scan;
//   emit     the kept regions as mfx_region records, their sums 0 for pass 2
//   finish   after pass 2: the key of the extreme K* -> the double
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "mfx_internal.h"
#include "mfx_kernels.h"
#define MFX_REGIONS_DEVICE
#include "mfx_regions.h"

static_assert(MFX_RG_TILE == MFX_TILE, "mfx_regions.h restates the tile");

namespace {
constexpr uint32_t WAVES = MFX_BLOCK / 64;

__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;                                                   // lane 0 holds the wave's sum
}
__device__ __forceinline__ uint64_t wave_exclusive(uint32_t x) {      // sum of the lanes in front
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t s = x;
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)s, off, 64);
    if (lane >= off) s += y;
  }
  return s - x;
}

__global__ __launch_bounds__(MFX_BLOCK) void mfx_rg_count_kernel(const uint64_t *planes, uint64_t ntiles, const uint32_t *tile_contig, uint64_t *cnt_s,
                                                                 uint64_t *cnt_e, uint64_t *tile_flag) {
  const uint64_t nw = ntiles * MFX_RG_WORDS, nct = ntiles * MFX_RG_CLASSES;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t ct = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); ct < nct; ct += (uint64_t)gridDim.x * WAVES) {      // wave-uniform
    const uint64_t *plane = planes + (ct / ntiles) * nw;
    const uint64_t i = (ct % ntiles) * MFX_RG_WORDS + lane;
    const uint64_t w = plane[i];
    const uint64_t ns = wave_sum((uint64_t)__popcll(mfx_rg_starts(w, mfx_rg_prev_msb(plane, tile_contig, i))));
    const uint64_t ne = wave_sum((uint64_t)__popcll(mfx_rg_ends(w, mfx_rg_next_lsb(plane, tile_contig, nw, i))));
    const bool any = __any(w != 0ull);
    if (lane == 0u) {
      cnt_s[ct] = ns;
      cnt_e[ct] = ne;
      if (any) tile_flag[ct % ntiles] = 1ull;                 // (up to three waves store the same value)
    }
  }
}

__global__ __launch_bounds__(MFX_BLOCK) void mfx_rg_scatter_kernel(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig,
                                                                   const uint64_t *off_s, const uint64_t *off_e, uint32_t *run_contig, uint64_t *run_start,
                                                                   uint64_t *run_end) {
  const uint64_t nw = ntiles * MFX_RG_WORDS, nct = ntiles * MFX_RG_CLASSES;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t ct = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); ct < nct; ct += (uint64_t)gridDim.x * WAVES) {
    const uint64_t *plane = planes + (ct / ntiles) * nw;
    const uint32_t c = tile_contig[ct % ntiles];
    const uint64_t i = (ct % ntiles) * MFX_RG_WORDS + lane;
    const uint64_t w = plane[i];
    uint64_t s = mfx_rg_starts(w, mfx_rg_prev_msb(plane, tile_contig, i));
    uint64_t e = mfx_rg_ends(w, mfx_rg_next_lsb(plane, tile_contig, nw, i));
    uint64_t is = off_s[ct] + wave_exclusive((uint32_t)__popcll(s));
    uint64_t ie = off_e[ct] + wave_exclusive((uint32_t)__popcll(e));
    while (s) { run_contig[is] = c; run_start[is++] = mfx_rg_position(tile_start, c, i, mfx_rg_pop_bit(s)); }
    while (e) run_end[ie++] = mfx_rg_position(tile_start, c, i, mfx_rg_pop_bit(e)) + 1ull;
  }
}

struct ClsRuns { uint64_t at[MFX_RG_CLASSES + 1]; };          // class c's runs: [at[c], at[c + 1])

__global__ __launch_bounds__(MFX_BLOCK) void mfx_rg_heads_kernel(const uint32_t *run_contig, const uint64_t *run_start, const uint64_t *run_end, uint64_t nruns,
                                                                 ClsRuns cr, uint64_t gap, uint64_t *head, uint64_t *len) {
  const uint64_t stride = (uint64_t)gridDim.x * MFX_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * MFX_BLOCK + threadIdx.x; i <= nruns; i += stride) {
    if (i == nruns) { head[i] = 0ull; len[i] = 0ull; continue; }      // the scans' last entry: the totals
    const bool first = i == cr.at[0] || i == cr.at[1] || i == cr.at[2];
    head[i] = mfx_rg_head(first, first ? 0u : run_contig[i - 1], first ? 0ull : run_end[i - 1], run_contig[i], run_start[i], gap) ? 1ull : 0ull;
    len[i] = run_end[i] - run_start[i];
  }
}

// head_x: the exclusive scan of the heads, nruns + 1 entries -- run i is a head when head_x[i + 1] != head_x[i], its region is head_x[i + 1] - 1
__global__ __launch_bounds__(MFX_BLOCK) void mfx_rg_bounds_kernel(const uint64_t *head_x, uint64_t nruns, uint64_t *reg_first, uint64_t *reg_last) {
  const uint64_t stride = (uint64_t)gridDim.x * MFX_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * MFX_BLOCK + threadIdx.x; i < nruns; i += stride) {
    const uint64_t r = head_x[i + 1] - 1ull;
    if (head_x[i + 1] != head_x[i]) reg_first[r] = i;
    if (i + 1 == nruns || head_x[i + 2] != head_x[i + 1]) reg_last[r] = i;
  }
}

__global__ __launch_bounds__(MFX_BLOCK) void mfx_rg_keep_kernel(const uint64_t *reg_first, const uint64_t *reg_last, const uint64_t *len_x, uint64_t nraw,
                                                                uint64_t min_kmers, uint64_t *keep) {
  const uint64_t stride = (uint64_t)gridDim.x * MFX_BLOCK;
  for (uint64_t r = (uint64_t)blockIdx.x * MFX_BLOCK + threadIdx.x; r <= nraw; r += stride)
    keep[r] = (r < nraw && len_x[reg_last[r] + 1] - len_x[reg_first[r]] >= min_kmers) ? 1ull : 0ull;
}

__global__ __launch_bounds__(MFX_BLOCK) void mfx_rg_emit_kernel(const uint64_t *reg_first, const uint64_t *reg_last, const uint64_t *len_x, const uint64_t *keep_x,
                                                                uint64_t nraw, ClsRuns cr, const uint32_t *run_contig, const uint64_t *run_start,
                                                                const uint64_t *run_end, uint64_t *regs) {
  const uint64_t stride = (uint64_t)gridDim.x * MFX_BLOCK;
  for (uint64_t r = (uint64_t)blockIdx.x * MFX_BLOCK + threadIdx.x; r < nraw; r += stride) {
    if (keep_x[r + 1] == keep_x[r]) continue;
    const uint64_t f = reg_first[r], l = reg_last[r];
    const uint64_t cls = f >= cr.at[2] ? 2ull : f >= cr.at[1] ? 1ull : 0ull;
    uint64_t *o = regs + keep_x[r] * MFX_RG_REC_WORDS;
    o[0] = (uint64_t)run_contig[f] | (cls << 32);
    o[1] = run_start[f];
    o[2] = run_end[l];
    o[3] = len_x[l + 1] - len_x[f];
    o[4] = 0ull; o[5] = 0ull; o[6] = 0ull;
  }
}

__global__ __launch_bounds__(MFX_BLOCK) void mfx_rg_finish_kernel(uint64_t *regs, uint64_t nreg) {
  const uint64_t stride = (uint64_t)gridDim.x * MFX_BLOCK;
  for (uint64_t r = (uint64_t)blockIdx.x * MFX_BLOCK + threadIdx.x; r < nreg; r += stride) {
    uint64_t *o = regs + r * MFX_RG_REC_WORDS;
    const uint32_t cls = (uint32_t)(o[0] >> 32);
    const double x = cls == MFX_REGION_COLLAPSED ? mfx_trk_unkey(o[6]) : cls == MFX_REGION_EXPANDED ? mfx_trk_unkey(~o[6]) : 0.0;
    o[6] = (uint64_t)__double_as_longlong(x);
  }
}

// dst[i] = src[idx[i]]: the few totals the host needs of a scanned array, put side by side for one copy
struct Picks { uint64_t at[4]; };
__global__ void mfx_rg_pick_kernel(const uint64_t *src, Picks pk, uint32_t n, uint64_t *dst) {
  if (threadIdx.x < n) dst[threadIdx.x] = src[pk.at[threadIdx.x]];
}

unsigned grid_for(uint64_t items, uint64_t per_block) {
  const uint64_t b = (items + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : b < 8192 ? b : 8192);
}
}  // namespace

// the scans and the sum work in the caller's temporary storage (mfx_k_rg_temp_bytes of the largest n it will pass) and wait for nothing
size_t mfx_k_rg_temp_bytes(uint64_t n) {
  size_t a = 0, b = 0;
  uint64_t *x = nullptr;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, x, x, (size_t)(n ? n : 1), (hipStream_t) nullptr);
  (void)hipcub::DeviceReduce::Sum(nullptr, b, x, x, (size_t)(n ? n : 1), (hipStream_t) nullptr);
  return (a > b ? a : b) + 256;
}
hipError_t mfx_k_rg_scan(uint64_t *d, uint64_t n, void *tmp, size_t tmp_bytes, hipStream_t st) {
  if (n == 0) return hipSuccess;
  size_t bytes = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d, d, (size_t)n, st);
  if (e != hipSuccess) return e;
  if (bytes > tmp_bytes) return hipErrorInvalidValue;
  return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, d, d, (size_t)n, st);
}
hipError_t mfx_k_rg_sum(const uint64_t *d, uint64_t n, uint64_t *out, void *tmp, size_t tmp_bytes, hipStream_t st) {
  if (n == 0) return hipMemsetAsync(out, 0, sizeof(uint64_t), st);
  size_t bytes = 0;
  hipError_t e = hipcub::DeviceReduce::Sum(nullptr, bytes, d, out, (size_t)n, st);
  if (e != hipSuccess) return e;
  if (bytes > tmp_bytes) return hipErrorInvalidValue;
  return hipcub::DeviceReduce::Sum(tmp, bytes, d, out, (size_t)n, st);
}
hipError_t mfx_k_rg_pick(const uint64_t *src, const uint64_t *idx, uint32_t n, uint64_t *dst, hipStream_t st) {
  Picks pk;
  if (n > 4) return hipErrorInvalidValue;
  for (uint32_t i = 0; i < 4; ++i) pk.at[i] = i < n ? idx[i] : 0;
  mfx_rg_pick_kernel<<<1, 64, 0, st>>>(src, pk, n, dst);
  return hipGetLastError();
}

hipError_t mfx_k_rg_count(const uint64_t *planes, uint64_t ntiles, const uint32_t *tile_contig, uint64_t *cnt_s, uint64_t *cnt_e, uint64_t *tile_flag, hipStream_t st) {
  if (ntiles == 0) return hipSuccess;
  mfx_rg_count_kernel<<<grid_for(ntiles * MFX_RG_CLASSES, WAVES), MFX_BLOCK, 0, st>>>(planes, ntiles, tile_contig, cnt_s, cnt_e, tile_flag);
  return hipGetLastError();
}
hipError_t mfx_k_rg_scatter(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig, const uint64_t *off_s,
                            const uint64_t *off_e, uint32_t *run_contig, uint64_t *run_start, uint64_t *run_end, hipStream_t st) {
  if (ntiles == 0) return hipSuccess;
  mfx_rg_scatter_kernel<<<grid_for(ntiles * MFX_RG_CLASSES, WAVES), MFX_BLOCK, 0, st>>>(planes, ntiles, tile_start, tile_contig, off_s, off_e, run_contig, run_start, run_end);
  return hipGetLastError();
}
hipError_t mfx_k_rg_heads(const uint32_t *run_contig, const uint64_t *run_start, const uint64_t *run_end, uint64_t nruns, const uint64_t *cls_run, uint64_t gap,
                          uint64_t *head, uint64_t *len, hipStream_t st) {
  ClsRuns cr;
  for (uint32_t c = 0; c <= MFX_RG_CLASSES; ++c) cr.at[c] = cls_run[c];
  mfx_rg_heads_kernel<<<grid_for(nruns + 1, MFX_BLOCK), MFX_BLOCK, 0, st>>>(run_contig, run_start, run_end, nruns, cr, gap, head, len);
  return hipGetLastError();
}
hipError_t mfx_k_rg_bounds(const uint64_t *head_x, uint64_t nruns, uint64_t *reg_first, uint64_t *reg_last, hipStream_t st) {
  if (nruns == 0) return hipSuccess;
  mfx_rg_bounds_kernel<<<grid_for(nruns, MFX_BLOCK), MFX_BLOCK, 0, st>>>(head_x, nruns, reg_first, reg_last);
  return hipGetLastError();
}
hipError_t mfx_k_rg_keep(const uint64_t *reg_first, const uint64_t *reg_last, const uint64_t *len_x, uint64_t nraw, uint64_t min_kmers, uint64_t *keep, hipStream_t st) {
  mfx_rg_keep_kernel<<<grid_for(nraw + 1, MFX_BLOCK), MFX_BLOCK, 0, st>>>(reg_first, reg_last, len_x, nraw, min_kmers, keep);
  return hipGetLastError();
}
hipError_t mfx_k_rg_emit(const uint64_t *reg_first, const uint64_t *reg_last, const uint64_t *len_x, const uint64_t *keep_x, uint64_t nraw, const uint64_t *cls_run,
                         const uint32_t *run_contig, const uint64_t *run_start, const uint64_t *run_end, uint64_t *regs, hipStream_t st) {
  if (nraw == 0) return hipSuccess;
  ClsRuns cr;
  for (uint32_t c = 0; c <= MFX_RG_CLASSES; ++c) cr.at[c] = cls_run[c];
  mfx_rg_emit_kernel<<<grid_for(nraw, MFX_BLOCK), MFX_BLOCK, 0, st>>>(reg_first, reg_last, len_x, keep_x, nraw, cr, run_contig, run_start, run_end, regs);
  return hipGetLastError();
}
hipError_t mfx_k_rg_finish(uint64_t *regs, uint64_t nreg, hipStream_t st) {
  if (nreg == 0) return hipSuccess;
  mfx_rg_finish_kernel<<<grid_for(nreg, MFX_BLOCK), MFX_BLOCK, 0, st>>>(regs, nreg);
  return hipGetLastError();
}
