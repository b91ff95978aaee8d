// mfx_diploid.hip -- the device part of mfx_db_diploid (mfx_db.cpp; the rule: mfx_diploid.h): two haplotype assemblies against the reads in
// one windowed pass that ends in reductions.  The windows, the block decode, the role tag (mfx_trio_tag_kernel) and the pairwise merge
// (mfx_merge_pairs_kernel) are what they were.  New here, per window:
//
//   a. mfx_dip_pairs_kernel: the tagged merged run of hap1 and hap2 into the PAIR RUN, one record (k-mer, c1 | c2 << 32) per k-mer, ascending
//      and dense.  mfx_combine_kernel's shape with one output: a count run over tiles of MFX_DIP_TILE positions, one tile scan, a scatter run
//      that computes the same again and stores.  No atomic orders anything: a second run gives the same bytes.
//   b. mfx_join_kernel (mfx_join_device.h) with mfx_dip_consumer: the merge-path walk of the read run against the pair run, the asm value 64
//      bits wide.  The read run is read once and never rewritten; only the assemblies went through the merge.
//
// The consumer's reductions, all exact integer adds or fp64 sums of integers (the order takes no part):
//   the class image and the cn image through mfx_spectrum.h's bins, as two row blocks of ONE array of 32-bit LDS bins (the class image's 4
//     rows in front, the cn image's copies + 2 behind), columns below L = mfx_dip_lds_cols in LDS and flushed once per workgroup, the others
//     by 64-bit global atomics; MFX_SPECTRUM_AGG's aggregated form is honoured (every lane of a wave calls in every turn);
//   the 18 counters (mfx_diploid.h) in registers, reduced per wave, then per workgroup in LDS, then one 64-bit add per workgroup and counter
//     into the workgroup's copy of the counter lines (MFX_DIP_STAT_SHARDS copies);
//   with a peak: one tot[64] and three und[64] piece sums in LDS as mfx_join_completeness keeps them, and its readK table.
//
// LDS and occupancy (160 KB a CU, workgroups of 256 lanes = one wave per SIMD), all static:
//   the tile 32 KB (16 KB of k-mers, 16 KB of 64-bit values) + 32 KB bins + 8 KB readK table + 2 KB piece sums + 576 B counters + the cuts
//   = 74.6 KB: two workgroups a CU, two waves a SIMD (as the -spectrum join).
// No 32-bit LDS bin can wrap: a workgroup adds at most one to one bin of each image per pair it owns, and a launch holds la + lb < 2^32
// merged positions (mfx_join_launch refuses more).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfx_device.h"
#include "mfx_diploid.h"
#include "mfx_join_device.h"
#include "mfx_kernels.h"
#include "mfx_kstar.h"
#include "mfx_spectrum.h"

// ---------------------------------------------------------------------------
// a. the pair run
// ---------------------------------------------------------------------------
constexpr uint32_t MFX_DIP_ROUNDS = 8;
constexpr uint32_t MFX_DIP_TILE = 256u * MFX_DIP_ROUNDS;

template <bool SCATTER>
__global__ __launch_bounds__(256) void mfx_dip_pairs_kernel(const uint64_t *keys, const uint32_t *vals, uint64_t n, uint64_t *tile_off, uint64_t *pk, uint64_t *pv) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t tid = threadIdx.x, wv = tid >> 6, ln = tid & 63u;
  uint64_t base = SCATTER ? tile_off[blockIdx.x] : 0ull;
  for (uint32_t r = 0; r < MFX_DIP_ROUNDS; ++r) {              // (uniform)
    const uint64_t i = (uint64_t)blockIdx.x * MFX_DIP_TILE + (uint64_t)r * 256u + tid;
    const bool head = i < n && mfx_trio_head(keys, i);
    const unsigned long long m = __ballot(head);
    if (ln == 0u) s_cnt[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0u, total = 0u;
    for (uint32_t w = 0; w < 4u; ++w) { const uint32_t x = s_cnt[w]; total += x; if (w < wv) before += x; }
    if (SCATTER && head) {
      const uint64_t at = base + before + (uint32_t)__popcll(m & ((1ull << ln) - 1ull));      // (at <= i < n: a head per position at the most)
      pk[at] = mfx_trio_kmer(keys[i]);
      pv[at] = mfx_dip_gather(keys, vals, n, i);
    }
    base += total;
    __syncthreads();                                           // (s_cnt is written again in the next round)
  }
  if (!SCATTER && tid == 0u) tile_off[blockIdx.x] = base;
}

// t[0 .. n) -> their exclusive prefix sums, t[n] = the total; one workgroup (mfx_tile_scan_kernel, mfx_merge.hip)
__global__ __launch_bounds__(256) void mfx_dip_tile_scan_kernel(uint64_t *t, uint32_t n) {
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

uint64_t mfx_dip_tiles(uint64_t n) { return (n + MFX_DIP_TILE - 1) / MFX_DIP_TILE; }

// tile_off: mfx_dip_tiles(n) + 1 words; the records of the pair run are its last word when the stream has run.  pk, pv: room for n records.
hipError_t mfx_k_dip_pairs(const uint64_t *keys, const uint32_t *vals, uint64_t n, uint64_t *tile_off, uint64_t *pk, uint64_t *pv, hipStream_t st) {
  const uint64_t tiles = mfx_dip_tiles(n);
  if (tiles == 0) return hipSuccess;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  mfx_dip_pairs_kernel<false><<<(unsigned)tiles, 256, 0, st>>>(keys, vals, n, tile_off, pk, pv);
  mfx_dip_tile_scan_kernel<<<1, 256, 0, st>>>(tile_off, (uint32_t)tiles);
  mfx_dip_pairs_kernel<true><<<(unsigned)tiles, 256, 0, st>>>(keys, vals, n, tile_off, pk, pv);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// b. the join's consumer
// ---------------------------------------------------------------------------
template <bool AGG>
struct mfx_dip_consumer {
  typedef uint64_t asm_t;
  static constexpr uint32_t NLUT = 1024;                       // readK per common read count, as in mfx_join_completeness
  struct lds {
    uint32_t bins[MFX_DIP_LDS_WORDS];
    double rk[NLUT], tot[64], und[3][64];
    unsigned long long st[4][MFX_DIP_NSTATS];
  };
  mfx_spectrum_args cls, cn;                                   // the class image (copies = 2: its 4 rows) and the cn image; one lds_cols
  uint64_t minV, maxV;
  int pieces, pshift;
  double peak;
  uint32_t n_prob;
  const uint32_t *probK;
  const double *probP;
  double *sums;                                                // [256]: tot[64], und[3][64]
  unsigned long long *counters;                                // MFX_DIP_STAT_WORDS
  uint64_t counted_cls, counted_cn;
  uint64_t st[MFX_DIP_NSTATS];

  __device__ __forceinline__ uint32_t *cn_bins(lds &s) const { return s.bins + MFX_DIP_ROWS * cls.lds_cols; }
  __device__ __forceinline__ void begin(lds &s) {
    counted_cls = counted_cn = 0;
#pragma unroll
    for (uint32_t i = 0; i < MFX_DIP_NSTATS; ++i) st[i] = 0;
    if (threadIdx.x < 64) { s.tot[threadIdx.x] = 0.0; s.und[0][threadIdx.x] = 0.0; s.und[1][threadIdx.x] = 0.0; s.und[2][threadIdx.x] = 0.0; }
    if (pieces)
      for (uint32_t v = threadIdx.x; v < NLUT; v += blockDim.x) {
        double rk, pr;
        mfx_getK_core(peak, n_prob, probK, probP, v, rk, pr);
        s.rk[v] = rk;
      }
    mfx_spec_begin(cls, s.bins);
    mfx_spec_begin(cn, cn_bins(s));
  }
  __device__ __forceinline__ void pair(lds &s, bool have, uint64_t key, uint32_t rv, uint64_t av) {
    const uint32_t r = have ? rv : 0u;                         // (a lane without a pair adds zeros)
    const mfx_dip_class k = mfx_dip_rule(r, have ? av : 0ull, minV, maxV);
    mfx_dip_count(st, r, k);
    counted_cls += mfx_spec_count<AGG>(cls, s.bins, have, k.rf, k.row);
    counted_cn += mfx_spec_count<AGG>(cn, cn_bins(s), have, k.rf, k.cb);
    if (pieces && r != 0u) {                                   // an asm-only k-mer takes no part (merfin-completeness.C:106-109)
      double readK, prob;
      if (r < NLUT) readK = s.rk[r];
      else mfx_getK_core(peak, n_prob, probK, probP, r, readK, prob);
      const uint32_t piece = (uint32_t)(key >> pshift) & 63u;
      atomicAdd(&s.tot[piece], readK);
      const double u1 = mfx_dip_under(readK, k.c1), u2 = mfx_dip_under(readK, k.c2), ub = mfx_dip_under(readK, k.cb);
      if (u1 != 0.0) atomicAdd(&s.und[0][piece], u1);
      if (u2 != 0.0) atomicAdd(&s.und[1][piece], u2);
      if (ub != 0.0) atomicAdd(&s.und[2][piece], ub);
    }
  }
  __device__ __forceinline__ void end(lds &s) {
    mfx_spec_end(cls, s.bins, counted_cls);
    mfx_spec_end(cn, cn_bins(s), counted_cn);
    const uint32_t tid = threadIdx.x, wv = tid >> 6, ln = tid & 63u;
#pragma unroll
    for (uint32_t i = 0; i < MFX_DIP_NSTATS; ++i) {
      unsigned long long x = st[i];
      for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
      if (ln == 0u) s.st[wv][i] = x;
    }
    __syncthreads();                                           // (the piece sums are complete as well: mfx_spec_end has synchronised twice)
    if (tid < MFX_DIP_NSTATS) {
      const unsigned long long x = s.st[0][tid] + s.st[1][tid] + s.st[2][tid] + s.st[3][tid];
      if (x) atomicAdd(&counters[(blockIdx.x % MFX_DIP_STAT_SHARDS) * MFX_DIP_STAT_STRIDE + tid], x);
    }
    if (pieces && tid < 64u) {
      if (s.tot[tid] != 0.0) atomicAdd(&sums[tid], s.tot[tid]);
#pragma unroll
      for (uint32_t x = 0; x < 3u; ++x)
        if (s.und[x][tid] != 0.0) atomicAdd(&sums[64u * (x + 1u) + tid], s.und[x][tid]);
    }
  }
};

// the read run a against the pair run (pk, pv), both strictly ascending.  cls / cn: the two images (cls.copies == 2, one lds_cols, each with its
// counter word behind it), added to; sums[256] (pieces != 0) and counters[MFX_DIP_STAT_WORDS] added to; stats[0] += the k-mers both runs hold
hipError_t mfx_k_dip_join(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *pk, const uint64_t *pv, uint64_t lb, const mfx_spectrum_args &cls,
                          const mfx_spectrum_args &cn, uint64_t minV, uint64_t maxV, int k, int pieces, double peak, uint32_t n_prob, const uint32_t *probK,
                          const double *probP, double *sums, uint64_t *counters, uint64_t *stats, int grid, hipStream_t st) {
  if (cls.copies != 2u || cls.lds_cols != cn.lds_cols || cls.max_mult != cn.max_mult || cls.aggregate != cn.aggregate ||
      (uint64_t)(MFX_DIP_ROWS + cn.copies + 2u) * cn.lds_cols > MFX_DIP_LDS_WORDS)
    return hipErrorInvalidValue;                               // (the two row blocks fit the bins)
  auto fill = [&](auto &c) {
    c.cls = cls; c.cn = cn; c.minV = minV; c.maxV = maxV; c.pieces = pieces; c.pshift = mfx_dip_pshift(k);
    c.peak = peak; c.n_prob = n_prob; c.probK = probK; c.probP = probP; c.sums = sums;
    c.counters = reinterpret_cast<unsigned long long *>(counters);
  };
  if (cn.aggregate) {
    mfx_dip_consumer<true> c;
    fill(c);
    return mfx_join_launch(ka, va, la, pk, pv, lb, c, stats, grid, st);
  }
  mfx_dip_consumer<false> c;
  fill(c);
  return mfx_join_launch(ka, va, la, pk, pv, lb, c, stats, grid, st);
}
