// mfx_join.hip -- mfx_join_kernel: the sorted join of a window's read run and asm run (what mfx_delta_decode_kernel leaves of two sorted
// databases, mfx_db.cpp: mfx_db_join_*) that ends in a reduction: -completeness' 64 + 64 piece sums or the -spectrum image.  No hash table,
// no sort, no merged run: the 12 bytes of a record are read once and nothing is written back but the reduction.
//
// Tiling is mfx_merge_pairs_kernel's merge path (mfx_merge.hip).  A workgroup takes MFX_JOIN_TILE consecutive positions of the merged order
// at a time: two binary searches in global memory cut the runs (mfx_merge_cut), the two pieces are staged in LDS (24 KB: the k-mers and the
// counts of a tile), every lane finds its own diagonal's cut in LDS and walks MFX_JOIN_PER positions (mfx_join_lane, mfx_join.h: the walk
// the host restates) -- fully unrolled, its state in registers, no scratch.  The workgroups are persistent and stride over the tiles, so a
// consumer's LDS is set up and flushed once per workgroup, not once per tile.
//
// OWNERSHIP of a key that both runs hold (mfx_join.h has the rule in full): the lane whose share holds the READ record owns the pair and
// looks one asm record ahead in merged order, across its share's and its tile's end; a lane that holds an ASM record whose predecessor in
// merged order is the equal read record skips it.  The two records across a tile's ends are read from global memory into registers (the
// same address in every lane), not staged: the LDS of the walk is the merge kernel's.
//
// LDS and occupancy (160 KB a CU, workgroups of 256 lanes = one wave per SIMD):
//   completeness  24 KB + 8 KB readK table + 1 KB piece sums = 33 KB: four workgroups a CU, four waves a SIMD
//   spectrum      24 KB + 32 KB bins = 56 KB: two workgroups a CU, two waves a SIMD
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfx_device.h"
#include "mfx_join.h"
#include "mfx_join_device.h"                                   // mfx_join_kernel, mfx_join_launch
#include "mfx_kernels.h"
#include "mfx_kstar.h"
#include "mfx_spectrum.h"

// ---------------------------------------------------------------------------
// The consumers: begin (once per workgroup), pair (MFX_JOIN_PER times per lane and tile, every lane of a wave together), end.
// ---------------------------------------------------------------------------

// mfx_completeness_kernel's sums (mfx_kernels.hip; merfin-completeness.C:70-117) from the pair instead of a table slot: the raw read count
// (-min / -max do not apply there), asm-only k-mers skipped.  readK is an integer: the fp64 sums are exact in any order.
struct mfx_join_completeness {
  typedef uint32_t asm_t;
  static constexpr uint32_t NLUT = 1024;                       // readK per common read count, as in mfx_completeness_kernel
  struct lds { double rk[NLUT], tot[64], und[64]; };
  double peak;
  uint32_t n_prob;
  const uint32_t *probK;
  const double *probP;
  double *pieces;                                              // [128]: total[64], undrc[64]
  int pshift;                                                  // piece = top 6 bits of the 2k-bit k-mer
  __device__ __forceinline__ void begin(lds &s) {
    if (threadIdx.x < 64) { s.tot[threadIdx.x] = 0.0; s.und[threadIdx.x] = 0.0; }
    for (uint32_t v = threadIdx.x; v < NLUT; v += blockDim.x) {
      double rk, pr;
      mfx_getK_core(peak, n_prob, probK, probP, v, rk, pr);
      s.rk[v] = rk;
    }
    __syncthreads();
  }
  __device__ __forceinline__ void pair(lds &s, bool have, uint64_t key, uint32_t rv, uint32_t av) {
    if (!have || rv == 0u) return;                             // asm-only k-mer (:106-109)
    double readK, prob;
    if (rv < NLUT) readK = s.rk[rv];
    else mfx_getK_core(peak, n_prob, probK, probP, rv, readK, prob);
    const double asmK = (double)av;
    const uint32_t piece = (uint32_t)(key >> pshift) & 63u;
    atomicAdd(&s.tot[piece], readK);                           // :113
    if (readK > asmK) atomicAdd(&s.und[piece], readK - asmK);  // :115-116
  }
  __device__ __forceinline__ void end(lds &s) {
    __syncthreads();
    if (threadIdx.x < 64) {
      if (s.tot[threadIdx.x] != 0.0) atomicAdd(&pieces[threadIdx.x], s.tot[threadIdx.x]);
      if (s.und[threadIdx.x] != 0.0) atomicAdd(&pieces[64 + threadIdx.x], s.und[threadIdx.x]);
    }
  }
};

// mfx_spectrum_kernel's bins (mfx_spectrum.h, its device functions as they are; a.t takes no part): the read count through -min / -max as
// that kernel applies them, a read-only k-mer with asm count 0, an asm-only k-mer with read count 0.
template <bool AGG>
struct mfx_join_spectrum {
  typedef uint32_t asm_t;
  struct lds { uint32_t bins[MFX_SPEC_LDS_WORDS]; };
  mfx_spectrum_args a;
  uint64_t minV, maxV;
  uint64_t counted;
  __device__ __forceinline__ void begin(lds &s) { counted = 0; mfx_spec_begin(a, s.bins); }
  __device__ __forceinline__ void pair(lds &s, bool have, uint64_t, uint32_t rv, uint32_t av) {
    const uint32_t r = (rv < minV || rv > maxV) ? 0u : rv;     // -min / -max (merfin.C:199-200)
    counted += mfx_spec_count<AGG>(a, s.bins, have, r, av);
  }
  __device__ __forceinline__ void end(lds &s) { mfx_spec_end(a, s.bins, counted); }
};

hipError_t mfx_k_join_completeness(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *kb, const uint32_t *vb, uint64_t lb, int k, double peak,
                                   uint32_t n_prob, const uint32_t *probK, const double *probP, double *pieces, uint64_t *stats, int grid, hipStream_t st) {
  mfx_join_completeness c;
  c.peak = peak; c.n_prob = n_prob; c.probK = probK; c.probP = probP; c.pieces = pieces;
  c.pshift = 2 * k >= 6 ? 2 * k - 6 : 0;
  return mfx_join_launch(ka, va, la, kb, vb, lb, c, stats, grid, st);
}

hipError_t mfx_k_join_spectrum(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *kb, const uint32_t *vb, uint64_t lb, const mfx_spectrum_args &a,
                               uint64_t minV, uint64_t maxV, uint64_t *stats, int grid, hipStream_t st) {
  if (a.aggregate) {
    mfx_join_spectrum<true> c;
    c.a = a; c.minV = minV; c.maxV = maxV;
    return mfx_join_launch(ka, va, la, kb, vb, lb, c, stats, grid, st);
  }
  mfx_join_spectrum<false> c;
  c.a = a; c.minV = minV; c.maxV = maxV;
  return mfx_join_launch(ka, va, la, kb, vb, lb, c, stats, grid, st);
}
