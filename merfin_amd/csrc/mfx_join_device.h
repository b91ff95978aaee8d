// mfx_join_device.h -- mfx_join_kernel and its launcher, for the kernel files that bring a consumer of their own (mfx_join.hip: the
// -completeness sums and the -spectrum image; mfx_diploid.hip: the two-assembly reductions).  The tiling, the ownership rule and the LDS of
// the walk are described in mfx_join.hip; the walk itself is mfx_join.h's, one text for the device and the host.
//
// A consumer C has: asm_t, the value type of the asm run (uint32_t, or uint64_t for a pair run: the tile's counts are then staged 64 bits
// wide, 32 KB instead of 24 KB a tile); struct lds; begin(lds &) once per workgroup; pair(lds &, have, key, rv, av) MFX_JOIN_PER times per
// lane and tile, every lane of a wave together; end(lds &).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfx_join.h"

// stats[0]: the k-mers both runs hold.
template <class C>
__global__ __launch_bounds__(MFX_JOIN_LANES) void mfx_join_kernel(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *kb, const typename C::asm_t *vb,
                                                                  uint64_t lb, C c, unsigned long long *stats) {
  typedef typename C::asm_t V;
  __shared__ uint64_t s_k[MFX_JOIN_TILE];
  __shared__ V s_v[MFX_JOIN_TILE];
  __shared__ uint64_t s_cut[2];
  __shared__ typename C::lds s_c;
  const uint32_t tid = threadIdx.x;
  const uint64_t total = la + lb, tiles = (total + MFX_JOIN_TILE - 1) / MFX_JOIN_TILE;
  uint32_t both = 0u;
  c.begin(s_c);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // (uniform)
    const uint64_t d0 = tile * MFX_JOIN_TILE, d1 = d0 + MFX_JOIN_TILE < total ? d0 + MFX_JOIN_TILE : total;
    if (tid < 2u) s_cut[tid] = mfx_merge_cut<uint64_t>(ka, la, kb, lb, tid ? d1 : d0);
    __syncthreads();
    const uint64_t a0 = s_cut[0], b0 = d0 - a0;
    const uint32_t na = (uint32_t)(s_cut[1] - a0), n = (uint32_t)(d1 - d0), nb = n - na;
    for (uint32_t i = tid; i < n; i += MFX_JOIN_LANES) {
      s_k[i] = i < na ? ka[a0 + i] : kb[b0 + (i - na)];
      s_v[i] = i < na ? (V)va[a0 + i] : vb[b0 + (i - na)];
    }
    const bool more_b = b0 + nb < lb;
    const mfx_join_tile_t<V> T{s_k, s_v, na, nb, a0 ? ka[a0 - 1] : MFX_JOIN_NONE, more_b ? kb[b0 + nb] : MFX_JOIN_NONE, more_b ? vb[b0 + nb] : (V)0};
    __syncthreads();
    const uint32_t t0 = tid * MFX_JOIN_PER < n ? tid * MFX_JOIN_PER : n, t1 = t0 + MFX_JOIN_PER < n ? t0 + MFX_JOIN_PER : n;
    mfx_join_lane(T, t0, t1, [&](bool have, uint64_t key, uint32_t rv, V av) {
      both += (have && rv != 0u && av != (V)0) ? 1u : 0u;
      c.pair(s_c, have, key, rv, av);
    });
    __syncthreads();                                             // (the tile and its cuts are written again in the next turn)
  }
  c.end(s_c);
  for (int o = 32; o; o >>= 1) both += __shfl_xor(both, o, 64);
  if ((tid & 63u) == 0u && both) atomicAdd(&stats[0], (unsigned long long)both);
}

template <class C>
static hipError_t mfx_join_launch(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *kb, const typename C::asm_t *vb, uint64_t lb, const C &c,
                                  uint64_t *stats, int grid, hipStream_t st) {
  const uint64_t tiles = mfx_join_tiles(la, lb);
  if (tiles == 0) return hipSuccess;
  if (la + lb > 0xffffffffull) return hipErrorInvalidValue;    // (a workgroup adds one to an LDS bin per pair at the most: none can wrap)
  const uint64_t g = tiles < (uint64_t)(grid > 0 ? grid : 1) ? tiles : (uint64_t)(grid > 0 ? grid : 1);
  mfx_join_kernel<C><<<(unsigned)g, MFX_JOIN_LANES, 0, st>>>(ka, va, la, kb, vb, lb, c, reinterpret_cast<unsigned long long *>(stats));
  return hipGetLastError();
}
