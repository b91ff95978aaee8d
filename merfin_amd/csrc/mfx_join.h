// mfx_join.h -- the plain arithmetic of mfx_db_join_* (mfx_db_join.cpp) and of mfx_join_kernel (mfx_join.hip): how two ascending runs are cut
// into tiles and lane shares of the merged order, and which lane owns a key that both runs hold.  The lane walk below is compiled for the
// device and for the host from one text: the kernel runs it over a tile staged in LDS, mfx_join_host over plain arrays, tile after tile
// and lane after lane -- tools/native/db_join_sanitize.cpp drives that under the sanitizers, tests/test_join_cpu.py through
// mfx_db_join_host.  No HIP call, no library state.
//
// The merged order is mfx_merge_cut's (mfx_merge.h): ascending, a key of both runs as the read record first and its asm twin next to it.
// Position p of that order belongs to tile p / MFX_JOIN_TILE and, inside the tile, to lane (p % MFX_JOIN_TILE) / MFX_JOIN_PER.
//
// OWNERSHIP.  The lane whose share holds the READ record of a key owns the pair: it looks at the next asm record of the merged order --
// inside its share, in the next lane's share or in the next tile (one record across the boundary) -- and takes its count when the keys
// are equal.  A lane that holds an ASM record skips it when the read record in front of it in merged order -- inside its share, in the
// lane before or in the tile before (one record back across the boundary) -- has the same key; else the key is asm-only and the lane owns
// it.  Both runs ascend strictly, so a key has at most one record in each, and every key is seen as one pair by one lane.
#pragma once
#include <stdint.h>

#include "mfx_merge.h"

constexpr uint32_t MFX_JOIN_PER = 8;                           // merged positions per lane (the lane grain)
constexpr uint32_t MFX_JOIN_LANES = 256;
constexpr uint32_t MFX_JOIN_TILE = MFX_JOIN_LANES * MFX_JOIN_PER;      // merged positions per tile
constexpr uint64_t MFX_JOIN_NONE = ~0ull;                      // no record across the boundary (a k-mer is below 2^62)

// A tile as a lane sees it: k[0 .. na) the tile's read k-mers, k[na .. na + nb) its asm k-mers, v their counts; prev_a the read k-mer in
// front of the tile, next_bk / next_bv the asm record behind it (MFX_JOIN_NONE where the run has none).  V: the asm run's value -- a count
// (uint32_t: mfx_db_join_*) or the two counts of a pair run in one word (uint64_t: mfx_db_diploid, mfx_diploid.h); a read count staged in v
// is widened to V and is a uint32_t again where the walk hands it on.
template <class V>
struct mfx_join_tile_t {
  const uint64_t *k;
  const V *v;
  uint32_t na, nb;
  uint64_t prev_a, next_bk;
  V next_bv;
};
using mfx_join_tile = mfx_join_tile_t<uint32_t>;

// The share [t0, t1) of the tile's merged positions, t1 - t0 <= MFX_JOIN_PER: sink(have, k-mer, read count, asm count) is called
// MFX_JOIN_PER times whatever the share holds (a consumer may vote across the wave), `have` for the pairs the lane owns; a count of 0
// stands for "not in that run".
template <class V, class Sink>
MFX_MERGE_HD void mfx_join_lane(const mfx_join_tile_t<V> &T, uint32_t t0, uint32_t t1, Sink &&sink) {
  uint32_t i = mfx_merge_cut<uint32_t>(T.k, T.na, T.k + T.na, T.nb, t0), j = t0 - i;
  uint64_t last_a = i ? T.k[i - 1] : T.prev_a;
#if defined(__HIPCC__)                                         // (g++ builds this text as well: tools/native/diploid_sanitize.cpp)
#pragma unroll
#endif
  for (uint32_t r = 0; r < MFX_JOIN_PER; ++r) {
    const bool on = t0 + r < t1, ha = on && i < T.na, hb = j < T.nb;
    const uint64_t xa = ha ? T.k[i] : MFX_JOIN_NONE;
    const uint64_t xb = hb ? T.k[T.na + j] : T.next_bk;          // the next asm record of the merged order, the tile's or the one behind it
    const V vb = hb ? T.v[T.na + j] : T.next_bv;
    const bool from_a = ha && xa <= xb;                          // (the tile's cut: no read k-mer of the tile is above next_bk)
    const bool twin = xb == (from_a ? xa : last_a);
    const bool have = on && (from_a || !twin);
    const uint32_t rv = from_a ? (uint32_t)T.v[i] : 0u;
    sink(have, from_a ? xa : xb, rv, (from_a && !twin) ? (V)0 : vb);
    if (from_a) { last_a = xa; ++i; }
    else if (on) ++j;
  }
}

// the tile of merged positions [d0, d1) of the runs: where it starts in the two runs, what it holds of each, the records across its ends
struct mfx_join_cuts { uint64_t a0, b0; uint32_t na, nb; };
inline mfx_join_cuts mfx_join_tile_cuts(const uint64_t *ka, uint64_t la, const uint64_t *kb, uint64_t lb, uint64_t d0, uint64_t d1) {
  const uint64_t a0 = mfx_merge_cut<uint64_t>(ka, la, kb, lb, d0), a1 = mfx_merge_cut<uint64_t>(ka, la, kb, lb, d1);
  return mfx_join_cuts{a0, d0 - a0, (uint32_t)(a1 - a0), (uint32_t)((d1 - d0) - (a1 - a0))};
}
inline uint64_t mfx_join_tiles(uint64_t la, uint64_t lb) { return (la + lb + MFX_JOIN_TILE - 1) / MFX_JOIN_TILE; }

// The kernel's walk on the host: every tile staged as the kernel stages it, every lane's share walked by mfx_join_lane.
template <class V, class Sink>
inline void mfx_join_host(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *kb, const V *vb, uint64_t lb, Sink &&sink) {
  std::vector<uint64_t> sk(MFX_JOIN_TILE);
  std::vector<V> sv(MFX_JOIN_TILE);
  const uint64_t total = la + lb;
  for (uint64_t d0 = 0; d0 < total; d0 += MFX_JOIN_TILE) {
    const uint64_t d1 = std::min<uint64_t>(d0 + MFX_JOIN_TILE, total);
    const mfx_join_cuts c = mfx_join_tile_cuts(ka, la, kb, lb, d0, d1);
    const uint32_t n = c.na + c.nb;
    for (uint32_t x = 0; x < n; ++x) {
      sk[x] = x < c.na ? ka[c.a0 + x] : kb[c.b0 + (x - c.na)];
      sv[x] = x < c.na ? (V)va[c.a0 + x] : vb[c.b0 + (x - c.na)];
    }
    const bool more_b = c.b0 + c.nb < lb;
    const mfx_join_tile_t<V> T{sk.data(), sv.data(), c.na, c.nb, c.a0 ? ka[c.a0 - 1] : MFX_JOIN_NONE, more_b ? kb[c.b0 + c.nb] : MFX_JOIN_NONE,
                               more_b ? vb[c.b0 + c.nb] : (V)0};
    for (uint32_t lane = 0; lane < MFX_JOIN_LANES; ++lane) {
      const uint32_t t0 = std::min(lane * MFX_JOIN_PER, n), t1 = std::min(t0 + MFX_JOIN_PER, n);
      mfx_join_lane(T, t0, t1, sink);
    }
  }
}

// A window's dense run of an input: its blocks hold `len` records from `off` on, `below` of them under the window and `above` at or over
// its end -- a prefix of the first block and a suffix of the last (mfx_delta_decode_kernel leaves the numbers per block).  False for
// numbers no ascending input gives.
inline bool mfx_join_trim(uint64_t off, uint64_t len, const uint32_t *below, const uint32_t *above, uint64_t nblocks, uint64_t *run_off, uint64_t *run_len) {
  uint64_t nb = 0, na = 0;
  for (uint64_t j = 0; j < nblocks; ++j) { nb += below[j]; na += above[j]; }
  if (nb + na > len || (nblocks && (nb != below[0] || na != above[nblocks - 1]))) return false;
  *run_off = off + nb;
  *run_len = len - nb - na;
  return true;
}
