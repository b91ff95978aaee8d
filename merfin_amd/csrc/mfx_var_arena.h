// mfx_var_arena.h -- the device arena of one batch of the variant modes (mfx_paths.cpp): every array a batch's kernels read or write is a
// piece of ONE allocation that its owner keeps from batch to batch.  Host arithmetic only, no HIP: tools/native/var_arena_check.cpp runs
// it over a host buffer under the sanitizers.
//
// Two forms.  SCORING (mfx_score_paths, mfx_score_paths_trv): the text, the lookup's values and counters, the path table, the scores, the
// tables of the clusters the device enumerates.  CLAIM (mfx_claim_paths_batch): the text, the geometry of the one contig it is, the path
// table the traverse kernel fills, the cluster tables -- no values and no scores; its empty pieces keep one element (or 8 bytes).
#pragma once

#include "mfx_traverse.h"

#include <stdint.h>

#include <type_traits>

constexpr uint64_t MFX_VAR_TILE = 4096;        // MFX_TILE (mfx_internal.h): the lookup and claim kernels load whole tiles, one past the end

struct mfx_var_sizes {
  uint64_t total = 0;                 // bytes of the batch's text: the host's paths and the room of the device's
  uint64_t npaths = 0, nvals = 0;     // path slots and rows, the host's and the device's together
  uint64_t ncl = 0, nvar = 0, nal = 0, win_bytes = 0, al_bytes = 0;      // the device part's tables (mfx_trv_batch)
  bool     need_dk = false;
  bool     claim = false;
};

struct mfx_var_arena {
  uint8_t  *text = nullptr;                                     // [text_bytes]
  uint32_t *readV = nullptr, *asmV = nullptr;                   // [total]            scoring
  uint64_t *stats = nullptr;                                    // [2]                scoring
  uint64_t *geo = nullptr;                                      // [4]                claim: contig_off[1], contig_len[1], tile_start[2]
  uint64_t *off = nullptr, *voff = nullptr, *cfirst = nullptr;  // [npaths]
  uint32_t *len = nullptr, *nv = nullptr;                       // [npaths]
  int32_t  *gt = nullptr;                                       // [nvals]
  uint32_t *vidx = nullptr, *vlen = nullptr;                    // [nvals]
  uint32_t *numM = nullptr;                                     // [npaths]           scoring
  double   *totdk = nullptr;                                    // [npaths] need_dk   scoring
  mfx_trv_cluster *cl = nullptr;                                // [ncl]
  mfx_trv_variant *var = nullptr;                               // [nvar]
  mfx_trv_allele  *al = nullptr;                                // [nal]
  char     *win = nullptr, *alt = nullptr;                      // [win_bytes], [al_bytes]
  uint32_t *np = nullptr, *status = nullptr;                    // [ncl]
  uint64_t  text_bytes = 0;
};

// Lays the pieces of a batch of these sizes out, each from a 256-byte boundary, and returns the bytes they take together.  `a` null: the
// sum only (what the owner grows its allocation to); else `base` is that allocation and *a gets the pieces' addresses.
static inline uint64_t mfx_var_arena_lay(const mfx_var_sizes &z, uint8_t *base, mfx_var_arena *a) {
  uint64_t need = 0;
  mfx_var_arena none, &A = a ? *a : none;
  auto put = [&](auto *&p, uint64_t bytes) {
    if (a) p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + need);
    need += (bytes + 255) & ~255ull;
  };
  const uint64_t text_bytes = ((z.total + MFX_VAR_TILE - 1) / MFX_VAR_TILE + 2) * MFX_VAR_TILE + 256;
  const uint64_t pad = z.claim ? 8 : 0;                                      // the claim form's cluster tables are never empty pieces
  auto some = [&](uint64_t n) { return n || !z.claim ? n : 1; };              // ... nor are its path table and per-cluster words
  const uint64_t NP = some(z.npaths), NV = z.nvals ? z.nvals : 1, NC = some(z.ncl);
  A.text_bytes = text_bytes;
  put(A.text, text_bytes);
  if (z.claim) put(A.geo, 4 * 8);
  else {
    put(A.readV, z.total * 4);
    put(A.asmV, z.total * 4);
    put(A.stats, 2 * 8);
  }
  put(A.off, NP * 8);
  put(A.len, NP * 4);
  put(A.nv, NP * 4);
  put(A.voff, NP * 8);
  put(A.cfirst, NP * 8);
  put(A.gt, NV * 4);
  put(A.vidx, NV * 4);
  put(A.vlen, NV * 4);
  if (!z.claim) {
    put(A.numM, NP * 4);
    put(A.totdk, (z.need_dk ? NP : 1) * 8);
  }
  put(A.cl, NC * sizeof(mfx_trv_cluster));
  put(A.var, z.nvar * sizeof(mfx_trv_variant) + pad);
  put(A.al, z.nal * sizeof(mfx_trv_allele) + pad);
  put(A.win, z.win_bytes + pad);
  put(A.alt, z.al_bytes + pad);
  put(A.np, NC * 4);
  put(A.status, NC * 4);
  return need;
}
