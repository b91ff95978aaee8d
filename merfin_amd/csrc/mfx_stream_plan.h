// mfx_stream_plan.h -- the host arithmetic of the packed transport of an assembly in host memory (mfx_stream.cpp: the streamed -hist and
// mfx_seq_upload): where the contigs lie, where the tiles are cut into chunks, which bases a chunk carries, and the share of a chunk that one
// host thread encodes.  No HIP call: tools/native/stream_plan_check.cpp runs all of it without a device.
#pragma once
#include "mfx_internal.h"

#include <string.h>
#include <algorithm>
#include <vector>

extern "C" void mfx_pack_bases(const uint8_t *src, uint64_t n, uint64_t *codes, uint32_t *valid);      // mfx_pack.cpp

// where the contigs of `lens` lie in the padded buffer and which tiles they own
inline void seq_layout_fill(mfx_seq *s, const uint64_t *lens, uint32_t ncontigs) {
  s->ncontigs = ncontigs;
  s->off.resize(ncontigs);
  s->len.assign(lens, lens + ncontigs);
  s->tile_start.resize((size_t)ncontigs + 1);
  uint64_t o = 0, t = 0;
  for (uint32_t c = 0; c < ncontigs; ++c) {
    s->off[c] = o;
    s->tile_start[c] = t;
    t += (lens[c] + MFX_TILE - 1) / MFX_TILE;
    s->total_bases += lens[c];
    o = (o + lens[c] + 1 + MFX_ALIGN - 1) / MFX_ALIGN * MFX_ALIGN;   // >= 1 separator byte, next contig 128-byte aligned
  }
  s->tile_start[ncontigs] = t;
  s->ntiles = t;
  s->buf_bytes = o + MFX_TILE + 2 * MFX_ALIGN;                        // tail tiles read one tile + halo past the end
}

struct Piece { uint32_t contig; uint64_t pos, n; };      // bases [pos, pos+n) of a contig

// the bases the tiles [t0, t1) read: their own positions plus the (k-1)-base halo behind the last tile of a contig
// piece (a whole 128-byte line of it: the next chunk re-sends those bytes, same values)
inline void chunk_pieces(const mfx_seq *s, uint64_t t0, uint64_t t1, std::vector<Piece> &out) {
  out.clear();
  uint32_t c = (uint32_t)(std::upper_bound(s->tile_start.begin(), s->tile_start.end(), t0) - s->tile_start.begin()) - 1;
  for (; c < s->ncontigs && s->tile_start[c] < t1; ++c) {
    const uint64_t cb = std::max(t0, s->tile_start[c]), ce = std::min(t1, s->tile_start[c + 1]);
    if (ce <= cb) continue;                                 // an empty contig owns no tile
    const uint64_t p0 = (cb - s->tile_start[c]) * MFX_TILE;
    const uint64_t p1 = std::min<uint64_t>(s->len[c], (ce - s->tile_start[c]) * MFX_TILE + MFX_ALIGN);
    if (p1 > p0) out.push_back({c, p0, p1 - p0});
  }
}

// The chunk boundaries of a streamed run over T tiles, ascending, the last one T.  Chunks grow from CH0 to CH tiles (production: 2048 and
// 32768, 8 MB to 128 MB of bases): the first tile reaches the kernel after ~0.2 ms, and the bulk runs in few, long launches (every launch pays
// a ramp-up and a tail of its persistent blocks: 47 launches of 64 MB cost 38 ms of kernel time for 3 Gb, one launch 33.4 ms) ...
// ... and shrink again at the end (64, 32, 16 MB): what follows the last upload is the evaluation of the last chunk alone
inline std::vector<uint64_t> stream_cuts(uint64_t T, uint64_t CH0, uint64_t CH) {
  std::vector<uint64_t> cuts, tail;                         // tail: sizes of the closing chunks, last first
  uint64_t back = 0;
  for (uint64_t sz = 2 * CH0; sz < CH && back + sz + CH <= T / 2; sz *= 2) { tail.push_back(sz); back += sz; }
  const uint64_t front_end = T - back;
  uint64_t t0 = 0;
  for (uint64_t sz = CH0; t0 < front_end; sz = std::min(CH, sz * 2)) {
    uint64_t t1 = std::min(front_end, t0 + sz);
    if (front_end - t1 < sz / 2) t1 = front_end;            // no short launch in the middle (at most 1.5 x CH tiles)
    cuts.push_back(t1);
    t0 = t1;
  }
  for (size_t i = tail.size(); i-- > 0;) { t0 += tail[i]; cuts.push_back(t0); }
  return cuts;
}
// ... of an upload: CH tiles each, the last one what is left
inline std::vector<uint64_t> upload_cuts(uint64_t T, uint64_t CH) {
  std::vector<uint64_t> cuts;
  for (uint64_t t0 = 0; t0 < T; t0 += CH) cuts.push_back(std::min(T, t0 + CH));
  return cuts;
}

// one chunk: the tiles [t0, t1) of the sequence, the bases they read, and the range [lo, hi) of the padded buffer those span
struct StreamChunk { std::vector<Piece> pieces; uint64_t lo = 0, hi = 0, t0 = 0, t1 = 0; };

// the chunks of the tiles [TL, TL + cuts.back()) cut at TL + cuts[i].  keep_empty: a chunk without bases stays (the streamed run still launches
// its tile range); the upload has nothing to send for it
inline std::vector<StreamChunk> stream_chunks(const mfx_seq *s, uint64_t TL, const std::vector<uint64_t> &cuts, bool keep_empty) {
  std::vector<StreamChunk> chunks;
  uint64_t t0 = 0;
  for (const uint64_t cut : cuts) {
    StreamChunk c;
    c.t0 = TL + t0;
    c.t1 = TL + cut;
    t0 = cut;
    chunk_pieces(s, c.t0, c.t1, c.pieces);
    if (!c.pieces.empty()) {
      c.lo = s->off[c.pieces.front().contig] + c.pieces.front().pos;                 // a multiple of 128
      c.hi = (s->off[c.pieces.back().contig] + c.pieces.back().pos + c.pieces.back().n + 31) / 32 * 32;
    } else if (!keep_empty) continue;
    chunks.push_back(std::move(c));
  }
  return chunks;
}

// words (32 bases) of a staging buffer that holds any of the chunks, rounded up to `round` of them
inline size_t stage_words(const std::vector<StreamChunk> &chunks, size_t round) {
  size_t m = 0;
  for (const StreamChunk &c : chunks) m = std::max<size_t>(m, (c.hi - c.lo) / 32);
  return (m + 2 + round - 1) / round * round;
}

// the words [w0, w1) of a chunk that packer w of W encodes
inline void chunk_share(const StreamChunk &c, unsigned w, unsigned W, uint64_t *w0, uint64_t *w1) {
  const uint64_t nw = (c.hi - c.lo) / 32;
  *w0 = nw * w / W;
  *w1 = nw * (w + 1) / W;
}

// packer w of W encodes its share of the chunk into the staging planes (word 0 = the bases from c.lo on)
inline void pack_chunk_share(const mfx_seq *s, const char *const *bases, const StreamChunk &c, unsigned w, unsigned W, uint64_t *codes, uint32_t *valid) {
  uint64_t w0, w1;
  chunk_share(c, w, W, &w0, &w1);
  if (w1 <= w0) return;
  memset(codes + w0, 0, (w1 - w0) * 8);                // gaps between contigs and the words behind a contig's end
  memset(valid + w0, 0, (w1 - w0) * 4);
  const uint64_t my_lo = c.lo + 32 * w0, my_hi = c.lo + 32 * w1;
  for (const Piece &pc : c.pieces) {
    const uint64_t at = s->off[pc.contig] + pc.pos;      // a multiple of 128
    const uint64_t b = std::max(my_lo, at), e = std::min(my_hi, at + pc.n);
    if (e > b) mfx_pack_bases(reinterpret_cast<const uint8_t *>(bases[pc.contig]) + pc.pos + (b - at), e - b, codes + (b - c.lo) / 32, valid + (b - c.lo) / 32);
  }
}

// the validity words of [w0, w1) that are not all ones, as {word index | word << 32}, in order; their number, or -1: more than `cap`
inline int64_t list_valid_exceptions(const uint32_t *valid, uint64_t w0, uint64_t w1, uint64_t *out, size_t cap) {
  size_t cnt = 0;
  for (uint64_t i = w0; i < w1; ++i) {
    const uint32_t vw = valid[i];
    if (vw == 0xffffffffu) continue;
    if (cnt == cap) return -1;
    out[cnt++] = (uint64_t)i | ((uint64_t)vw << 32);
  }
  return (int64_t)cnt;
}
