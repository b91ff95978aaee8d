// The host arithmetic of the packed transport (csrc/mfx_stream_plan.h: chunk cuts, chunks and their pieces, the share of a chunk one host
// thread encodes, the list of its exceptional validity words) without a device, under AddressSanitizer + UBSan: every buffer is a host
// block of exactly the size the code may touch.
//   g++ -fsanitize=address,undefined -std=c++17 -I merfin_amd/csrc -I include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
//       tools/native/stream_plan_check.cpp merfin_amd/csrc/mfx_pack.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "mfx_stream_plan.h"

static int bad = 0, cases = 0;
#define CHECK(x) do { if (!(x)) { if (++bad <= 40) printf("MISMATCH %s:%d: %s\n", __FILE__, __LINE__, #x); } } while (0)

typedef std::vector<uint64_t> U64s;

// ---- 1. cuts ---------------------------------------------------------------------------------------------------------------------------
static void check_cuts(uint64_t T, uint64_t CH0, uint64_t CH) {
  const U64s cuts = stream_cuts(T, CH0, CH);
  if (T == 0) { CHECK(cuts.empty()); return; }
  CHECK(!cuts.empty() && cuts.back() == T);
  U64s sz;
  for (size_t i = 0; i < cuts.size(); ++i) {
    CHECK(cuts[i] > (i ? cuts[i - 1] : 0));                      // strictly ascending, no empty chunk
    sz.push_back(cuts[i] - (i ? cuts[i - 1] : 0));
    CHECK(2 * sz.back() <= 3 * CH);                              // at most 1.5 CH tiles
  }
  // chunks never shrink before the schedule's end; from the first that does, what FOLLOWS halves down to 2 CH0 (that first one is either
  // part of this tail or the last, irregular chunk in front of it)
  size_t d = 1;
  while (d < sz.size() && sz[d] >= sz[d - 1]) ++d;
  if (d + 1 < sz.size()) {
    CHECK(sz.back() == 2 * CH0);
    for (size_t i = d + 1; i + 1 < sz.size(); ++i) CHECK(sz[i] == 2 * sz[i + 1] && sz[i] < CH);
  }
}

static void cuts_part() {
  for (uint64_t T : {0ull, 1ull, 2047ull, 2048ull, 2049ull, 3071ull, 3072ull, 6143ull, 6144ull, 14336ull, 14337ull, 100000ull, 732422ull}) check_cuts(T, 2048, 32768);
  for (uint64_t T = 0; T <= 4096; ++T) check_cuts(T, 2, 32);
  // the production schedule, as the loop inside hist_run_streamed_packed made it before it moved here (a scratch program around that loop)
  CHECK(stream_cuts(3072, 2048, 32768) == U64s({2048, 3072}));
  CHECK(stream_cuts(6144, 2048, 32768) == U64s({2048, 6144}));
  CHECK(stream_cuts(14336, 2048, 32768) == U64s({2048, 6144, 14336}));
  CHECK(stream_cuts(15037, 2048, 32768) == U64s({2048, 6144, 15037}));      // (no chunk shorter than half its size: 701 tiles join the third)
  CHECK(stream_cuts(100000, 2048, 32768) == U64s({2048, 6144, 14336, 30720, 63488, 87712, 95904, 100000}));
  CHECK(stream_cuts(732422, 2048, 32768) ==
        U64s({2048,   6144,   14336,  30720,  63488,  96256,  129024, 161792, 194560, 227328, 260096, 292864, 325632, 358400,
              391168, 423936, 456704, 489472, 522240, 555008, 587776, 620544, 653312, 686080, 703750, 720134, 728326, 732422}));
  CHECK(upload_cuts(0, 8192).empty() && upload_cuts(8192, 8192) == U64s({8192}) && upload_cuts(8193, 8192) == U64s({8192, 8193}));
  CHECK(upload_cuts(4 * 8192 + 3, 8192) == U64s({8192, 16384, 24576, 32768, 32771}));
  ++cases;
}

// ---- 2. chunks -------------------------------------------------------------------------------------------------------------------------
struct World {
  mfx_seq s;
  std::vector<std::vector<uint8_t>> text;                        // every contig a block of exactly its length
  std::vector<const char *> bases;
  std::vector<uint64_t> ref_codes;                               // the planes of the whole padded buffer: one mfx_pack_bases call per contig
  std::vector<uint32_t> ref_valid;
  explicit World(const U64s &lens) {
    seq_layout_fill(&s, lens.data(), (uint32_t)lens.size());
    uint64_t x = 88172645463325252ull + lens.size();
    static const char alphabet[] = "ACGTACGTACGTACGTacgtNnRYKMSWBDHV-*";
    for (uint64_t n : lens) {
      text.emplace_back(n);
      for (auto &b : text.back()) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const unsigned r = (unsigned)(x >> 40) & 1023;
        b = r < 1000 ? (uint8_t)"ACGT"[r & 3] : r < 1016 ? (uint8_t)alphabet[(x >> 20) % (sizeof(alphabet) - 1)] : r < 1020 ? 0 : 255;
      }
      bases.push_back(reinterpret_cast<const char *>(text.back().data()));
    }
    ref_codes.assign(s.buf_bytes / 32, 0);
    ref_valid.assign(s.buf_bytes / 32, 0);
    for (uint32_t c = 0; c < s.ncontigs; ++c) {
      CHECK(s.off[c] % MFX_ALIGN == 0);
      mfx_pack_bases(text[c].data(), s.len[c], ref_codes.data() + s.off[c] / 32, ref_valid.data() + s.off[c] / 32);
    }
  }
};

static void check_chunks(const World &w, uint64_t TL, uint64_t TH, const U64s &cuts) {
  const mfx_seq *s = &w.s;
  const std::vector<StreamChunk> ch = stream_chunks(s, TL, cuts, true), up = stream_chunks(s, TL, cuts, false);
  CHECK(ch.size() == cuts.size());
  size_t nu = 0;
  uint64_t next = TL;
  for (const StreamChunk &c : ch) {
    CHECK(c.t0 == next && c.t1 > c.t0);                          // every tile of [TL, TH) in exactly one chunk
    next = c.t1;
    if (c.pieces.empty()) { CHECK(c.lo == 0 && c.hi == 0 && c.t0 >= s->ntiles); continue; }      // (only a tile range behind the sequence carries nothing)
    CHECK(nu < up.size() && up[nu].lo == c.lo && up[nu].hi == c.hi && up[nu].t0 == c.t0 && up[nu].t1 == c.t1 && up[nu].pieces.size() == c.pieces.size());
    ++nu;
    CHECK(c.lo % 128 == 0 && c.hi % 32 == 0 && c.hi > c.lo && c.hi <= s->buf_bytes);
    for (size_t i = 0; i < c.pieces.size(); ++i) {
      const Piece &p = c.pieces[i];
      CHECK(p.n > 0 && p.pos + p.n <= s->len[p.contig] && (i == 0 || p.contig > c.pieces[i - 1].contig));      // a contig in at most one piece
      CHECK(s->off[p.contig] + p.pos >= c.lo && s->off[p.contig] + p.pos + p.n <= c.hi);
    }
    for (uint64_t t = c.t0; t < std::min(c.t1, s->ntiles); ++t) {      // every base a tile reads, its halo up to the contig's end included
      const uint32_t k = (uint32_t)(std::upper_bound(s->tile_start.begin(), s->tile_start.end(), t) - s->tile_start.begin()) - 1;
      const uint64_t b0 = (t - s->tile_start[k]) * MFX_TILE, b1 = std::min<uint64_t>(s->len[k], b0 + MFX_TILE + MFX_ALIGN);
      int holds = 0;
      for (const Piece &p : c.pieces) holds += p.contig == k && p.pos <= b0 && b1 <= p.pos + p.n;
      CHECK(holds == 1);
    }
  }
  CHECK(next == TL + (cuts.empty() ? 0 : cuts.back()) && nu == up.size());
  for (size_t round : {(size_t)131072, (size_t)4096}) {
    const size_t sw = stage_words(ch, round);
    CHECK(sw % round == 0 && sw == stage_words(up, round));
    for (const StreamChunk &c : ch) CHECK((c.hi - c.lo) / 32 + 2 <= sw);
  }
  (void)TH;
}

// ---- 3. encoder shares -----------------------------------------------------------------------------------------------------------------
static void check_shares(const World &w, const std::vector<StreamChunk> &chunks) {
  for (const StreamChunk &c : chunks) {
    const uint64_t nw = (c.hi - c.lo) / 32;
    for (unsigned W : {1u, 2u, 3u, 16u, 64u}) {
      std::unique_ptr<uint64_t[]> codes(new uint64_t[nw]);                 // sized exactly, filled with what must not stay
      std::unique_ptr<uint32_t[]> valid(new uint32_t[nw]);
      memset(codes.get(), 0xAB, nw * 8);
      memset(valid.get(), 0xAB, nw * 4);
      uint64_t covered = 0;
      for (unsigned t = 0; t < W; ++t) {
        uint64_t w0, w1;
        chunk_share(c, t, W, &w0, &w1);
        CHECK(w0 == covered && w1 >= w0);                                  // the shares tile [0, nw)
        covered = w1;
        pack_chunk_share(&w.s, w.bases.data(), c, t, W, codes.get(), valid.get());
      }
      CHECK(covered == nw);
      CHECK(nw == 0 || memcmp(codes.get(), w.ref_codes.data() + c.lo / 32, nw * 8) == 0);
      CHECK(nw == 0 || memcmp(valid.get(), w.ref_valid.data() + c.lo / 32, nw * 4) == 0);
      // the exceptional validity words of every share: exactly those that are not all ones, in order; out of room exactly beyond `cap`
      for (unsigned t = 0; t < W; ++t) {
        uint64_t w0, w1;
        chunk_share(c, t, W, &w0, &w1);
        U64s want;
        for (uint64_t i = w0; i < w1; ++i) if (valid[i] != 0xffffffffu) want.push_back(i | ((uint64_t)valid[i] << 32));
        for (size_t cap : {want.size(), want.size() + 3, want.size() - 1, (size_t)0}) {
          if (cap > want.size() + 3) continue;                             // (size - 1 of an empty list)
          std::unique_ptr<uint64_t[]> out(new uint64_t[cap]);
          const int64_t n = list_valid_exceptions(valid.get(), w0, w1, out.get(), cap);
          if (want.size() > cap) CHECK(n == -1);
          else CHECK(n == (int64_t)want.size() && (n == 0 || memcmp(out.get(), want.data(), (size_t)n * 8) == 0));
        }
      }
    }
  }
}

static void world(const char *name, const U64s &lens, uint64_t CH0, uint64_t CH, uint64_t UCH, bool shares = true) {
  const World w(lens);
  const uint64_t T = w.s.ntiles;
  uint64_t nt = 0;
  for (uint64_t n : lens) nt += (n + MFX_TILE - 1) / MFX_TILE;
  CHECK(T == nt && w.s.tile_start.back() == T);
  check_chunks(w, 0, T, stream_cuts(T, CH0, CH));
  check_chunks(w, 0, T, upload_cuts(T, UCH));
  if (T) { U64s past = upload_cuts(T, UCH); past.push_back(T + 5); check_chunks(w, 0, T + 5, past); }      // a range behind the sequence: kept / dropped
  // parts [TL, TH): every cut of the range in turn as TL, the end one third further on -- inside contigs wherever a contig has several tiles
  for (uint64_t TL = 0; TL < T; TL += std::max<uint64_t>(1, T / 7)) {
    const uint64_t TH = std::min(T, TL + std::max<uint64_t>(1, T / 3));
    check_chunks(w, TL, TH, stream_cuts(TH - TL, CH0, CH));
    if (shares && T <= 64) check_shares(w, stream_chunks(&w.s, TL, stream_cuts(TH - TL, CH0, CH), true));
  }
  if (shares) {
    check_shares(w, stream_chunks(&w.s, 0, stream_cuts(T, CH0, CH), true));
    check_shares(w, stream_chunks(&w.s, 0, upload_cuts(T, UCH), false));
  }
  printf("case %s: %zu contigs, %llu tiles\n", name, lens.size(), (unsigned long long)T);
  ++cases;
}

int main() {
  cuts_part();
  const uint64_t TILE = MFX_TILE, CH0 = 2048;
  world("one base", {1}, 2, 32, 8);
  world("a tile exactly, one less, one more", {TILE, TILE - 1, TILE + 1}, 2, 32, 1);
  world("empty contigs first, last and in a row", {0, 0, 5000, 0, 0, 0, 9000, 131, 0}, 2, 32, 2);
  world("only empty contigs", {0, 0}, 2, 32, 8);
  world("300 contigs of 100 bases", U64s(300, 100), 2, 32, 8);
  world("several tiles per contig, small chunks", {7 * TILE + 77, 5, 33 * TILE - 127, 0, 12 * TILE + 4095, 128, 127, 129}, 2, 8, 4);
  // the production schedule around its first cut (2048 tiles; the second contig makes the run long enough for one): a contig of CH0 tiles
  // less one base ends one base before the cut, one of CH0 tiles and a base is cut a tile and a base before its end
  world("CH0 tiles - 1 base", {CH0 * TILE - 1, 1100 * TILE}, 2048, 32768, 8192);
  world("CH0 tiles + 1 base", {CH0 * TILE + 1, 1100 * TILE}, 2048, 32768, 8192);
  printf("%s (%d mismatches, %d cases)\n", bad ? "FAILED" : "OK", bad, cases);
  return bad ? 1 : 0;
}
