// mfx_db.cpp -- k-mer database ingest: disk -> device index.
//
// Replaces merylFileReader + merylExactLookup::load as used by
// merfinGlobal::load_Kmers (src/merfin/merfin-globals.C:114-163).  Three
// on-disk forms are accepted:
//   MFX_DB_FLAT   this repo's flat binary (header + u64 k-mers + u32 counts);
//                 always verifiable, used by the tests and by fixtures.
//   MFX_DB_TEXT   `meryl print` text: "<kmer>\t<count>\n" (plain or .gz/.bz2/.xz).
//   MFX_DB_MERYL  a meryl database directory (merylIndex + 64 x 0xBBBBBB.merylData).
//                 The decoder follows the layout of marbl/meryl-utility as
//                 recalled in SURVEY.md Appendix C.  It is UNVALIDATED: the
//                 reference checkout contains no meryl source and no database,
//                 so the decoder has only been exercised against this repo's
//                 own writer of the same layout (tests/meryl_layout.py).  It
//                 refuses anything whose magic numbers / sizes do not match
//                 rather than guessing.
#include "mfx_internal.h"
#include "mfx_kernels.h"
#include "mfx_grow.h"
#include "mfx_merge.h"
#include "mfx_join.h"
#include "mfx_spectrum.h"
#include "mfx_trio.h"
#include "mfx_diploid.h"
#include "mfx_kstar.h"
#include "mfx_pipe.h"
#include "mfx_place.h"

#include <dirent.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <sys/mman.h>
#include <fcntl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

namespace {

typedef unsigned __int128 u128;


bool is_dir(const std::string &p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}
bool is_file(const std::string &p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

int base_code(unsigned char c) {
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'T': case 't': return 2;
    case 'G': case 'g': return 3;
    default: return -1;
  }
}

// ---- flat binary ------------------------------------------------------------
struct FlatHeader {
  char     magic[8];     // "MFXKMER1"
  uint32_t k;
  uint32_t flags;        // bit 0: canonical; bit 1: PACKED records (k <= 21); bit 2: DELTA-coded blocks (sorted k-mers, k <= 31)
  uint64_t n;
  uint64_t n_escape;     // packed: records whose count did not fit the record (was: reserved, 0)
};
// Payload, plain : n k-mers (8 bytes; 16 for k > 31), then n uint32 counts.
// Payload, packed: n records {k-mer << 22 | count} (mfx_internal.h MFX_PACKED_*: 8 bytes per k-mer instead of 12 on disk, in
//                  the staging lanes and over PCIe; a count field of all ones = escape), then the n_escape escaped k-mers
//                  (uint64) and their counts (uint32).
// Payload, delta : what a SORTED database (strictly ascending k-mers: `meryl print` order) is written as -- blocks of
//                  MFX_DELTA_BLOCK k-mers, each {first k-mer (in the directory); count-1 differences of kbits bits; count values
//                  of vbits bits, all ones = escape}: uint64 nblocks, the directory (nblocks + 1 entries {first k-mer, file offset
//                  of the block (48 bits) | kbits << 48 | vbits << 56}; the last entry closes the last block), the blocks (8-byte
//                  aligned; bit fields LSB-first in little-endian uint64 words, the values start at a word boundary), then
//                  the n_escape escaped k-mers and counts as in the packed form.  kbits / vbits are chosen per block (vbits: what
//                  makes block + escapes smallest): 2.5-3 bytes per k-mer of a 30x human read set.  Blocks are decoded by the
//                  kernel that inserts them (mfx_table_add_delta_kernel): on disk, in the staging lanes and over PCIe the
//                  database is a third of its packed size.
constexpr uint32_t FLAT_PACKED = 2u;
constexpr uint32_t FLAT_DELTA = 4u;
// Payload, placed: a delta-coded file whose records are not the k-mers but the numbers P of mfx_place.h -- one to one with the canonical
//                  k-mers, ascending P = ascending LINE of the compact table, for a table of any size (13 <= k <= 30) -- in ascending
//                  order: what `merfin -convert -placed` makes.  The table's update kernel then walks the table line after line instead
//                  of reading a random line per record (mfx_table_add_placed_kernel).  Directory and blocks as in the delta form with P
//                  in the k-mer's place (2k + 3 bits); the escape list holds k-mers.  Bits 8-15 of `flags`: MFX_PLACE_VERSION of the
//                  functions that made P (another version is refused: convert again).
constexpr uint32_t FLAT_PLACED = 8u;
inline uint32_t flat_place_version(const FlatHeader &h) { return (h.flags >> 8) & 0xffu; }

// The header's counts are bounded by the file's size BEFORE any arithmetic uses them (a damaged or crafted header must end in
// MFX_E_FORMAT, never in a wrapped size check, a std::length_error through the C ABI or an out-of-bounds scatter): every
// escape takes 12 bytes; a k-mer takes 8 (16) + 4 bytes plain, 8 packed, and at least 2 bits delta-coded (vbits >= 2).
// nullptr = acceptable, else what is wrong.
const char *flat_header_problem(const FlatHeader &h, uint64_t fsize) {
  if (memcmp(h.magic, "MFXKMER1", 8) != 0) return "bad magic (not a flat k-mer file)";
  if (h.k < 1 || h.k > (uint32_t)MFX_MAX_K) return "k out of range";
  if (fsize < sizeof(FlatHeader)) return "truncated header";
  const uint64_t body = fsize - sizeof(FlatHeader);
  if (h.n_escape > body / 12) return "escape count beyond the file's size";
  const uint64_t rest = body - h.n_escape * 12;
  if (h.flags & FLAT_PLACED) {
    if (!(h.flags & FLAT_DELTA)) return "a placed database is delta-coded";
    if (h.k < (uint32_t)MFX_PLACE_MIN_K || h.k > (uint32_t)MFX_PLACE_MAX_K) return "placed records hold 13 <= k <= 31";
    if (flat_place_version(h) != MFX_PLACE_VERSION) return "placed by another version of the placement functions (convert the database again)";
  }
  if (h.flags & FLAT_DELTA) {
    if (h.k > (uint32_t)MFX_MAX_K_NARROW) return "delta-coded blocks hold k <= 31";
    if (h.n / 4 > rest) return "k-mer count beyond the file's size";
  } else if (h.flags & FLAT_PACKED) {
    if (h.k > (uint32_t)MFX_MAX_K_PACKED) return "packed records hold k <= 21";
    if (h.n > rest / 8) return "k-mer count beyond the file's size";
  } else {
    const uint64_t per = (h.k > (uint32_t)MFX_MAX_K_NARROW ? 16u : 8u) + 4u;
    if (h.n > rest / per) return "k-mer count beyond the file's size";
  }
  if (h.n_escape > h.n) return "more escapes than k-mers";
  return nullptr;
}
// a k-mer of k <= 31 bases has no bit at or above 2k
inline bool flat_key_fits(uint64_t key, uint32_t k) { return k >= 32 || (key >> (2 * k)) == 0; }
// bits of a record's key: the k-mer's 2k, or the 2k + 3 of a placed record
inline uint32_t flat_rec_bits(const FlatHeader &h) { return (h.flags & FLAT_PLACED) ? (uint32_t)mfx_p_bits((int)h.k) : 2u * h.k; }
inline bool flat_rec_fits(uint64_t key, const FlatHeader &h) { const uint32_t b = flat_rec_bits(h); return b >= 64 || (key >> b) == 0; }

// ---- meryl stuffedBits reader (UNVALIDATED) -----------
// A stuffedBits file image: u64 dataBlockLenMax (bits), u32 dataBlocksLen,
// u32 dataBlocksMax, u64 bgn[dataBlocksLen], u64 len[dataBlocksLen] (bits),
// then ceil(len/64) little-endian u64 words per block; values are packed
// MSB-first inside each word.
struct BitReader {
  const uint64_t *w = nullptr;
  uint64_t nbits = 0, pos = 0;
  bool ok = true;
  uint64_t get(uint32_t n) {               // n <= 64
    if (n == 0) return 0;
    if (pos + n > nbits) { ok = false; return 0; }
    uint64_t wi = pos >> 6, bo = pos & 63, v;
    if (bo + n <= 64) {
      v = (w[wi] << bo) >> (64 - n);
    } else {
      uint32_t n1 = 64 - (uint32_t)bo, n2 = n - n1;
      v = (((w[wi] << bo) >> bo) << n2) | (w[wi + 1] >> (64 - n2));
    }
    pos += n;
    return v;
  }
  uint64_t unary() {                        // number of 0 bits before the next 1 (the 1 is consumed)
    uint64_t z = 0;
    while (true) {
      if (pos >= nbits) { ok = false; return 0; }
      uint64_t wi = pos >> 6, bo = pos & 63;
      uint64_t rest = w[wi] << bo;
      if (rest) {
        uint32_t lz = (uint32_t)__builtin_clzll(rest);
        z += lz;
        pos += lz + 1;
        return z;
      }
      z += 64 - bo;
      pos += 64 - bo;
    }
  }
};

const uint64_t MERYL_IDX_MAGIC1 = 0x646e496c7972656dULL;   // "merylInd"
const uint64_t MERYL_DAT_MAGIC1 = 0x7461446c7972656dULL;   // "merylDat"
const uint64_t MERYL_DAT_MAGIC2 = 0x0a3030656c694661ULL;   // "aFile00\n"

struct StuffedFile {
  std::vector<uint64_t> words;     // all block payloads, concatenated
  std::vector<uint64_t> blk_word;  // first word of each block
  std::vector<uint64_t> blk_bits;  // bit length of each block
};

// reads ONE stuffedBits image starting at the current file offset; returns
// false at clean EOF, sets *err on a malformed image.
bool read_stuffed(FILE *f, StuffedFile &out, std::string *err) {
  uint64_t lenmax;
  uint32_t nblk, maxblk;
  size_t r = fread(&lenmax, 8, 1, f);
  if (r != 1) return false;                                   // EOF
  if (fread(&nblk, 4, 1, f) != 1 || fread(&maxblk, 4, 1, f) != 1) { *err = "truncated stuffedBits header"; return false; }
  if (nblk == 0 || nblk > maxblk || maxblk > (1u << 24)) { *err = "implausible stuffedBits block count"; return false; }
  std::vector<uint64_t> bgn(nblk), len(nblk);
  if (fread(bgn.data(), 8, nblk, f) != nblk || fread(len.data(), 8, nblk, f) != nblk) { *err = "truncated stuffedBits tables"; return false; }
  out.words.clear(); out.blk_word.clear(); out.blk_bits.clear();
  for (uint32_t b = 0; b < nblk; ++b) {
    if (len[b] > lenmax) { *err = "stuffedBits block longer than its declared maximum"; return false; }
    uint64_t nw = (len[b] + 63) / 64;
    size_t at = out.words.size();
    out.words.resize(at + nw + 1);
    if (nw && fread(out.words.data() + at, 8, nw, f) != nw) { *err = "truncated stuffedBits payload"; return false; }
    out.words[at + nw] = 0;
    out.blk_word.push_back(at);
    out.blk_bits.push_back(len[b]);
  }
  return true;
}

struct MerylIndex {
  uint32_t prefixSize = 0, suffixSize = 0, numFilesBits = 0, numBlocksBits = 0, flags = 0;
  int version = 0;
  // statistics block that follows the sizes (merylHistogram, first three 64-bit fields)
  bool     has_stats = false;
  uint64_t numUnique = 0, numDistinct = 0, numTotal = 0;
};

// What one decoded .merylData file amounts to; summed over the 64 files it must reproduce the master
// index's statistics (conformance checks of SURVEY App. C, applied on every load).
struct MerylFileSums {
  uint64_t kmers = 0;      // sum of the block headers' nKmers
  uint64_t unique = 0;     // k-mers with value 1
  uint64_t total = 0;      // sum of the values
  uint64_t blocks = 0;
};

// MFX_MERYL_LENIENT=1 turns the statistics cross-check into a warning (the statistics layout is the least
// certain part of the recalled format); the structural checks always fail hard.
bool meryl_lenient() {
  const char *e = getenv("MFX_MERYL_LENIENT");
  return e && atoi(e) != 0;
}

int read_meryl_master(const std::string &dir, MerylIndex &mi) {
  std::string p = dir + "/merylIndex";
  FILE *f = fopen(p.c_str(), "rb");
  if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s'", p.c_str());
  StuffedFile sf;
  std::string err;
  bool ok = read_stuffed(f, sf, &err);
  fclose(f);
  if (!ok) return mfx_fail(MFX_E_FORMAT, "'%s': %s", p.c_str(), err.empty() ? "empty file" : err.c_str());
  BitReader br;
  br.w = sf.words.data() + sf.blk_word[0];
  br.nbits = sf.blk_bits[0];
  uint64_t m1 = br.get(64), m2 = br.get(64);
  if (m1 != MERYL_IDX_MAGIC1)
    return mfx_fail(MFX_E_FORMAT, "'%s': bad magic %016lx (not a meryl index)", p.c_str(), (unsigned long)m1);
  // "ex__v.0N": 0x3N302e765f5f7865
  if ((m2 & 0xf0ffffffffffffffULL) != 0x30302e765f5f7865ULL)
    return mfx_fail(MFX_E_FORMAT, "'%s': unrecognised index version word %016lx", p.c_str(), (unsigned long)m2);
  mi.version = (int)((m2 >> 56) & 0x0f);
  if (mi.version < 1 || mi.version > 9)
    return mfx_fail(MFX_E_FORMAT, "'%s': unsupported meryl index version %d", p.c_str(), mi.version);
  mi.prefixSize = (uint32_t)br.get(32);
  mi.suffixSize = (uint32_t)br.get(32);
  mi.numFilesBits = (uint32_t)br.get(32);
  mi.numBlocksBits = (uint32_t)br.get(32);
  if (mi.version >= 2) mi.flags = (uint32_t)br.get(32);
  if (!br.ok || mi.numFilesBits != 6 || mi.prefixSize < 6 || mi.prefixSize + mi.suffixSize == 0 ||
      ((mi.prefixSize + mi.suffixSize) & 1) || mi.prefixSize + mi.suffixSize > 128 ||
      mi.numFilesBits + mi.numBlocksBits != mi.prefixSize)
    return mfx_fail(MFX_E_FORMAT, "'%s': inconsistent sizes (prefix %u suffix %u files %u blocks %u)", p.c_str(),
                    mi.prefixSize, mi.suffixSize, mi.numFilesBits, mi.numBlocksBits);
  if (br.pos + 192 <= br.nbits) {
    mi.numUnique = br.get(64);
    mi.numDistinct = br.get(64);
    mi.numTotal = br.get(64);
    mi.has_stats = br.ok;
    if (mi.has_stats && (mi.numUnique > mi.numDistinct || mi.numDistinct > mi.numTotal)) {
      if (!meryl_lenient())
        return mfx_fail(MFX_E_FORMAT, "'%s': statistics are not ordered (unique %lu <= distinct %lu <= total %lu expected); "
                        "MFX_MERYL_LENIENT=1 skips the statistics checks", p.c_str(), (unsigned long)mi.numUnique,
                        (unsigned long)mi.numDistinct, (unsigned long)mi.numTotal);
      mi.has_stats = false;
    }
  }
  return MFX_OK;
}

// Σ over the 64 files against the master statistics: a decoder (or a database) that disagrees with itself must
// not load quietly.  with_values: the values were decoded too (a full load), not only the block headers.
int check_meryl_sums(const std::string &dir, const MerylIndex &mi, const std::vector<MerylFileSums> &per, bool with_values) {
  if (!mi.has_stats) return MFX_OK;
  MerylFileSums s;
  for (const auto &x : per) { s.kmers += x.kmers; s.unique += x.unique; s.total += x.total; }
  std::string why;
  char b[256];
  if (s.kmers != mi.numDistinct) {
    snprintf(b, sizeof(b), "the data blocks hold %lu k-mers, the index statistics say %lu distinct", (unsigned long)s.kmers, (unsigned long)mi.numDistinct);
    why = b;
  } else if (with_values && s.total != mi.numTotal) {
    snprintf(b, sizeof(b), "the values sum to %lu, the index statistics say %lu total", (unsigned long)s.total, (unsigned long)mi.numTotal);
    why = b;
  } else if (with_values && s.unique != mi.numUnique) {
    snprintf(b, sizeof(b), "%lu k-mers have value 1, the index statistics say %lu unique", (unsigned long)s.unique, (unsigned long)mi.numUnique);
    why = b;
  }
  if (why.empty()) return MFX_OK;
  if (meryl_lenient()) {
    fprintf(stderr, "WARNING: meryl database '%s': %s (MFX_MERYL_LENIENT=1: continuing).\n", dir.c_str(), why.c_str());
    return MFX_OK;
  }
  return mfx_fail(MFX_E_FORMAT, "meryl database '%s' is inconsistent: %s (a truncated copy, or a layout this decoder does not "
                  "know; MFX_MERYL_LENIENT=1 downgrades this to a warning)", dir.c_str(), why.c_str());
}

std::string meryl_file_name(const std::string &dir, uint32_t file, const char *ext) {
  char b[16];
  for (int i = 0; i < 6; ++i) b[i] = ((file >> (5 - i)) & 1) ? '1' : '0';
  b[6] = 0;
  return dir + "/0x" + b + ext;
}

// decode every block of one .merylData file; emit(kmer, value)
// count_only: stop after each block's header (the k-mer count lives there)
template <class F>
int read_meryl_data(const std::string &path, uint32_t file, const MerylIndex &mi, F &&emit, MerylFileSums *sums, bool count_only = false) {
  FILE *f = fopen(path.c_str(), "rb");
  // meryl writes all 64 data files, empty pieces included: a missing one means a truncated / partially copied
  // database, which must not load as "no k-mers here"
  if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s': a meryl database has all 64 data files (partial copy?)", path.c_str());
  StuffedFile sf;
  std::string err;
  int rc = MFX_OK;
  bool have_prev = false;
  uint64_t prev_prefix = 0;
  while (rc == MFX_OK && read_stuffed(f, sf, &err)) {
    // a data block may be split over several stuffedBits chunks; treat them as one bit stream
    std::vector<uint64_t> stream;
    uint64_t bits = 0;
    bool aligned = true;
    for (size_t b = 0; b < sf.blk_word.size(); ++b) {
      if (!aligned) { rc = mfx_fail(MFX_E_FORMAT, "'%s': non-word-aligned interior chunk", path.c_str()); break; }
      uint64_t nw = (sf.blk_bits[b] + 63) / 64;
      stream.insert(stream.end(), sf.words.begin() + sf.blk_word[b], sf.words.begin() + sf.blk_word[b] + nw);
      bits += sf.blk_bits[b];
      aligned = (sf.blk_bits[b] % 64) == 0;
    }
    if (rc) break;
    stream.push_back(0);
    BitReader br;
    br.w = stream.data();
    br.nbits = bits;
    if (br.get(64) != MERYL_DAT_MAGIC1 || br.get(64) != MERYL_DAT_MAGIC2) { rc = mfx_fail(MFX_E_FORMAT, "'%s': bad data-block magic", path.c_str()); break; }
    uint64_t prefix = br.get(64), nk = br.get(64);
    uint32_t kcode = (uint32_t)br.get(8), ubits = (uint32_t)br.get(32), bbits = (uint32_t)br.get(32);
    (void)br.get(64);                                        // k1 (unused)
    uint32_t ccode = (uint32_t)br.get(8);
    (void)br.get(64); (void)br.get(64);                      // c1, c2 (unused)
    if (!br.ok || kcode != 1 || (ccode != 1 && ccode != 2) || ubits + bbits != mi.suffixSize || bbits > 128 ||
        (prefix >> mi.numBlocksBits) != file || mi.suffixSize > 122) {
      rc = mfx_fail(MFX_E_FORMAT, "'%s': unsupported / inconsistent data block (kCode %u cCode %u unary %u binary %u suffix %u prefix %lx)",
                    path.c_str(), kcode, ccode, ubits, bbits, mi.suffixSize, (unsigned long)prefix);
      break;
    }
    // blocks appear in increasing prefix order, so the k-mers of a file are strictly increasing across blocks too
    if (have_prev && prefix <= prev_prefix) {
      rc = mfx_fail(MFX_E_FORMAT, "'%s': block prefixes not strictly increasing (%lx after %lx)", path.c_str(), (unsigned long)prefix, (unsigned long)prev_prefix);
      break;
    }
    have_prev = true;
    prev_prefix = prefix;
    if (mi.prefixSize < 64 && (prefix >> mi.prefixSize) != 0) {      // prefixSize >= 64: every 64-bit prefix fits (and the shift would be undefined)
      rc = mfx_fail(MFX_E_FORMAT, "'%s': block prefix %lx wider than %u bits", path.c_str(), (unsigned long)prefix, mi.prefixSize);
      break;
    }
    sums->blocks++;
    // a k-mer of the block takes at least one bit of unary code, its binary part and its count: a header that claims more
    // k-mers than the block has bits for is damaged (and must not size an allocation)
    if (nk > (br.nbits - br.pos) / (1ull + bbits + (ccode == 1 ? 32u : 64u))) {
      rc = mfx_fail(MFX_E_FORMAT, "'%s': a data block of %lu bits claims %lu k-mers", path.c_str(), (unsigned long)br.nbits, (unsigned long)nk);
      break;
    }
    if (count_only) { sums->kmers += nk; continue; }
    std::vector<u128> sfx(nk);
    u128 hi = 0;
    for (uint64_t i = 0; i < nk; ++i) {
      hi += br.unary();
      // the binary part is read in two pieces when it is wider than a word (k > 32 + prefix bits)
      u128 bin = bbits > 64 ? (((u128)br.get(bbits - 64) << 64) | br.get(64)) : (u128)br.get(bbits);
      sfx[i] = (bbits >= 128 ? (u128)0 : (hi << bbits)) | bin;
      if (i && sfx[i] <= sfx[i - 1]) { rc = mfx_fail(MFX_E_FORMAT, "'%s': suffixes not strictly increasing", path.c_str()); break; }
    }
    if (rc) break;
    const u128 smask = ((u128)1 << mi.suffixSize) - 1;          // suffixSize <= 122
    if (nk && (sfx[nk - 1] & ~smask)) { rc = mfx_fail(MFX_E_FORMAT, "'%s': suffix wider than %u bits", path.c_str(), mi.suffixSize); break; }
    uint64_t uniq = 0, tot = 0;
    for (uint64_t i = 0; i < nk; ++i) {
      uint64_t v = br.get(ccode == 1 ? 32 : 64);
      const u128 km = ((u128)prefix << mi.suffixSize) | sfx[i];
      uniq += (v == 1);
      tot += v;
      emit((uint64_t)km, (uint64_t)(km >> 64), v > 0xffffffffull ? 0xffffffffu : (uint32_t)v);
    }
    if (!br.ok) { rc = mfx_fail(MFX_E_FORMAT, "'%s': data block shorter than its header claims", path.c_str()); break; }
    sums->kmers += nk;
    sums->unique += uniq;
    sums->total += tot;
  }
  fclose(f);
  if (rc == MFX_OK && !err.empty()) rc = mfx_fail(MFX_E_FORMAT, "'%s': %s", path.c_str(), err.c_str());
  return rc;
}

// The 64 files of a meryl database are independent: decode them on the host threads the library may use.
// fn(file) returns MFX_OK or a failure whose message is in the CALLING thread's mfx_last_error(); the first
// failure (lowest file number wins) is re-raised on this thread.
template <class F>
int for_each_meryl_file(F &&fn) {
  const unsigned nt = std::max(1u, std::min(64u, (unsigned)mfx_host_threads()));
  std::atomic<uint32_t> next(0);
  std::mutex emu;
  int bad_rc = MFX_OK;
  uint32_t bad_file = 64;
  std::string bad_msg;
  auto work = [&]() {
    for (uint32_t fl; (fl = next.fetch_add(1)) < 64;) {
      int rc;
      try { rc = fn(fl); }                                     // (nothing may leave a worker thread -- or the C ABI -- as an exception)
      catch (const std::bad_alloc &) { rc = mfx_fail(MFX_E_NOMEM, "meryl data file %u: out of memory", fl); }
      catch (const std::exception &e) { rc = mfx_fail(MFX_E_FORMAT, "meryl data file %u: %s", fl, e.what()); }
      if (rc != MFX_OK) {
        std::lock_guard<std::mutex> g(emu);
        if (fl < bad_file) { bad_file = fl; bad_rc = rc; bad_msg = mfx_last_error(); }
      }
    }
  };
  if (nt == 1) work();
  else {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(work);
    for (auto &x : th) x.join();
  }
  return bad_rc == MFX_OK ? MFX_OK : mfx_fail(bad_rc, "%s", bad_msg.c_str());
}

int detect(const std::string &path) {
  if (is_dir(path)) return MFX_DB_MERYL;
  if (!is_file(path)) return 0;
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return 0;
  char m[8] = {0};
  size_t r = fread(m, 1, 8, f);
  fclose(f);
  if (r == 8 && memcmp(m, "MFXKMER1", 8) == 0) return MFX_DB_FLAT;
  return MFX_DB_TEXT;
}

// batches (kmer,value) pairs into the index
struct Feeder {
  mfx_index *const *ixs;               // one table, or the shards of one process: every batch goes to all of them
  uint32_t nix;
  int side;
  uint64_t minV, maxV;
  std::mutex *mu = nullptr;            // several decoder threads feed one index: inserts are serialised
  std::vector<uint64_t> k;             // 1 word per k-mer, 2 (low, high) when the index holds k > 31
  std::vector<uint32_t> v;
  int rc = MFX_OK;
  void flush() {
    if (v.empty() || rc) return;
    std::unique_lock<std::mutex> lk;
    if (mu) lk = std::unique_lock<std::mutex>(*mu);
    const bool timing = getenv("MFX_DB_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    rc = mfx_index_add_multi(ixs, nix, k.data(), v.data(), v.size(), side, minV, maxV);
    if (timing) fprintf(stderr, "[mfx db] batch of %zu k-mers inserted in %.1f ms\n", v.size(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
    k.clear(); v.clear();
  }
  void push(uint64_t lo, uint64_t hi, uint32_t val) {
    k.push_back(lo);
    if (ixs[0]->wide()) k.push_back(hi);
    v.push_back(val);
    if (v.size() >= (1u << 24)) flush();
  }
};

// One line of `meryl print` text at [p, end): "<kmer>\t<count>".  Returns 1 = k-mer parsed, 0 = blank line, -1 = malformed.
inline int parse_text_line(const char *p, const char *end, u128 &km, int &n, unsigned long long &v) {
  km = 0;
  n = 0;
  while (p < end && base_code((unsigned char)*p) >= 0) { km = (km << 2) | (u128)base_code((unsigned char)*p); ++p; ++n; }
  if (n == 0 && (p == end || *p == '\n' || *p == '\r')) return 0;
  if (n == 0 || n > MFX_MAX_K || p == end || (*p != '\t' && *p != ' ')) return -1;
  while (p < end && (*p == '\t' || *p == ' ')) ++p;
  if (p == end || *p < '0' || *p > '9') return -1;
  v = 0;
  while (p < end && *p >= '0' && *p <= '9') { v = v > (~0ull - 9) / 10 ? ~0ull : v * 10 + (unsigned)(*p - '0'); ++p; }
  return 1;
}

template <class F>
int scan_text(const std::string &path, int *k_out, F &&emit, uint64_t *count) {
  mfx_file h = mfx_open_reader(path.c_str());          // compressedFileReader: decompressor chosen by suffix, no shell
  FILE *f = h.f;
  if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s'", path.c_str());
  char line[512];
  int k = 0, rc = MFX_OK;
  uint64_t ln = 0;
  while (fgets(line, sizeof(line), f)) {
    ++ln;
    u128 km;
    int n;
    unsigned long long v = 0;
    const int what = parse_text_line(line, line + strlen(line), km, n, v);
    if (what == 0) continue;
    if (what < 0) { rc = mfx_fail(MFX_E_FORMAT, "'%s' line %lu: expected '<kmer>\\t<count>'", path.c_str(), (unsigned long)ln); break; }
    if (k == 0) k = n;
    if (n != k) { rc = mfx_fail(MFX_E_FORMAT, "'%s' line %lu: k-mer length %d differs from %d", path.c_str(), (unsigned long)ln, n, k); break; }
    emit((uint64_t)km, (uint64_t)(km >> 64), v > 0xffffffffull ? 0xffffffffu : (uint32_t)v);
    ++*count;
  }
  if (mfx_close(h, rc != MFX_OK) && rc == MFX_OK)
    rc = mfx_fail(MFX_E_IO, "reading '%s' failed (stream error or the decompressor exited with an error)", path.c_str());
  if (k_out) *k_out = k;
  return rc;
}

// An UNCOMPRESSED `meryl print` file parsed by the host threads: the file is cut into 32 MB pieces, a piece belongs to
// the thread that draws it and covers the lines that START in it (pread of the piece plus the tail of its last
// line).  make(t) returns thread t's sink: sink(lo, hi, v) per k-mer, sink.done() once (its return value is the
// thread's status).  A 6 G-line database (150 GB of text) is minutes of single-threaded fgets otherwise.
// on_piece(t, pc), if given, tells that thread t starts piece pc (a sink that wants the file's order back collects by piece).
inline uint64_t text_piece_bytes() {
  uint64_t PIECE = 32ull << 20;
  if (const char *e = getenv("MFX_TEXT_PIECE")) { const long v = atol(e); if (v >= 64) PIECE = (uint64_t)v; }   // tests: many pieces of a small file
  return PIECE;
}

template <class Make>
int scan_text_parallel(const std::string &path, int *k_out, uint64_t *count, Make &&make,
                       const std::function<void(unsigned, uint64_t)> &on_piece = nullptr) {
  const int fd = open(path.c_str(), O_RDONLY);
  struct stat st;
  if (fd < 0 || fstat(fd, &st) != 0) { if (fd >= 0) close(fd); return mfx_fail(MFX_E_IO, "cannot open '%s'", path.c_str()); }
  const uint64_t PIECE = text_piece_bytes();
  const uint64_t size = (uint64_t)st.st_size, TAIL = 4096;
  const uint64_t npieces = (size + PIECE - 1) / PIECE;
  const unsigned nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({npieces, 64, (uint64_t)mfx_host_threads()}));
  std::atomic<uint64_t> next(0), total(0);
  std::atomic<int> kk(0);
  std::mutex emu;
  int bad_rc = MFX_OK;
  uint64_t bad_at = ~0ull;
  std::string bad_msg;
  auto fail_at = [&](uint64_t at, int rc, const std::string &msg) {
    std::lock_guard<std::mutex> g(emu);
    if (at < bad_at) { bad_at = at; bad_rc = rc; bad_msg = msg; }
  };
  auto work = [&](unsigned t) {
    auto sink = make(t);
    std::vector<char> buf(PIECE + TAIL + 1);
    uint64_t mine = 0;
    for (uint64_t pc; (pc = next.fetch_add(1)) < npieces;) {
      { std::lock_guard<std::mutex> g(emu); if (bad_rc != MFX_OK) break; }
      if (on_piece) on_piece(t, pc);
      const uint64_t b = pc * PIECE, want = std::min(size - (b ? b - 1 : 0), PIECE + TAIL + (b ? 1 : 0));
      // one byte before the piece tells whether a line starts exactly at b
      const uint64_t from = b ? b - 1 : 0;
      uint64_t got = 0;
      while (got < want) {
        ssize_t r = pread(fd, buf.data() + got, want - got, (off_t)(from + got));
        if (r <= 0) break;
        got += (uint64_t)r;
      }
      if (got < want) { fail_at(b, MFX_E_IO, "reading '" + path + "' failed"); break; }
      const char *p = buf.data(), *end = buf.data() + got;
      const char *lim = buf.data() + std::min<uint64_t>(got, (b ? 1 : 0) + PIECE);     // lines starting before lim are this piece's
      if (b) {                                               // skip the line that started in the previous piece
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        p = nl ? nl + 1 : end;
      }
      while (p < lim) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        const char *le = nl ? nl : end;
        if (!nl && from + got < size) { fail_at(from + (uint64_t)(p - buf.data()), MFX_E_FORMAT, "'" + path + "': a line longer than 4096 bytes"); break; }
        u128 km;
        int n;
        unsigned long long v;
        const int what = parse_text_line(p, le, km, n, v);
        if (what < 0) {
          char where[64];
          snprintf(where, sizeof(where), "%lu", (unsigned long)(from + (uint64_t)(p - buf.data())));
          fail_at(from + (uint64_t)(p - buf.data()), MFX_E_FORMAT, "'" + path + "' at byte " + where + ": expected '<kmer>\\t<count>'");
          break;
        }
        if (what > 0) {
          int k0 = kk.load(std::memory_order_relaxed);          // (a CAS per line would bounce the cache line between all threads)
          if (k0 == 0) kk.compare_exchange_strong(k0, n);
          if (k0 != 0 && k0 != n) {
            char msg[160];
            snprintf(msg, sizeof(msg), "' at byte %lu: k-mer length %d differs from %d", (unsigned long)(from + (uint64_t)(p - buf.data())), n, k0);
            fail_at(from + (uint64_t)(p - buf.data()), MFX_E_FORMAT, "'" + path + msg);
            break;
          }
          sink((uint64_t)km, (uint64_t)(km >> 64), v > 0xffffffffull ? 0xffffffffu : (uint32_t)v);
          ++mine;
        }
        p = le + 1;
      }
    }
    const int rc = sink.done();
    if (rc != MFX_OK) fail_at(~0ull - 1, rc, mfx_last_error());
    total.fetch_add(mine);
  };
  if (nt == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(work, t);
    for (auto &x : th) x.join();
  }
  close(fd);
  if (k_out) *k_out = kk.load();
  if (count) *count = total.load();
  return bad_rc == MFX_OK ? MFX_OK : mfx_fail(bad_rc, "%s", bad_msg.c_str());
}

inline bool text_is_plain(const std::string &path) { return mfx_suffix_tool(path) == nullptr; }


// ---- delta-coded flat form ---------------------------------------------------
struct DeltaBlockPlan { uint8_t kb = 0, vb = 2; uint32_t nesc = 0; uint64_t bytes = 0; };

// widths and size of block [b, b + cnt) of a strictly ascending database: the rule itself is mfx_delta.h, shared with the encoder kernels
DeltaBlockPlan plan_delta_block(const uint64_t *kmers, const uint32_t *values, uint32_t cnt) {
  DeltaBlockPlan p;
  uint64_t maxd = 0;
  for (uint32_t i = 1; i < cnt; ++i) maxd = std::max(maxd, kmers[i] - kmers[i - 1]);
  p.kb = (uint8_t)mfx_bit_length(maxd);
  uint32_t hist[MFX_DELTA_VBINS] = {0};                       // bit length of value + 1: a value fits vb bits iff that is <= vb
  for (uint32_t i = 0; i < cnt; ++i) ++hist[mfx_delta_vbin(values[i])];
  uint32_t vb, nesc;
  mfx_delta_vbits(hist, cnt, vb, nesc);
  p.vb = (uint8_t)vb;
  p.nesc = nesc;
  p.bytes = mfx_delta_bytes(cnt, p.kb, p.vb);
  return p;
}

void put_bits(uint64_t *w, uint64_t bit, uint32_t nbits, uint64_t x) {       // into zeroed words
  const uint64_t i = bit >> 6;
  const uint32_t sh = (uint32_t)bit & 63u;
  w[i] |= x << sh;
  if (sh + nbits > 64u) w[i + 1] |= x >> (64u - sh);
}

void pack_delta_block(const uint64_t *kmers, const uint32_t *values, uint32_t cnt, const DeltaBlockPlan &p, uint64_t *out) {
  memset(out, 0, p.bytes);
  for (uint32_t i = 1; i < cnt; ++i) if (p.kb) put_bits(out, (uint64_t)(i - 1) * p.kb, p.kb, kmers[i] - kmers[i - 1]);
  uint64_t *vw = out + ((uint64_t)(cnt - 1) * p.kb + 63) / 64;
  const uint32_t esc = (1u << p.vb) - 1u;
  for (uint32_t i = 0; i < cnt; ++i) put_bits(vw, (uint64_t)i * p.vb, p.vb, values[i] >= esc ? esc : values[i]);
}

template <class F>
void par_blocks(uint64_t nblocks, F &&fn) {                   // fn(b) for every block, on the library's host threads
  const unsigned nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({(nblocks + 255) / 256, 64, (uint64_t)mfx_host_threads()}));
  if (nt == 1) { for (uint64_t b = 0; b < nblocks; ++b) fn(b); return; }
  std::atomic<uint64_t> nextb{0};
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([&]() {
      for (uint64_t b0 = nextb.fetch_add(256); b0 < nblocks; b0 = nextb.fetch_add(256))
        for (uint64_t b = b0; b < std::min(nblocks, b0 + 256); ++b) fn(b);
    });
  for (auto &x : th) x.join();
}

// 0 = written; 1 = the k-mers are not strictly ascending (the caller writes another form); < 0: error
// placed: `kmers` are the numbers P of mfx_place.h (ascending); the escape list then holds the k-mers they decode to
// sbits (placed, k = 31: mfx_place.h, mfx_p_split): the strand bit of every record; `kmers` are then the numbers P >> 1 -- ascending, equal for a
// pair that differs in the strand bit alone (0 first) -- and a record's count field holds count << 1 | s (a count of 2^21 or more is an escape)
int write_flat_delta(FILE *f, const char *path, FlatHeader h, const uint64_t *kmers, const uint32_t *true_values, uint64_t n, bool placed = false,
                     const uint8_t *sbits = nullptr) {
  std::vector<uint32_t> folded;
  if (sbits) {
    folded.resize(n);
    par_blocks((n + 65535) / 65536, [&](uint64_t b) {
      for (uint64_t i = b * 65536, e = std::min<uint64_t>(n, i + 65536); i < e; ++i)
        folded[i] = true_values[i] >= (1u << (MFX_DELTA_MAX_VBITS - 1)) ? 0xffffffffu : (true_values[i] << 1) | (uint32_t)(sbits[i] & 1u);
    });
  }
  const uint32_t *values = sbits ? folded.data() : true_values;
  const uint64_t nblocks = (n + MFX_DELTA_BLOCK - 1) / MFX_DELTA_BLOCK;
  auto cnt_of = [&](uint64_t b) { return (uint32_t)std::min<uint64_t>(MFX_DELTA_BLOCK, n - b * MFX_DELTA_BLOCK); };
  const bool timing = getenv("MFX_DB_TIMING") != nullptr;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double tw0 = now();
  double t_pack = 0, t_io = 0;
  std::vector<DeltaBlockPlan> plan(nblocks);
  std::atomic<int> unsorted{0};
  par_blocks(nblocks, [&](uint64_t b) {
    const uint64_t o = b * MFX_DELTA_BLOCK;
    const uint32_t cnt = cnt_of(b);
    for (uint32_t i = (b ? 0 : 1); i < cnt; ++i)
      if (kmers[o + i] < kmers[o + i - 1] || (kmers[o + i] == kmers[o + i - 1] && !(sbits && sbits[o + i - 1] < sbits[o + i]))) { unsorted = 1; return; }
    plan[b] = plan_delta_block(kmers + o, values + o, cnt);
  });
  if (unsorted) return 1;
  const double tw1 = now();
  std::vector<uint64_t> dir(2 * (nblocks + 1));
  uint64_t at = sizeof(FlatHeader) + 8 + dir.size() * 8;
  h.n_escape = 0;
  for (uint64_t b = 0; b < nblocks; ++b) {
    dir[2 * b] = kmers[b * MFX_DELTA_BLOCK];
    dir[2 * b + 1] = at | ((uint64_t)plan[b].kb << 48) | ((uint64_t)plan[b].vb << 56);
    at += plan[b].bytes;
    h.n_escape += plan[b].nesc;
  }
  dir[2 * nblocks] = 0;
  dir[2 * nblocks + 1] = at;
  if (at >> 48) return mfx_fail(MFX_E_INVAL, "mfx_db_write_flat: the database is too large for the delta form");
  h.flags |= FLAT_DELTA;
  if (placed) h.flags |= FLAT_PLACED | (MFX_PLACE_VERSION << 8);
  bool ok = fwrite(&h, sizeof(h), 1, f) == 1 && fwrite(&nblocks, 8, 1, f) == 1 && fwrite(dir.data(), 8, dir.size(), f) == dir.size();
  // the blocks, packed by all threads a piece (<= 256 MB) at a time
  std::vector<uint64_t> buf;
  for (uint64_t b0 = 0; b0 < nblocks && ok;) {
    uint64_t b1 = b0, bytes = 0;
    while (b1 < nblocks && (b1 == b0 || bytes + plan[b1].bytes <= (256ull << 20))) bytes += plan[b1++].bytes;
    buf.resize(bytes / 8);
    const uint64_t base = dir[2 * b0 + 1] & 0xffffffffffffull;
    const double tp0 = now();
    par_blocks(b1 - b0, [&](uint64_t i) {
      const uint64_t b = b0 + i;
      pack_delta_block(kmers + b * MFX_DELTA_BLOCK, values + b * MFX_DELTA_BLOCK, cnt_of(b), plan[b],
                       buf.data() + ((dir[2 * b + 1] & 0xffffffffffffull) - base) / 8);
    });
    const double tp1 = now();
    ok = fwrite(buf.data(), 8, buf.size(), f) == buf.size();
    t_pack += tp1 - tp0; t_io += now() - tp1;
    b0 = b1;
  }
  // the escapes: the counts that did not fit their block's field
  std::vector<uint64_t> ek;
  std::vector<uint32_t> ev;
  for (uint64_t b = 0; b < nblocks; ++b) {
    if (!plan[b].nesc) continue;
    const uint32_t esc = (1u << plan[b].vb) - 1u;
    for (uint64_t i = b * MFX_DELTA_BLOCK, e = i + cnt_of(b); i < e; ++i)
      if (values[i] >= esc) {
        uint32_t top, hi, pm;
        ek.push_back(placed ? mfx_p_decode_s((int)h.k, kmers[i], sbits ? sbits[i] : 0u, top, hi, pm) : kmers[i]);
        ev.push_back(true_values[i]);
      }
  }
  ok = ok && ek.size() == h.n_escape &&
       (ek.empty() || (fwrite(ek.data(), 8, ek.size(), f) == ek.size() && fwrite(ev.data(), 4, ev.size(), f) == ev.size()));
  if (timing) fprintf(stderr, "[mfx db] delta writer: plan %.2f s, pack %.2f s, write %.2f s, all %.2f s (%lu blocks)\n", tw1 - tw0, t_pack, t_io, now() - tw0,
                      (unsigned long)nblocks);
  return ok ? 0 : mfx_fail(MFX_E_IO, "short write to '%s'", path);
}

// the escape list of a packed / delta-coded file (n_escape was bounded by the file's size: flat_header_problem)
int load_flat_escapes(mfx_index *const *ixs, uint32_t nix, int fd, const char *path, const FlatHeader &h, uint64_t at, int side,
                      uint64_t minV, uint64_t maxV) {
  std::vector<uint64_t> ek;
  std::vector<uint32_t> ev;
  try { ek.resize(h.n_escape); ev.resize(h.n_escape); }
  catch (const std::exception &) { return mfx_fail(MFX_E_NOMEM, "'%s': no memory for %lu escapes", path, (unsigned long)h.n_escape); }
  if (pread(fd, ek.data(), h.n_escape * 8, (off_t)at) != (ssize_t)(h.n_escape * 8) ||
      pread(fd, ev.data(), h.n_escape * 4, (off_t)(at + h.n_escape * 8)) != (ssize_t)(h.n_escape * 4))
    return mfx_fail(MFX_E_IO, "reading '%s' failed", path);
  for (uint64_t i = 0; i < h.n_escape; ++i)
    if (!flat_key_fits(ek[i], h.k)) return mfx_fail(MFX_E_FORMAT, "'%s': an escaped k-mer is wider than 2k bits", path);
  return mfx_index_add_multi(ixs, nix, ek.data(), ev.data(), h.n_escape, side, minV, maxV);
}

// the block directory of a delta-coded file, read and checked; *expect_out: where the blocks end (the escape list follows)
int read_delta_directory(int fd, const char *path, const FlatHeader &h, uint64_t fsize, std::vector<uint64_t> &dir, uint64_t *nblocks_out,
                         uint64_t *expect_out) {
  auto bad = [&](const char *what) { return mfx_fail(MFX_E_FORMAT, "'%s': %s", path, what); };
  uint64_t nblocks = 0;
  if (h.k > (uint32_t)MFX_MAX_K_NARROW || fsize < sizeof(h) + 8 || pread(fd, &nblocks, 8, sizeof(h)) != 8) return bad("truncated delta-coded payload");
  if (nblocks != (h.n + MFX_DELTA_BLOCK - 1) / MFX_DELTA_BLOCK) return bad("block count does not match the k-mer count");
  const uint64_t dir_off = sizeof(h) + 8, dir_bytes = (nblocks + 1) * 16;
  if (fsize < dir_off + dir_bytes) return bad("truncated block directory");
  try { dir.resize(2 * (nblocks + 1)); } catch (const std::exception &) { return mfx_fail(MFX_E_NOMEM, "'%s': no memory for %lu directory entries", path, (unsigned long)nblocks); }
  for (uint64_t o = 0; o < dir_bytes;) {
    const ssize_t r = pread(fd, (char *)dir.data() + o, dir_bytes - o, (off_t)(dir_off + o));
    if (r <= 0) return mfx_fail(MFX_E_IO, "reading '%s' failed", path);
    o += (uint64_t)r;
  }
  // the directory is checked before anything reads by it: offsets ascending, 8-byte aligned, inside the file, and every
  // block exactly as long as its widths say
  uint64_t expect = dir_off + dir_bytes;
  for (uint64_t b = 0; b <= nblocks; ++b) {
    const uint64_t off = dir[2 * b + 1] & 0xffffffffffffull;
    if (off != expect) return bad("inconsistent block directory");
    if (b == nblocks) break;
    const uint32_t kb = (uint32_t)(dir[2 * b + 1] >> 48) & 0xffu, vb = (uint32_t)(dir[2 * b + 1] >> 56) & 0xffu;
    const uint64_t cnt = std::min<uint64_t>(MFX_DELTA_BLOCK, h.n - b * MFX_DELTA_BLOCK);
    if (kb > flat_rec_bits(h) || vb < 2u || vb > (uint32_t)MFX_DELTA_MAX_VBITS) return bad("block field widths out of range");
    if (!flat_rec_fits(dir[2 * b], h)) return bad("a block's first k-mer is wider than 2k bits");
    // (the k-mers inside a block exist only in the kernel that decodes them: it refuses what is wider than 2k bits, index meta[4])
    if (b + 1 < nblocks && dir[2 * (b + 1)] <= dir[2 * b]) return bad("block directory not ascending");
    expect = off + (((cnt - 1) * kb + 63) / 64 + (cnt * vb + 63) / 64) * 8;
    if (expect > fsize) return bad("truncated delta-coded payload");
  }
  if (expect > fsize || fsize - expect < h.n_escape * 12) return bad("truncated delta-coded payload");
  *nblocks_out = nblocks;
  *expect_out = expect;
  return MFX_OK;
}

int load_flat_delta(mfx_index *const *ixs, uint32_t nix, int fd, const char *path, const FlatHeader &h, uint64_t fsize, int side,
                    uint64_t minV, uint64_t maxV) {
  std::vector<uint64_t> dir;
  uint64_t nblocks = 0, expect = 0;
  int rc = read_delta_directory(fd, path, h, fsize, dir, &nblocks, &expect);
  if (rc) return rc;
  if (h.n) rc = mfx_index_add_delta_file(ixs, nix, fd, path, dir.data(), nblocks, h.n, side, minV, maxV, (h.flags & FLAT_PLACED) ? 1 : 0);
  if (rc == MFX_OK && h.n_escape) rc = load_flat_escapes(ixs, nix, fd, path, h, expect, side, minV, maxV);
  return rc;
}

}  // namespace

// ---- for the staged load (mfx_api.cpp: mfx_db_stage) ----------------------------------------------------------------------
// opens `path` if it is a delta-coded flat database and reads + checks its directory; MFX_E_FORMAT with *fd_out = -1 when it is
// another kind of database (the caller then takes the ordinary load)
int mfx_flat_delta_open(const char *path, int *fd_out, mfx_flat_delta_info *info, std::vector<uint64_t> &dir) {
  *fd_out = -1;
  if (detect(std::string(path)) != MFX_DB_FLAT) return mfx_fail(MFX_E_FORMAT, "'%s' is not a flat k-mer file", path);
  int fd = open(path, O_RDONLY);
  struct stat st;
  if (fd < 0 || fstat(fd, &st) != 0) { if (fd >= 0) close(fd); return mfx_fail(MFX_E_IO, "cannot open '%s'", path); }
  FlatHeader h;
  if ((uint64_t)st.st_size < sizeof(h) || pread(fd, &h, sizeof(h), 0) != (ssize_t)sizeof(h)) { close(fd); return mfx_fail(MFX_E_FORMAT, "'%s': truncated header", path); }
  if (const char *why = flat_header_problem(h, (uint64_t)st.st_size)) { close(fd); return mfx_fail(MFX_E_FORMAT, "'%s': %s", path, why); }
  if (!(h.flags & FLAT_DELTA)) { close(fd); return mfx_fail(MFX_E_FORMAT, "'%s' is not delta-coded", path); }
  uint64_t nblocks = 0, expect = 0;
  if (int rc = read_delta_directory(fd, path, h, (uint64_t)st.st_size, dir, &nblocks, &expect)) { close(fd); return rc; }
  info->k = (int)h.k;
  info->placed = (h.flags & FLAT_PLACED) ? 1 : 0;
  info->n = h.n;
  info->n_escape = h.n_escape;
  info->nblocks = nblocks;
  info->escapes_off = expect;
  info->fsize = (uint64_t)st.st_size;
  *fd_out = fd;
  return MFX_OK;
}

// merylFileReader(path): opens the DB and reveals k (merfin-globals.C:118-119:
// "Make readDB first so we know the k size").
static int mfx_db_probe_impl(const char *path, mfx_db_info *out) {
  if (!path || !out) return mfx_fail(MFX_E_INVAL, "mfx_db_probe: null argument");
  memset(out, 0, sizeof(*out));
  std::string p(path);
  int fmt = detect(p);
  if (!fmt) return mfx_fail(MFX_E_IO, "k-mer database '%s' does not exist", path);
  out->format = fmt;
  if (fmt == MFX_DB_FLAT) {
    FILE *f = fopen(path, "rb");
    FlatHeader h;
    if (!f || fread(&h, sizeof(h), 1, f) != 1) { if (f) fclose(f); return mfx_fail(MFX_E_FORMAT, "'%s': truncated header", path); }
    fclose(f);
    out->k = (int)h.k;
    out->n_kmers = h.n;
    out->placed = (memcmp(h.magic, "MFXKMER1", 8) == 0 && (h.flags & FLAT_PLACED)) ? 1 : 0;
    return MFX_OK;
  }
  if (fmt == MFX_DB_TEXT) {
    uint64_t n = 0;
    int k = 0;
    struct Count { void operator()(uint64_t, uint64_t, uint32_t) {} int done() { return MFX_OK; } };
    int rc = text_is_plain(p) ? scan_text_parallel(p, &k, &n, [](unsigned) { return Count(); })
                              : scan_text(p, &k, [](uint64_t, uint64_t, uint32_t) {}, &n);
    if (rc) return rc;
    if (k == 0) return mfx_fail(MFX_E_FORMAT, "'%s': no k-mers found", path);
    out->k = k;
    out->n_kmers = n;
    return MFX_OK;
  }
  MerylIndex mi;
  int rc = read_meryl_master(p, mi);
  if (rc) return rc;
  out->k = (int)((mi.prefixSize + mi.suffixSize) / 2);
  // distinct k-mer count: sum of the block headers (cheap pass over the 64 data files)
  std::vector<MerylFileSums> per(64);
  rc = for_each_meryl_file([&](uint32_t fl) {
    return read_meryl_data(meryl_file_name(p, fl, ".merylData"), fl, mi, [](uint64_t, uint64_t, uint32_t) {}, &per[fl], true);
  });
  uint64_t n = 0;
  for (const auto &x : per) n += x.kmers;
  out->n_kmers = n;
  if (rc == MFX_OK) rc = check_meryl_sums(p, mi, per, false);
  return rc;
}

extern "C" int mfx_db_probe(const char *path, mfx_db_info *out) {
  try { return mfx_db_probe_impl(path, out); }                       // (nothing leaves the C ABI as an exception)
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_probe: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_probe: %s", e.what()); }
}


// merylExactLookup::load (merfin-globals.C:156,159): side 0 = read DB with the
// -min/-max filter, side 1 = assembly DB.
extern "C" int mfx_index_load_db(mfx_index *ix, const char *path, int side, uint64_t minV, uint64_t maxV) {
  if (!ix) return mfx_fail(MFX_E_INVAL, "mfx_index_load_db: null argument");
  return mfx_index_load_db_multi(&ix, 1, path, side, minV, maxV);
}

// One pass over the database feeds nix tables: the shards of one process each keep the k-mers they own
// (mfx_index_set_shard), so a config-5-sized read database is decoded ONCE, not once per GPU.
static int mfx_index_load_db_multi_impl(mfx_index *const *ixs, uint32_t nix, const char *path, int side, uint64_t minV, uint64_t maxV) {
  if (!ixs || nix == 0 || !path) return mfx_fail(MFX_E_INVAL, "mfx_index_load_db: null argument");
  for (uint32_t i = 0; i < nix; ++i)
    if (!ixs[i] || ixs[i]->k != ixs[0]->k) return mfx_fail(MFX_E_INVAL, "mfx_index_load_db_multi: the indexes of one load must hold the same k");
  mfx_index *ix = ixs[0];
  std::string p(path);
  int fmt = detect(p);
  if (!fmt) return mfx_fail(MFX_E_IO, "k-mer database '%s' does not exist", path);
  Feeder fd{ixs, nix, side, minV, maxV};
  uint64_t n = 0;
  int rc = MFX_OK;
  if (fmt == MFX_DB_FLAT) {
    // Several threads pread() slices of the file straight into the index's pinned staging lanes (no mapping to
    // fault in, no per-call pinning), overlapped with the PCIe transfer and the insert kernel of the previous chunk.
    int fdn = open(path, O_RDONLY);
    struct stat st;
    if (fdn < 0 || fstat(fdn, &st) != 0) { if (fdn >= 0) close(fdn); return mfx_fail(MFX_E_IO, "cannot open '%s'", path); }
    FlatHeader h;
    if ((uint64_t)st.st_size < sizeof(h) || pread(fdn, &h, sizeof(h), 0) != (ssize_t)sizeof(h)) {
      close(fdn);
      return mfx_fail(MFX_E_FORMAT, "'%s': truncated header", path);
    }
    if (const char *why = flat_header_problem(h, (uint64_t)st.st_size)) { close(fdn); return mfx_fail(MFX_E_FORMAT, "'%s': %s", path, why); }
    if ((int)h.k != ix->k) { close(fdn); return mfx_fail(MFX_E_INVAL, "'%s' holds %u-mers but the index is built for k=%d", path, h.k, ix->k); }
    const uint64_t kw = ix->key_words();                     // k > 31: 16-byte k-mers {low, high}
    if (h.flags & FLAT_DELTA) {
      rc = load_flat_delta(ixs, nix, fdn, path, h, (uint64_t)st.st_size, side, minV, maxV);
      close(fdn);
      return rc;
    }
    if (h.flags & FLAT_PACKED) {
      if (h.k > (uint32_t)MFX_MAX_K_PACKED || (uint64_t)st.st_size < sizeof(h) + h.n * 8 + h.n_escape * 12) {
        close(fdn);
        return mfx_fail(MFX_E_FORMAT, "'%s': truncated or inconsistent packed payload", path);
      }
      if (h.n) rc = mfx_index_add_from_file(ixs, nix, fdn, path, sizeof(h), 0, h.n, side, minV, maxV);
      if (rc == MFX_OK && h.n_escape)                        // the few counts beyond the record's field
        rc = load_flat_escapes(ixs, nix, fdn, path, h, sizeof(h) + h.n * 8, side, minV, maxV);
      close(fdn);
      return rc;
    }
    if ((uint64_t)st.st_size < sizeof(h) + h.n * (8 * kw + 4)) { close(fdn); return mfx_fail(MFX_E_FORMAT, "'%s': truncated payload", path); }
    if (h.n) rc = mfx_index_add_from_file(ixs, nix, fdn, path, sizeof(h), sizeof(h) + h.n * 8 * kw, h.n, side, minV, maxV);
    close(fdn);
  } else if (fmt == MFX_DB_TEXT) {
    int k = 0;
    if (text_is_plain(p)) {
      std::mutex mu;
      struct Sink {
        Feeder f;
        void operator()(uint64_t lo, uint64_t hi, uint32_t v) { f.push(lo, hi, v); }
        int done() { f.flush(); return f.rc; }
      };
      // the k of the file is only known after its first line: a wrong k would insert garbage, so it is checked first
      {
        int k1 = 0;
        if (FILE *f = fopen(path, "rb")) {
          char line[512];
          while (k1 == 0 && fgets(line, sizeof(line), f))
            for (const char *q = line; base_code((unsigned char)*q) >= 0; ++q) ++k1;
          fclose(f);
        }
        if (k1 != ix->k) rc = k1 ? mfx_fail(MFX_E_INVAL, "'%s' holds %d-mers but the index is built for k=%d", path, k1, ix->k)
                                 : mfx_fail(MFX_E_FORMAT, "'%s': no k-mers found", path);
      }
      if (rc == MFX_OK) rc = scan_text_parallel(p, &k, &n, [&](unsigned) { return Sink{Feeder{ixs, nix, side, minV, maxV, &mu}}; });
    } else {
      rc = scan_text(p, &k, [&](uint64_t lo, uint64_t hi, uint32_t v) { fd.push(lo, hi, v); }, &n);
    }
    if (rc == MFX_OK && k != ix->k) rc = mfx_fail(MFX_E_INVAL, "'%s' holds %d-mers but the index is built for k=%d", path, k, ix->k);
  } else {
    MerylIndex mi;
    rc = read_meryl_master(p, mi);
    if (rc == MFX_OK && (int)((mi.prefixSize + mi.suffixSize) / 2) != ix->k)
      rc = mfx_fail(MFX_E_INVAL, "'%s' holds %u-mers but the index is built for k=%d", path, (mi.prefixSize + mi.suffixSize) / 2, ix->k);
    if (rc == MFX_OK) {
      std::mutex mu;
      std::vector<MerylFileSums> per(64);
      rc = for_each_meryl_file([&](uint32_t fl) {
        Feeder tf{ixs, nix, side, minV, maxV, &mu};
        int r = read_meryl_data(meryl_file_name(p, fl, ".merylData"), fl, mi, [&](uint64_t lo, uint64_t hi, uint32_t v) { tf.push(lo, hi, v); }, &per[fl]);
        if (r == MFX_OK) tf.flush();
        return r ? r : tf.rc;
      });
      if (rc == MFX_OK) rc = check_meryl_sums(p, mi, per, true);
    }
  }
  if (rc == MFX_OK) fd.flush();
  return rc ? rc : fd.rc;
}

extern "C" int mfx_index_load_db_multi(mfx_index *const *ixs, uint32_t nix, const char *path, int side, uint64_t minV, uint64_t maxV) {
  try { return mfx_index_load_db_multi_impl(ixs, nix, path, side, minV, maxV); }                       // (nothing leaves the C ABI as an exception)
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_index_load_db_multi: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_index_load_db_multi: %s", e.what()); }
}


// writes this repo's flat binary form (fixtures, interchange)
static int mfx_db_write_flat_impl(const char *path, int k, const uint64_t *kmers, const uint32_t *values, uint64_t n) {
  if (!path || (n && (!kmers || !values))) return mfx_fail(MFX_E_INVAL, "mfx_db_write_flat: null argument");
  FILE *f = fopen(path, "wb");
  if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", path);
  FlatHeader h;
  memcpy(h.magic, "MFXKMER1", 8);
  h.k = (uint32_t)k;
  h.flags = 0;
  h.n = n;
  h.n_escape = 0;
  const char *de = getenv("MFX_FLAT_DELTA");
  if (k <= MFX_MAX_K_NARROW && n && !(de && atoi(de) == 0)) {   // sorted k-mers: delta-coded blocks
    const int rc = write_flat_delta(f, path, h, kmers, values, n);
    if (rc <= 0) { fclose(f); return rc; }
  }
  const char *pe = getenv("MFX_FLAT_PACKED");
  if (k <= MFX_MAX_K_PACKED && !(pe && atoi(pe) == 0)) {    // packed records: 8 bytes per k-mer
    h.flags |= FLAT_PACKED;
    std::vector<uint64_t> ek;
    std::vector<uint32_t> ev;
    bool ok = true;
    {
      // the escapes first (their number goes into the header), then the records in pieces
      for (uint64_t i = 0; i < n; ++i) if (values[i] >= MFX_PACKED_VMASK) { ek.push_back(kmers[i]); ev.push_back(values[i]); }
      h.n_escape = ek.size();
      ok = fwrite(&h, sizeof(h), 1, f) == 1;
      std::vector<uint64_t> rec(std::min<uint64_t>(n, 1u << 20));
      for (uint64_t o = 0; o < n && ok; o += rec.size()) {
        const uint64_t m = std::min<uint64_t>(rec.size(), n - o);
        for (uint64_t i = 0; i < m; ++i)
          rec[i] = (kmers[o + i] << MFX_PACKED_VBITS) | (values[o + i] >= MFX_PACKED_VMASK ? MFX_PACKED_VMASK : values[o + i]);
        ok = fwrite(rec.data(), 8, m, f) == m;
      }
      ok = ok && (ek.empty() || (fwrite(ek.data(), 8, ek.size(), f) == ek.size() && fwrite(ev.data(), 4, ev.size(), f) == ev.size()));
    }
    fclose(f);
    return ok ? MFX_OK : mfx_fail(MFX_E_IO, "short write to '%s'", path);
  }
  const size_t kw = k > MFX_MAX_K_NARROW ? 2 : 1;           // k > 31: two words per k-mer {low 64 bits, high bits}
  bool ok = fwrite(&h, sizeof(h), 1, f) == 1 && (n == 0 || (fwrite(kmers, 8 * kw, n, f) == n && fwrite(values, 4, n, f) == n));
  fclose(f);
  return ok ? MFX_OK : mfx_fail(MFX_E_IO, "short write to '%s'", path);
}

extern "C" int mfx_db_write_flat(const char *path, int k, const uint64_t *kmers, const uint32_t *values, uint64_t n) {
  try { return mfx_db_write_flat_impl(path, k, kmers, values, n); }                       // (nothing leaves the C ABI as an exception)
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_write_flat: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_write_flat: %s", e.what()); }
}


// ---------------------------------------------------------------------------
// mfx_db_convert: any accepted database -> this library's flat form, on the host (no device).  The point is the
// delta-coded form: `meryl print` text of a 30x human read set parses at ~120 M lines/s (a minute per run), the
// same database as delta-coded blocks loads in half a second.  The k-mers are collected in input order -- which
// is ascending for `meryl print` text and for meryl directories read file by file -- and sorted (bucket by the top
// bits, then every bucket on its own) only if they are not; k > 31 keeps its order (plain 16-byte k-mers).
// ---------------------------------------------------------------------------
namespace {
struct Collected { std::vector<uint64_t> k; std::vector<uint32_t> v; };

uint64_t flat_get_bits(const uint64_t *w, uint64_t bit, uint32_t nbits) {
  const uint64_t i = bit >> 6;
  const uint32_t sh = (uint32_t)bit & 63u;
  uint64_t x = w[i] >> sh;
  if (sh + nbits > 64u) x |= w[i + 1] << (64u - sh);
  return nbits >= 64 ? x : x & ((1ull << nbits) - 1ull);
}

// a flat file into host arrays (all three encodings; k > 31: two words per k-mer)
int read_flat_host(const std::string &path, int *k_out, std::vector<uint64_t> &keys, std::vector<uint32_t> &vals) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s'", path.c_str());
  auto bad = [&](const char *what) { fclose(f); return mfx_fail(MFX_E_FORMAT, "'%s': %s", path.c_str(), what); };
  FlatHeader h;
  if (fread(&h, sizeof(h), 1, f) != 1) return bad("truncated header");
  struct stat fst;
  if (fstat(fileno(f), &fst) != 0) { fclose(f); return mfx_fail(MFX_E_IO, "cannot stat '%s'", path.c_str()); }
  if (const char *why = flat_header_problem(h, (uint64_t)fst.st_size)) return bad(why);
  *k_out = (int)h.k;
  const size_t kw = h.k > (uint32_t)MFX_MAX_K_NARROW ? 2 : 1;
  try { keys.resize(h.n * kw); vals.resize(h.n); }
  catch (const std::exception &) { fclose(f); return mfx_fail(MFX_E_NOMEM, "'%s': no memory for %lu k-mers", path.c_str(), (unsigned long)h.n); }
  struct EscSplit { uint64_t i, p; uint32_t s; };              // an escaped record of a placed 31-mer file: position, stored number, strand bit (2: not known yet)
  std::vector<EscSplit> esc_split;
  auto escapes = [&]() -> bool {                              // the side list of a packed / delta file: counts by k-mer
    std::vector<uint64_t> ek(h.n_escape);
    std::vector<uint32_t> ev(h.n_escape);
    if (h.n_escape && (fread(ek.data(), 8, ek.size(), f) != ek.size() || fread(ev.data(), 4, ev.size(), f) != ev.size())) return false;
    std::vector<std::pair<uint64_t, uint32_t>> e(h.n_escape);
    for (size_t i = 0; i < e.size(); ++i) e[i] = {ek[i], ev[i]};
    std::sort(e.begin(), e.end());
    for (uint64_t i = 0; i < h.n; ++i)
      if (vals[i] == 0xffffffffu && !e.empty()) {             // marked below
        auto it = std::lower_bound(e.begin(), e.end(), std::make_pair(keys[i], 0u));
        if ((it == e.end() || it->first != keys[i]) && !esc_split.empty()) {
          // a placed 31-mer whose strand bit the block does not say (no twin beside it): the other strand's k-mer then
          auto es = std::lower_bound(esc_split.begin(), esc_split.end(), i, [](const EscSplit &a, uint64_t x) { return a.i < x; });
          if (es != esc_split.end() && es->i == i && es->s == 2u) {
            uint32_t top, hi, pm;
            keys[i] = mfx_p_decode_s((int)h.k, es->p, 1u, top, hi, pm);
            it = std::lower_bound(e.begin(), e.end(), std::make_pair(keys[i], 0u));
          }
        }
        if (it == e.end() || it->first != keys[i]) return false;
        vals[i] = it->second;
      }
    return true;
  };
  if (h.flags & FLAT_DELTA) {
    uint64_t nblocks = 0;
    if (kw != 1 || fread(&nblocks, 8, 1, f) != 1 || nblocks != (h.n + MFX_DELTA_BLOCK - 1) / MFX_DELTA_BLOCK) return bad("inconsistent delta-coded payload");
    std::vector<uint64_t> dir(2 * (nblocks + 1));
    if (fread(dir.data(), 8, dir.size(), f) != dir.size()) return bad("truncated block directory");
    std::vector<uint64_t> w;
    for (uint64_t b = 0; b < nblocks; ++b) {
      const uint64_t off = dir[2 * b + 1] & 0xffffffffffffull, nxt = dir[2 * b + 3] & 0xffffffffffffull;
      const uint32_t kb = (uint32_t)(dir[2 * b + 1] >> 48) & 0xffu, vb = (uint32_t)(dir[2 * b + 1] >> 56) & 0xffu;
      const uint64_t cnt = std::min<uint64_t>(MFX_DELTA_BLOCK, h.n - b * MFX_DELTA_BLOCK);
      if (nxt < off || (nxt - off) != (((cnt - 1) * kb + 63) / 64 + (cnt * vb + 63) / 64) * 8 || vb < 2 || vb > (uint32_t)MFX_DELTA_MAX_VBITS || kb > flat_rec_bits(h))
        return bad("inconsistent block directory");
      w.assign((nxt - off) / 8 + 1, 0);
      if (fseek(f, (long)off, SEEK_SET) != 0 || fread(w.data(), 8, (nxt - off) / 8, f) != (nxt - off) / 8) return bad("truncated block");
      const uint64_t *vw = w.data() + ((cnt - 1) * kb + 63) / 64;
      uint64_t cur = dir[2 * b];
      for (uint64_t e = 0; e < cnt; ++e) {
        if (e && kb) cur += flat_get_bits(w.data(), (e - 1) * kb, kb);
        keys[b * MFX_DELTA_BLOCK + e] = cur;
        const uint32_t v = (uint32_t)flat_get_bits(vw, e * vb, vb);
        vals[b * MFX_DELTA_BLOCK + e] = v == (1u << vb) - 1u ? 0xffffffffu : v;
      }
    }
    if (h.flags & FLAT_PLACED) {                              // the records are placement numbers: back to k-mers (in the file's order)
      for (uint64_t i = 0; i < h.n; ++i) if (!flat_rec_fits(keys[i], h)) return bad("a placed record is wider than 2k + 3 bits");
      const bool split = mfx_p_split((int)h.k);               // k = 31: the count field holds count << 1 | strand bit
      // (an ESCAPED record's field is all ones: its strand bit is the second of a pair of equal numbers', or whichever of the two k-mers the
      // escape list holds -- resolved in escapes() below from the numbers kept here)
      if (split)
        for (uint64_t i = 0; i < h.n; ++i)
          if (vals[i] == 0xffffffffu)
            esc_split.push_back({i, keys[i], (i > 0 && keys[i - 1] == keys[i]) ? 1u : (i + 1 < h.n && keys[i + 1] == keys[i]) ? 0u : 2u});
      par_blocks((h.n + 65535) / 65536, [&](uint64_t b) {
        for (uint64_t i = b * 65536, e = std::min<uint64_t>(h.n, i + 65536); i < e; ++i) {
          uint32_t top, hi, pm, sb = 0;
          if (split && vals[i] != 0xffffffffu) { sb = vals[i] & 1u; vals[i] >>= 1; }
          else if (split) {
            auto it = std::lower_bound(esc_split.begin(), esc_split.end(), i, [](const EscSplit &a, uint64_t x) { return a.i < x; });
            sb = it->s == 1u ? 1u : 0u;
          }
          keys[i] = mfx_p_decode_s((int)h.k, keys[i], sb, top, hi, pm);
        }
      });
    }
    if (fseek(f, (long)(dir[2 * nblocks + 1] & 0xffffffffffffull), SEEK_SET) != 0 || !escapes()) return bad("inconsistent escape list");
  } else if (h.flags & FLAT_PACKED) {
    if (kw != 1 || (h.n && fread(keys.data(), 8, h.n, f) != h.n)) return bad("truncated packed payload");
    for (uint64_t i = 0; i < h.n; ++i) {
      const uint32_t v = (uint32_t)keys[i] & MFX_PACKED_VMASK;
      keys[i] >>= MFX_PACKED_VBITS;
      vals[i] = v == MFX_PACKED_VMASK ? 0xffffffffu : v;
    }
    if (!escapes()) return bad("inconsistent escape list");
  } else if (h.n && (fread(keys.data(), 8 * kw, h.n, f) != h.n || fread(vals.data(), 4, h.n, f) != h.n)) return bad("truncated payload");
  // every k-mer inside 2k bits: what follows (sort_pairs' bucket index, the writers' bit widths) relies on it
  if (kw == 1) {
    for (uint64_t i = 0; i < h.n; ++i)
      if (!flat_key_fits(keys[i], h.k)) return bad("a k-mer is wider than 2k bits");
  } else if (h.k < 64) {
    for (uint64_t i = 0; i < h.n; ++i)
      if (keys[2 * i + 1] >> (2 * h.k - 64)) return bad("a k-mer is wider than 2k bits");
  }
  fclose(f);
  return MFX_OK;
}

// ascending order of (k, v) for one-word k-mers: buckets by the top bits, every bucket sorted on its own, all on the host threads
void sort_pairs(int k, std::vector<uint64_t> &keys, std::vector<uint32_t> &vals, int bits = 0) {      // bits: width of the keys (0: the k-mer's 2k)
  const uint64_t n = vals.size();
  if (!bits) bits = 2 * k;
  const int shift = std::max(0, bits - 12);
  const size_t NB = (size_t)1 << std::min(12, bits);
  // histogram and scatter by slices of the input, one per host thread (a 6 G-k-mer database is two 50 GB passes)
  const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({n / (1u << 20) + 1, 64, (uint64_t)mfx_host_threads()}));
  std::vector<std::vector<uint64_t>> cnt(T, std::vector<uint64_t>(NB, 0));
  auto slices = [&](auto &&fn) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t) th.emplace_back([&, t]() { fn(t, n * t / T, n * (t + 1) / T); });
    for (auto &x : th) x.join();
  };
  slices([&](unsigned t, uint64_t b, uint64_t e) { for (uint64_t i = b; i < e; ++i) ++cnt[t][keys[i] >> shift]; });
  std::vector<uint64_t> start(NB + 1, 0);
  for (size_t b = 0; b < NB; ++b) {
    uint64_t at = start[b];
    for (unsigned t = 0; t < T; ++t) { const uint64_t c = cnt[t][b]; cnt[t][b] = at; at += c; }     // slice t's first destination in bucket b
    start[b + 1] = at;
  }
  std::vector<uint64_t> k2(n);
  std::vector<uint32_t> v2(n);
  slices([&](unsigned t, uint64_t b, uint64_t e) {
    for (uint64_t i = b; i < e; ++i) { const uint64_t d = cnt[t][keys[i] >> shift]++; k2[d] = keys[i]; v2[d] = vals[i]; }
  });
  keys.swap(k2); vals.swap(v2);
  std::vector<uint64_t>().swap(k2); std::vector<uint32_t>().swap(v2);
  par_blocks(NB, [&](uint64_t b) {
    const uint64_t lo = start[b], hi = start[b + 1];
    if (hi - lo < 2 || std::is_sorted(keys.begin() + lo, keys.begin() + hi)) return;
    std::vector<std::pair<uint64_t, uint32_t>> t(hi - lo);
    for (uint64_t i = lo; i < hi; ++i) t[i - lo] = {keys[i], vals[i]};
    std::sort(t.begin(), t.end());
    for (uint64_t i = lo; i < hi; ++i) { keys[i] = t[i - lo].first; vals[i] = t[i - lo].second; }
  });
}
}  // namespace

// any accepted database -> its k-mers (k <= 31: ascending, every k-mer once) and counts in memory: what mfx_db_convert writes and
// mfx_db_convert_placed re-keys.  t_read / t_order: seconds (diagnostics)
static int read_db_sorted(const char *in_path, int *k_out, std::vector<uint64_t> &keys, std::vector<uint32_t> &vals, double *t_read = nullptr, double *t_order = nullptr) {
  const std::string p(in_path);
  const int fmt = detect(p);
  if (!fmt) return mfx_fail(MFX_E_IO, "k-mer database '%s' does not exist", in_path);
  int k = 0, rc = MFX_OK;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = now();
  auto gather = [&](std::vector<Collected> &parts, size_t kw) {   // parts in input order -> one pair of arrays
    uint64_t n = 0;
    for (auto &c : parts) n += c.v.size();
    keys.resize(n * kw);
    vals.resize(n);
    uint64_t at = 0;
    for (auto &c : parts) {
      if (!c.v.empty()) { memcpy(keys.data() + at * kw, c.k.data(), c.k.size() * 8); memcpy(vals.data() + at, c.v.data(), c.v.size() * 4); }
      at += c.v.size();
      Collected().k.swap(c.k); Collected().v.swap(c.v);
    }
  };
  if (fmt == MFX_DB_FLAT) rc = read_flat_host(p, &k, keys, vals);
  else if (fmt == MFX_DB_TEXT) {
    // k first (the first line), then every line; plain files by all host threads, collected PER PIECE of the file so that
    // the file's order -- ascending for `meryl print` -- survives the threads
    {
      mfx_file fh = mfx_open_reader(in_path);
      char line[512];
      while (fh.f && k == 0 && fgets(line, sizeof(line), fh.f))
        for (const char *q = line; base_code((unsigned char)*q) >= 0; ++q) ++k;
      if (fh.f) (void)mfx_close(fh, true);
      if (k == 0) return mfx_fail(MFX_E_FORMAT, "'%s': no k-mers found", in_path);
      if (k > MFX_MAX_K) return mfx_fail(MFX_E_FORMAT, "'%s': k-mers of more than %d bases", in_path, MFX_MAX_K);
    }
    const size_t kw = k > MFX_MAX_K_NARROW ? 2 : 1;
    uint64_t n = 0;
    int k2 = 0;
    if (text_is_plain(p)) {
      struct stat st;
      if (stat(in_path, &st) != 0) return mfx_fail(MFX_E_IO, "cannot open '%s'", in_path);
      const uint64_t PIECE = text_piece_bytes(), npieces = ((uint64_t)st.st_size + PIECE - 1) / PIECE;
      std::vector<Collected> per(npieces ? npieces : 1);
      std::vector<Collected *> cur(64, nullptr);
      struct Sink {
        Collected **c; size_t kw;
        void operator()(uint64_t lo, uint64_t hi, uint32_t v) { (*c)->k.push_back(lo); if (kw == 2) (*c)->k.push_back(hi); (*c)->v.push_back(v); }
        int done() { return MFX_OK; }
      };
      rc = scan_text_parallel(p, &k2, &n, [&](unsigned t) { return Sink{&cur[t], kw}; },
                              [&](unsigned t, uint64_t pc) {
                                cur[t] = &per[pc];
                                per[pc].v.reserve((size_t)(PIECE / (uint64_t)(k + 3)) + 16);
                                per[pc].k.reserve(((size_t)(PIECE / (uint64_t)(k + 3)) + 16) * kw);
                              });
      if (rc == MFX_OK) gather(per, kw);
    } else {
      std::vector<Collected> one(1);
      rc = scan_text(p, &k2, [&](uint64_t lo, uint64_t hi, uint32_t v) { one[0].k.push_back(lo); if (kw == 2) one[0].k.push_back(hi); one[0].v.push_back(v); }, &n);
      if (rc == MFX_OK) gather(one, kw);
    }
    if (rc == MFX_OK && k2 != k && n) rc = mfx_fail(MFX_E_FORMAT, "'%s': k-mer length %d differs from %d", in_path, k2, k);
  } else {
    MerylIndex mi;
    rc = read_meryl_master(p, mi);
    if (rc) return rc;
    k = (int)((mi.prefixSize + mi.suffixSize) / 2);
    const size_t kw = k > MFX_MAX_K_NARROW ? 2 : 1;
    std::vector<Collected> per(64);
    std::vector<MerylFileSums> sums(64);
    rc = for_each_meryl_file([&](uint32_t fl) {
      Collected &c = per[fl];
      return read_meryl_data(meryl_file_name(p, fl, ".merylData"), fl, mi,
                             [&](uint64_t lo, uint64_t hi, uint32_t v) { c.k.push_back(lo); if (kw == 2) c.k.push_back(hi); c.v.push_back(v); }, &sums[fl]);
    });
    if (rc == MFX_OK) rc = check_meryl_sums(p, mi, sums, true);
    if (rc == MFX_OK) gather(per, kw);
  }
  if (rc) return rc;
  const double t1 = now();
  if (k <= MFX_MAX_K_NARROW) {
    bool sorted = true;
    for (uint64_t i = 1; i < vals.size() && sorted; ++i) sorted = keys[i] > keys[i - 1];
    if (!sorted) {
      sort_pairs(k, keys, vals);
      for (uint64_t i = 1; i < vals.size(); ++i)
        if (keys[i] == keys[i - 1]) return mfx_fail(MFX_E_FORMAT, "'%s' lists a k-mer twice; a database holds every k-mer once", in_path);
    }
  }
  *k_out = k;
  if (t_read) *t_read = t1 - t0;
  if (t_order) *t_order = now() - t1;
  return MFX_OK;
}

static int mfx_db_convert_impl(const char *in_path, const char *out_path, uint64_t *n_out) {
  if (!in_path || !out_path) return mfx_fail(MFX_E_INVAL, "mfx_db_convert: null argument");
  int k = 0;
  std::vector<uint64_t> keys;
  std::vector<uint32_t> vals;
  double t_read = 0, t_order = 0;
  int rc = read_db_sorted(in_path, &k, keys, vals, &t_read, &t_order);
  if (rc) return rc;
  if (n_out) *n_out = vals.size();
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t2 = now();
  rc = mfx_db_write_flat(out_path, k, keys.data(), vals.data(), vals.size());
  if (getenv("MFX_DB_TIMING")) fprintf(stderr, "[mfx db] convert: read %.2f s, order %.2f s, write %.2f s\n", t_read, t_order, now() - t2);
  return rc;
}

// the flat form of ascending placement numbers P (mfx_place.h) and their counts
// sbits: the strand bits of a k = 31 file's records (mfx_place.h, mfx_p_split), pkeys then the numbers P >> 1; the C ABI's writer (arrays of P) serves k <= 30
static int mfx_db_write_flat_placed_impl(const char *path, int k, const uint64_t *pkeys, const uint32_t *values, uint64_t n, const uint8_t *sbits = nullptr) {
  if (!path || (n && (!pkeys || !values))) return mfx_fail(MFX_E_INVAL, "mfx_db_write_flat_placed: null argument");
  if (k < MFX_PLACE_MIN_K || k > MFX_PLACE_MAX_K) return mfx_fail(MFX_E_INVAL, "a placed database holds %d <= k <= %d (k = %d)", MFX_PLACE_MIN_K, MFX_PLACE_MAX_K, k);
  if (mfx_p_split(k) != (sbits != nullptr))
    return mfx_fail(MFX_E_INVAL, "mfx_db_write_flat_placed: the placement number of a %d-mer takes 65 bits; its placed database is made by mfx_db_convert_placed (merfin -convert -placed)", k);
  if (!n) return mfx_fail(MFX_E_INVAL, "mfx_db_write_flat_placed: no k-mers");
  for (uint64_t i = 0; i < n && !sbits; ++i)
    if (pkeys[i] >> mfx_p_bits(k)) return mfx_fail(MFX_E_INVAL, "mfx_db_write_flat_placed: record %lu is wider than a placement number of this k", (unsigned long)i);
  FILE *f = fopen(path, "wb");
  if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", path);
  FlatHeader h;
  memcpy(h.magic, "MFXKMER1", 8);
  h.k = (uint32_t)k;
  h.flags = 0;
  h.n = n;
  h.n_escape = 0;
  int rc = write_flat_delta(f, path, h, pkeys, values, n, true, sbits);
  if (fclose(f) != 0 && rc == 0) rc = mfx_fail(MFX_E_IO, "short write to '%s'", path);
  if (rc == 1) rc = mfx_fail(MFX_E_INVAL, "mfx_db_write_flat_placed: the records are not strictly ascending");
  return rc;
}
extern "C" int mfx_db_write_flat_placed(const char *path, int k, const uint64_t *pkeys, const uint32_t *values, uint64_t n) {
  try { return mfx_db_write_flat_placed_impl(path, k, pkeys, values, n); }
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_write_flat_placed: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_write_flat_placed: %s", e.what()); }
}

// P of n canonical k-mers, on the host (mfx_place.h; the device form: mfx_db_place_keys in mfx_api.cpp)
void mfx_place_keys_host(int k, const uint64_t *kmers, uint64_t n, uint64_t *out, uint8_t *sbits_out) {      // sbits_out: k = 31 (out then holds P >> 1)
  par_blocks((n + 65535) / 65536, [&](uint64_t b) {
    for (uint64_t i = b * 65536, e = std::min<uint64_t>(n, i + 65536); i < e; ++i) {
      const uint64_t key = kmers[i], rc = mfx_p_revcomp(key, k);
      uint32_t sb;
      out[i] = mfx_p_encode_s(k, key < rc ? key : rc, sb);
      if (sbits_out) sbits_out[i] = (uint8_t)sb;
    }
  });
}

// any accepted database -> the PLACED flat form: the records sorted by where the compact table puts them
static int mfx_db_convert_placed_impl(const char *in_path, const char *out_path, uint64_t *n_out) {
  if (!in_path || !out_path) return mfx_fail(MFX_E_INVAL, "mfx_db_convert_placed: null argument");
  {
    // k first: a database this form cannot hold is refused before its tens of GB are converted and read back
    mfx_db_info pi;
    if (int prc = mfx_db_probe(in_path, &pi)) return prc;
    if (pi.k < MFX_PLACE_MIN_K || pi.k > MFX_PLACE_MAX_K)
      return mfx_fail(MFX_E_INVAL, "'%s' holds %d-mers: a placed database holds %d <= k <= %d (use -convert without -placed)", in_path, pi.k, MFX_PLACE_MIN_K, MFX_PLACE_MAX_K);
  }
  // the database's k-mers in memory (any form), then re-keyed -- no intermediate file
  int k = 0;
  std::vector<uint64_t> keys;
  std::vector<uint32_t> vals;
  if (int rc = read_db_sorted(in_path, &k, keys, vals)) return rc;
  if (k < MFX_PLACE_MIN_K || k > MFX_PLACE_MAX_K)
    return mfx_fail(MFX_E_INVAL, "'%s' holds %d-mers: a placed database holds %d <= k <= %d (use -convert without -placed)", in_path, k, MFX_PLACE_MIN_K, MFX_PLACE_MAX_K);
  std::atomic<int> noncanon{0};
  par_blocks((vals.size() + 65535) / 65536, [&](uint64_t b) {
    for (uint64_t i = b * 65536, e = std::min<uint64_t>(vals.size(), i + 65536); i < e; ++i)
      if (keys[i] > mfx_p_revcomp(keys[i], k)) { noncanon = 1; return; }
  });
  if (noncanon) return mfx_fail(MFX_E_NONCANON, "'%s' is not canonical: a placed database holds canonical k-mers (the sequence-only index it feeds does)", in_path);
  if (n_out) *n_out = vals.size();
  if (!mfx_p_split(k)) {
    mfx_place_keys_host(k, keys.data(), vals.size(), keys.data(), nullptr);
    sort_pairs(k, keys, vals, mfx_p_bits(k));
    return mfx_db_write_flat_placed(out_path, k, keys.data(), vals.data(), vals.size());
  }
  // k = 31: the stored number is P >> 1, the strand bit beside it.  The records of either strand bit are sorted on their own and merged, the
  // s = 0 one of an equal pair first (the order of the 65-bit P)
  const uint64_t N = vals.size();
  std::vector<uint8_t> sb(N);
  mfx_place_keys_host(k, keys.data(), N, keys.data(), sb.data());
  std::vector<uint64_t> k1;
  std::vector<uint32_t> v1;
  {
    uint64_t n0 = 0;
    for (uint64_t i = 0; i < N; ++i) {
      if (sb[i]) { k1.push_back(keys[i]); v1.push_back(vals[i]); }
      else { keys[n0] = keys[i]; vals[n0] = vals[i]; ++n0; }
    }
    keys.resize(n0); vals.resize(n0);
  }
  sort_pairs(k, keys, vals, 64);
  sort_pairs(k, k1, v1, 64);
  std::vector<uint64_t> mk(N);
  std::vector<uint32_t> mv(N);
  for (uint64_t a = 0, b = 0, o = 0; o < N; ++o) {
    const bool take0 = b == k1.size() || (a < keys.size() && keys[a] <= k1[b]);
    if (take0) { mk[o] = keys[a]; mv[o] = vals[a]; sb[o] = 0; ++a; }
    else { mk[o] = k1[b]; mv[o] = v1[b]; sb[o] = 1; ++b; }
  }
  std::vector<uint64_t>().swap(keys); std::vector<uint64_t>().swap(k1);
  return mfx_db_write_flat_placed_impl(out_path, k, mk.data(), mv.data(), N, sb.data());
}
extern "C" int mfx_db_convert_placed(const char *in_path, const char *out_path, uint64_t *n_out) {
  try { return mfx_db_convert_placed_impl(in_path, out_path, n_out); }
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_convert_placed: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_convert_placed: %s", e.what()); }
}

extern "C" int mfx_db_convert(const char *in_path, const char *out_path, uint64_t *n_out) {
  try { return mfx_db_convert_impl(in_path, out_path, n_out); }                       // (nothing leaves the C ABI as an exception)
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_convert: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_convert: %s", e.what()); }
}


// ---------------------------------------------------------------------------
// mfx_index_write_db: one side of a full table as the sorted flat database `merfin -convert` makes -- what turns the claiming read
// counter's table (mfx_reads_begin_all) into a -readmers file.  On the device (mfx_sort.hip): one streaming pass counts the entries
// with a non-zero count on `side` per bin of their top MFX_DB_BIN_BITS key bits; the bins are grouped into key ranges of at most R
// entries (mfx_grow.h: mfx_group_bins); per range the entries are compacted out of the table, radix-sorted and copied behind the ranges
// before them.  Ranges ascend and are sorted, so the host arrays are the whole side in ascending order: the existing writer gets them.
// ---------------------------------------------------------------------------
constexpr int MFX_DB_BIN_BITS = 12;
constexpr uint64_t MFX_DB_RANGE_DEFAULT = 1ull << 28;        // entries per range: 2 x 12 bytes x 2^28 = 6 GB of device buffers + the sort's

namespace {
struct DbDev {                                                 // device buffers of one call, freed on every way out
  void *p[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~DbDev() { for (void *x : p) if (x) (void)hipFree(x); }
};
}  // namespace

// the refusals of mfx_index_write_db, for everything that reads a side of a full table by key bins; `who`: the entry point, for the texts
static int db_side_checks(const mfx_index *ix, int side, const char *who) {
  if (side != 0 && side != 1) return mfx_fail(MFX_E_INVAL, "%s: side %d (0: the read counts, 1: the assembly counts)", who, side);
  if (ix->seq_only) return mfx_fail(MFX_E_INVAL, "%s: a sequence-only or path-only index holds part of a database only; write a full index (mfx_index_create)", who);
  if (ix->wide()) return mfx_fail(MFX_E_INVAL, "%s: the sorted form holds k <= %d; this index holds %d-mers", who, MFX_MAX_K_NARROW, ix->k);
  if (ix->shard_n > 1) return mfx_fail(MFX_E_INVAL, "%s: a sharded index holds part of a database only", who);
  return MFX_OK;
}

namespace {
struct DeviceBack {                                            // the caller's device again on every way out
  int d = -1;
  DeviceBack() { if (hipGetDevice(&d) != hipSuccess) d = -1; }
  ~DeviceBack() { if (d >= 0) (void)hipSetDevice(d); }
};
}  // namespace

// bins[key >> shift] of the side's entries, on the host (nbins = 2^min(2k, 12)); d_bins: nbins + 1 device words, the last left zero
static int db_side_bins(const mfx_index *ix, int side, uint64_t *d_bins, std::vector<uint64_t> &bins) {
  const int key_bits = 2 * ix->k, bin_bits = std::min(key_bits, MFX_DB_BIN_BITS), shift = key_bits - bin_bits;
  const uint32_t nbins = 1u << bin_bits;
  MFX_HIP(mfx_memset_now(d_bins, 0, (nbins + 1) * sizeof(uint64_t)));
  MFX_HIP(mfx_k_db_bins(ix->view(), side, shift, nbins, d_bins, nullptr));
  bins.resize(nbins);
  MFX_HIP(hipMemcpy(bins.data(), d_bins, nbins * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return MFX_OK;
}

static int mfx_index_key_bins_impl(const mfx_index *ix, int side, uint64_t *out, uint32_t *nbins_out) {
  if (!ix || !out) return mfx_fail(MFX_E_INVAL, "mfx_index_key_bins: null argument");
  if (int rc = db_side_checks(ix, side, "mfx_index_key_bins")) return rc;
  DeviceBack back;
  MFX_HIP(hipSetDevice(ix->device));
  const uint32_t nbins = 1u << std::min(2 * ix->k, MFX_DB_BIN_BITS);
  DbDev D;
  MFX_HIP(hipMalloc(&D.p[0], (nbins + 1) * sizeof(uint64_t)));
  std::vector<uint64_t> bins;
  if (int rc = db_side_bins(ix, side, (uint64_t *)D.p[0], bins)) return rc;
  memset(out, 0, (1u << MFX_DB_BIN_BITS) * sizeof(uint64_t));
  memcpy(out, bins.data(), nbins * sizeof(uint64_t));
  if (nbins_out) *nbins_out = nbins;
  return MFX_OK;
}

extern "C" int mfx_index_key_bins(const mfx_index *ix, int side, uint64_t *bins, uint32_t *nbins) {
  try { return mfx_index_key_bins_impl(ix, side, bins, nbins); }
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_index_key_bins: out of memory"); }
}

// the writer that takes several tables (mfx_db_writer_*): the host arrays of the database so far, ascending
struct mfx_db_writer {
  std::string path;
  int k = 0;
  std::vector<uint64_t> keys;
  std::vector<uint32_t> vals;
  // the streamed kind (mfx_db_writer_open_streamed): the blocks go to the spool <path>.blocks as they are made.  What stays on the host is
  // the directory (16 bytes per MFX_DELTA_BLOCK k-mers), the escapes and the carry: the fewer than MFX_DELTA_BLOCK pairs behind the last
  // full block.  close writes header and directory, puts the spool behind them, then the escapes: the bytes of write_flat_delta.
  bool streamed = false;
  std::string spool;
  int fd = -1;
  uint64_t n = 0, spool_bytes = 0;                             // k-mers appended (those of the carry too); bytes of the spool
  std::vector<uint64_t> dir;                                   // per block written: its first k-mer, its spool offset | kb << 48 | vb << 56
  std::vector<uint64_t> ek;                                    // the escapes, in the file's order
  std::vector<uint32_t> ev;
  std::vector<uint64_t> ck;                                    // the carry
  std::vector<uint32_t> cv;
  uint64_t last = 0;                                           // the last k-mer appended (n > 0)
  size_t bounce = 16u << 20;                                   // bytes of one pinned bounce buffer (MFX_DB_BOUNCE, read at open)
  double t_export = 0, t_sort = 0, t_plan = 0, t_pack = 0, t_copy = 0, t_spool = 0;      // MFX_DB_TIMING
  bool merging = false;                                        // mfx_db_merge's writer: its split has these in the place of export and sort
  double t_read = 0, t_decode = 0, t_merge = 0, t_combine = 0;
  ~mfx_db_writer() {
    if (fd >= 0) close(fd);
    if (streamed && !spool.empty()) unlink(spool.c_str());
  }
};

static double db_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int spool_write(mfx_db_writer *w, const void *p, uint64_t bytes) {         // behind the spool's end
  const char *c = (const char *)p;
  for (uint64_t done = 0; done < bytes;) {
    const ssize_t r = pwrite(w->fd, c + done, bytes - done, (off_t)(w->spool_bytes + done));
    if (r <= 0) return mfx_fail(MFX_E_IO, "writing '%s' failed: %s", w->spool.c_str(), strerror(errno));
    done += (uint64_t)r;
  }
  w->spool_bytes += bytes;
  return MFX_OK;
}

namespace {
// an append to a streamed writer that fails adds nothing: spool, directory, escapes and carry as they were
struct StreamUndo {
  mfx_db_writer *w;
  uint64_t n, spool_bytes, last;
  size_t ndir, nesc;
  std::vector<uint64_t> ck;
  std::vector<uint32_t> cv;
  bool keep = false;
  explicit StreamUndo(mfx_db_writer *w_) : w(w_), n(w_->n), spool_bytes(w_->spool_bytes), last(w_->last), ndir(w_->dir.size()), nesc(w_->ek.size()),
                                           ck(w_->ck), cv(w_->cv) {}
  ~StreamUndo() {
    if (keep) return;
    w->n = n; w->last = last;
    w->dir.resize(ndir); w->ek.resize(nesc); w->ev.resize(nesc);
    w->ck.swap(ck); w->cv.swap(cv);
    if (w->spool_bytes != spool_bytes) { w->spool_bytes = spool_bytes; (void)!ftruncate(w->fd, (off_t)spool_bytes); }
  }
};

// full blocks packed on the host (pack_delta_block) and written to the spool a few MB at a time
struct StreamHostOut {
  mfx_db_writer *w;
  std::vector<uint64_t> buf;
  uint64_t pending = 0;                                        // bytes of buf not yet in the spool
  int add(const uint64_t *k, const uint32_t *v, uint32_t cnt) {
    const DeltaBlockPlan p = plan_delta_block(k, v, cnt);
    if (buf.size() < (pending + p.bytes) / 8) buf.resize((pending + p.bytes) / 8);
    pack_delta_block(k, v, cnt, p, buf.data() + pending / 8);
    w->dir.push_back(k[0]);
    w->dir.push_back((w->spool_bytes + pending) | ((uint64_t)p.kb << 48) | ((uint64_t)p.vb << 56));
    pending += p.bytes;
    if (p.nesc) {
      const uint32_t esc = (1u << p.vb) - 1u;
      for (uint32_t i = 0; i < cnt; ++i) if (v[i] >= esc) { w->ek.push_back(k[i]); w->ev.push_back(v[i]); }
    }
    return pending >= (8u << 20) ? flush() : MFX_OK;
  }
  int flush() {
    const uint64_t b = pending;
    pending = 0;
    return b ? spool_write(w, buf.data(), b) : MFX_OK;
  }
};
}  // namespace

// strictly ascending host arrays behind what a streamed writer holds (the caller checked the order)
static int stream_append_host(mfx_db_writer *w, const uint64_t *kmers, const uint32_t *values, uint64_t n) {
  if (n == 0) return MFX_OK;
  StreamUndo undo(w);
  StreamHostOut out{w};
  uint64_t pos = 0;
  if (!w->ck.empty()) {                                        // the carry first: filled up to a block, if the append reaches that far
    pos = std::min<uint64_t>(MFX_DELTA_BLOCK - w->ck.size(), n);
    w->ck.insert(w->ck.end(), kmers, kmers + pos);
    w->cv.insert(w->cv.end(), values, values + pos);
    if (w->ck.size() == MFX_DELTA_BLOCK) {
      if (int rc = out.add(w->ck.data(), w->cv.data(), MFX_DELTA_BLOCK)) return rc;
      w->ck.clear();
      w->cv.clear();
    }
  }
  for (; n - pos >= MFX_DELTA_BLOCK; pos += MFX_DELTA_BLOCK)
    if (int rc = out.add(kmers + pos, values + pos, MFX_DELTA_BLOCK)) return rc;
  if (pos < n) {                                               // (the carry is empty here)
    w->ck.assign(kmers + pos, kmers + n);
    w->cv.assign(values + pos, values + n);
  }
  if (int rc = out.flush()) return rc;
  w->n += n;
  w->last = kmers[n - 1];
  undo.keep = true;
  return MFX_OK;
}

// the device part: the side's entries, by key ranges compacted out of the table, sorted and copied behind what the writer holds
namespace {
struct DbBounce {                                              // two pinned buffers and their events: the packed bytes' way to the spool
  void *pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~DbBounce() {
    for (void *x : pin) if (x) (void)hipHostFree(x);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};
}  // namespace

// `bytes` of device memory behind the spool's end: the copy of piece i + 1 runs while piece i is written
static int spool_from_device(mfx_db_writer *w, DbBounce &B, const char *src, uint64_t bytes, double &t_copy, double &t_write) {
  const uint64_t piece = w->bounce;
  const uint64_t np = (bytes + piece - 1) / piece;
  auto len = [&](uint64_t i) { return std::min<uint64_t>(piece, bytes - i * piece); };
  for (uint64_t i = 0; i <= np; ++i) {
    if (i < np) {
      MFX_HIP(hipMemcpyAsync(B.pin[i & 1], src + i * piece, len(i), hipMemcpyDeviceToHost, nullptr));
      MFX_HIP(hipEventRecord(B.ev[i & 1], nullptr));
    }
    if (i > 0) {
      const double t0 = db_now();
      MFX_HIP(hipEventSynchronize(B.ev[(i - 1) & 1]));
      const double t1 = db_now();
      if (int rc = spool_write(w, B.pin[(i - 1) & 1], len(i - 1))) return rc;
      t_copy += t1 - t0;
      t_write += db_now() - t1;
    }
  }
  return MFX_OK;
}

namespace {
// what stream_append_device needs beside the pairs, for appends of at most `cap` pairs (the carry in front of them counted): plan and offsets
// of the blocks on the device and on the host, the escapes' buffers (grown to what an append escapes), the bounce buffers
struct StreamDev {
  DbDev D;                                                     // p[0]: plan and offsets of the blocks; p[1], p[2]: the escapes' k-mers and counts
  DbBounce B;
  uint64_t cap = 0, maxb = 0, esc_cap = 0;
  std::vector<mfx_delta_plan> plan;
  std::vector<uint64_t> woff;
  std::vector<uint32_t> eoff;
};
}  // namespace

static int stream_dev_init(StreamDev &S, const mfx_db_writer *w, uint64_t cap, const char *who, const char *knob) {
  S.cap = cap;
  S.maxb = cap / MFX_DELTA_BLOCK;
  if (hipMalloc(&S.D.p[0], (S.maxb ? S.maxb : 1) * (sizeof(mfx_delta_plan) + 8 + 4)) != hipSuccess) {
    (void)hipGetLastError();
    return mfx_fail(MFX_E_NOMEM, "%s: the block plan of %lu k-mers does not fit the device; lower %s", who, (unsigned long)cap, knob);
  }
  for (int i = 0; i < 2; ++i) {
    MFX_HIP(hipHostMalloc(&S.B.pin[i], w->bounce, hipHostMallocDefault));
    MFX_HIP(hipEventCreateWithFlags(&S.B.ev[i], hipEventDisableTiming));
  }
  return MFX_OK;
}

// Ascending pairs on the device behind what a streamed writer holds: rn > 0 pairs stand at s_keys + c and s_vals + c, c the pairs of the
// writer's carry (w->ck.size() when the arrays were filled), c + rn <= S.cap.  The carry is uploaded in front of them, the full blocks are
// planned and packed on the device (mfx_sort.hip) into d_out (out_bytes of it; 12 bytes a pair hold any block) and reach the spool through
// the bounce buffers; what is left is the next carry.  The first k-mer must lie above the writer's last.  A failure adds nothing.
static int stream_append_device(mfx_db_writer *w, StreamDev &S, uint64_t *s_keys, uint32_t *s_vals, uint64_t rn, uint64_t *d_out, uint64_t out_bytes,
                                const char *who, const char *knob) {
  StreamUndo undo(w);
  const uint64_t c = w->ck.size(), m = c + rn, nb = m / MFX_DELTA_BLOCK, rem = m % MFX_DELTA_BLOCK;
  if (rn == 0 || m > S.cap) return mfx_fail(MFX_E_INVAL, "%s: an append of %lu pairs behind a carry of %lu (buffers for %lu)", who, (unsigned long)rn, (unsigned long)c, (unsigned long)S.cap);
  if (c) {
    MFX_HIP(hipMemcpyAsync(s_keys, w->ck.data(), c * sizeof(uint64_t), hipMemcpyHostToDevice, nullptr));
    MFX_HIP(hipMemcpyAsync(s_vals, w->cv.data(), c * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
  }
  uint64_t ends[2] = {0, 0};                                   // the first and the last k-mer appended
  MFX_HIP(hipMemcpyAsync(&ends[0], s_keys + c, sizeof(uint64_t), hipMemcpyDeviceToHost, nullptr));
  MFX_HIP(hipMemcpyAsync(&ends[1], s_keys + m - 1, sizeof(uint64_t), hipMemcpyDeviceToHost, nullptr));
  MFX_HIP(hipStreamSynchronize(nullptr));
  double t0 = db_now(), t1;
  if (w->n != 0 && ends[0] <= w->last)
    return mfx_fail(MFX_E_INVAL, "%s: the appended k-mers start at %llu, not above the writer's last k-mer %llu: tables are appended in ascending key order, "
                    "their key ranges apart", who, (unsigned long long)ends[0], (unsigned long long)w->last);
  mfx_delta_plan *d_plan = (mfx_delta_plan *)S.D.p[0];
  uint64_t *d_woff = (uint64_t *)(d_plan + S.maxb);
  uint32_t *d_eoff = (uint32_t *)(d_woff + S.maxb);
  if (nb) {
    MFX_HIP(mfx_k_delta_plan(s_keys, s_vals, (uint32_t)nb, d_plan, nullptr));
    S.plan.resize(nb);
    MFX_HIP(hipMemcpy(S.plan.data(), d_plan, nb * sizeof(mfx_delta_plan), hipMemcpyDeviceToHost));
    S.woff.resize(nb);
    S.eoff.resize(nb);
    uint64_t words = 0, escapes = 0;
    for (uint64_t b = 0; b < nb; ++b) {                        // the plain scan: where every block's words and escapes start
      const uint32_t kb = S.plan[b].widths & 0xffu, vb = S.plan[b].widths >> 8;
      S.woff[b] = words;
      S.eoff[b] = (uint32_t)escapes;
      w->dir.push_back(S.plan[b].first);
      w->dir.push_back((w->spool_bytes + words * 8) | ((uint64_t)kb << 48) | ((uint64_t)vb << 56));
      words += mfx_delta_bytes(MFX_DELTA_BLOCK, kb, vb) / 8;
      escapes += S.plan[b].nesc;
    }
    if (words * 8 > out_bytes || escapes > m) return mfx_fail(MFX_E_HIP, "%s: the block plan of a key range is damaged", who);      // (nothing is packed beyond the buffers)
    if (escapes > S.esc_cap) {
      for (int i = 1; i < 3; ++i) if (S.D.p[i]) { (void)hipFree(S.D.p[i]); S.D.p[i] = nullptr; }
      S.esc_cap = 0;
      hipError_t ee = hipMalloc(&S.D.p[1], escapes * sizeof(uint64_t));
      if (ee == hipSuccess) ee = hipMalloc(&S.D.p[2], escapes * sizeof(uint32_t));
      if (ee != hipSuccess) {
        (void)hipGetLastError();
        return mfx_fail(MFX_E_NOMEM, "%s: the %lu escapes of a key range do not fit the device: %s; lower %s", who, (unsigned long)escapes, hipGetErrorString(ee), knob);
      }
      S.esc_cap = escapes;
    }
    MFX_HIP(hipMemcpyAsync(d_woff, S.woff.data(), nb * sizeof(uint64_t), hipMemcpyHostToDevice, nullptr));
    MFX_HIP(hipMemcpyAsync(d_eoff, S.eoff.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
    t1 = db_now();
    w->t_plan += t1 - t0;
    MFX_HIP(mfx_k_delta_pack(s_keys, s_vals, (uint32_t)nb, d_plan, d_woff, d_eoff, d_out, (uint64_t *)S.D.p[1], (uint32_t *)S.D.p[2], nullptr));
    MFX_HIP(hipStreamSynchronize(nullptr));                    // (woff / eoff are pageable: their copies are done before the next append changes them)
    t0 = db_now();
    w->t_pack += t0 - t1;
    if (int rc = spool_from_device(w, S.B, (const char *)d_out, words * 8, w->t_copy, w->t_spool)) return rc;
    if (escapes) {
      const size_t held = w->ek.size();
      w->ek.resize(held + escapes);
      w->ev.resize(held + escapes);
      MFX_HIP(hipMemcpy(w->ek.data() + held, S.D.p[1], escapes * sizeof(uint64_t), hipMemcpyDeviceToHost));
      MFX_HIP(hipMemcpy(w->ev.data() + held, S.D.p[2], escapes * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
  }
  w->ck.resize(rem);
  w->cv.resize(rem);
  if (rem && nb) {                                             // (no block made: the carry only grew, by what stands behind it)
    MFX_HIP(hipMemcpy(w->ck.data(), s_keys + nb * MFX_DELTA_BLOCK, rem * sizeof(uint64_t), hipMemcpyDeviceToHost));
    MFX_HIP(hipMemcpy(w->cv.data(), s_vals + nb * MFX_DELTA_BLOCK, rem * sizeof(uint32_t), hipMemcpyDeviceToHost));
  } else if (rem) {
    MFX_HIP(hipMemcpy(w->ck.data() + c, s_keys + c, rn * sizeof(uint64_t), hipMemcpyDeviceToHost));
    MFX_HIP(hipMemcpy(w->cv.data() + c, s_vals + c, rn * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  w->n += rn;
  w->last = ends[1];
  undo.keep = true;
  return MFX_OK;
}

// the device part of the streamed kind: per key range export and sort as below, the sort's output behind the carry, then stream_append_device
static int db_append_index_streamed(mfx_db_writer *w, const mfx_index *ix, int side, uint64_t *n_added, const char *who) {
  if (n_added) *n_added = 0;
  if (int rc = db_side_checks(ix, side, who)) return rc;
  if (ix->k != w->k) return mfx_fail(MFX_E_INVAL, "%s: the writer holds %d-mers, the index %d-mers", who, w->k, ix->k);
  uint64_t R = MFX_DB_RANGE_DEFAULT;
  if (const char *e = getenv("MFX_WRITE_DB_RANGE")) {
    const long long v = atoll(e);
    if (v > 0 && (uint64_t)v < R) R = (uint64_t)v;
  }
  DeviceBack back;
  MFX_HIP(hipSetDevice(ix->device));
  const int key_bits = 2 * ix->k, bin_bits = std::min(key_bits, MFX_DB_BIN_BITS), shift = key_bits - bin_bits;
  const uint32_t nbins = 1u << bin_bits;
  mfx_table_view t = ix->view();
  DbDev D;
  MFX_HIP(hipMalloc(&D.p[0], (nbins + 1) * sizeof(uint64_t)));     // the bins, then the export's counter
  uint64_t *d_bins = (uint64_t *)D.p[0];
  unsigned long long *d_count = (unsigned long long *)(d_bins + nbins);
  std::vector<uint64_t> bins;
  if (int rc = db_side_bins(ix, side, d_bins, bins)) return rc;
  std::vector<mfx_bin_range> ranges;
  mfx_group_bins(bins.data(), nbins, R, ranges);
  uint64_t n = 0, maxn = 0;
  for (const auto &r : ranges) { n += r.n; maxn = std::max(maxn, r.n); }
  if (n == 0) return MFX_OK;
  StreamUndo undo(w);
  // cap pairs: a range behind a carry.  p[1]: the export's k-mers, then its counts -- 12 bytes a pair, free again after the sort: a block
  // takes at most (62 + 22) bits a pair, so the packed words go there.  p[2], p[4]: the sorted pairs.
  const uint64_t cap = maxn + MFX_DELTA_BLOCK - 1;
  size_t tmp_bytes = 0;
  if (int rc = mfx_sort_db_pairs(nullptr, tmp_bytes, nullptr, nullptr, nullptr, nullptr, maxn, key_bits, nullptr)) return rc;
  hipError_t e = hipMalloc(&D.p[1], cap * 12);
  if (e == hipSuccess) e = hipMalloc(&D.p[2], cap * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc(&D.p[4], cap * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&D.p[5], tmp_bytes ? tmp_bytes : 1);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return mfx_fail(MFX_E_NOMEM, "%s: the buffers of a key range of %lu k-mers (%.3f GB) do not fit the device: %s; lower MFX_WRITE_DB_RANGE", who,
                    (unsigned long)maxn, ((double)cap * 24 + (double)tmp_bytes) / 1e9, hipGetErrorString(e));
  }
  uint64_t *x_keys = (uint64_t *)D.p[1], *s_keys = (uint64_t *)D.p[2], *d_out = (uint64_t *)D.p[1];
  uint32_t *x_vals = (uint32_t *)((char *)D.p[1] + cap * 8), *s_vals = (uint32_t *)D.p[4];
  StreamDev S;
  if (int rc = stream_dev_init(S, w, cap, who, "MFX_WRITE_DB_RANGE")) return rc;
  for (const auto &r : ranges) {
    double t0 = db_now();
    MFX_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), nullptr));
    MFX_HIP(mfx_k_db_export(t, side, shift, r.bin_lo, r.bin_hi, x_keys, x_vals, maxn, d_count, nullptr));
    unsigned long long got = 0;
    MFX_HIP(hipMemcpyAsync(&got, d_count, sizeof(got), hipMemcpyDeviceToHost, nullptr));
    MFX_HIP(hipStreamSynchronize(nullptr));
    if (got != r.n)
      return mfx_fail(MFX_E_INVAL, "%s: the table changed while it was written (a key range held %lu k-mers, then %lu); nothing else may "
                      "use the index during the call", who, (unsigned long)r.n, (unsigned long)got);
    double t1 = db_now();
    w->t_export += t1 - t0;
    if (r.n == 0) continue;
    const uint64_t c = w->ck.size();                             // c + r.n <= cap: c < MFX_DELTA_BLOCK, r.n <= maxn
    if (int rc = mfx_sort_db_pairs(D.p[5], tmp_bytes, x_keys, s_keys + c, x_vals, s_vals + c, r.n, key_bits, nullptr)) return rc;
    MFX_HIP(hipStreamSynchronize(nullptr));
    w->t_sort += db_now() - t1;
    if (int rc = stream_append_device(w, S, s_keys, s_vals, r.n, d_out, cap * 12, who, "MFX_WRITE_DB_RANGE")) return rc;
  }
  undo.keep = true;
  if (n_added) *n_added = n;
  return MFX_OK;
}

static int db_append_index(mfx_db_writer *w, const mfx_index *ix, int side, uint64_t *n_added, const char *who) {
  if (w->streamed) return db_append_index_streamed(w, ix, side, n_added, who);
  if (n_added) *n_added = 0;
  if (int rc = db_side_checks(ix, side, who)) return rc;
  if (ix->k != w->k) return mfx_fail(MFX_E_INVAL, "%s: the writer holds %d-mers, the index %d-mers", who, w->k, ix->k);
  uint64_t R = MFX_DB_RANGE_DEFAULT;
  if (const char *e = getenv("MFX_WRITE_DB_RANGE")) {          // read per call: tests reach several ranges on small tables
    const long long v = atoll(e);
    if (v > 0 && (uint64_t)v < R) R = (uint64_t)v;
  }
  DeviceBack back;
  MFX_HIP(hipSetDevice(ix->device));
  const int key_bits = 2 * ix->k, bin_bits = std::min(key_bits, MFX_DB_BIN_BITS), shift = key_bits - bin_bits;
  const uint32_t nbins = 1u << bin_bits;
  mfx_table_view t = ix->view();
  DbDev D;
  MFX_HIP(hipMalloc(&D.p[0], (nbins + 1) * sizeof(uint64_t)));     // the bins, then the export's counter
  uint64_t *d_bins = (uint64_t *)D.p[0];
  unsigned long long *d_count = (unsigned long long *)(d_bins + nbins);
  std::vector<uint64_t> bins;
  if (int rc = db_side_bins(ix, side, d_bins, bins)) return rc;
  std::vector<mfx_bin_range> ranges;
  mfx_group_bins(bins.data(), nbins, R, ranges);
  uint64_t n = 0, maxn = 0;
  for (const auto &r : ranges) { n += r.n; maxn = std::max(maxn, r.n); }
  if (n == 0) return MFX_OK;
  const uint64_t held = w->keys.size();
  struct Undo {                                                // an append that fails adds nothing
    mfx_db_writer *w; uint64_t held; bool keep = false;
    ~Undo() { if (!keep) { w->keys.resize(held); w->vals.resize(held); } }
  } undo{w, held};
  w->keys.reserve(held + n);                                     // exactly: resize alone would double the capacity.  The k-mers held move into the new
  w->vals.reserve(held + n);                                     // arrays, so both are alive for the move: see the header on the writer's host memory
  w->keys.resize(held + n);
  w->vals.resize(held + n);
  size_t tmp_bytes = 0;
  if (int rc = mfx_sort_db_pairs(nullptr, tmp_bytes, nullptr, nullptr, nullptr, nullptr, maxn, key_bits, nullptr)) return rc;
  hipError_t e = hipMalloc(&D.p[1], maxn * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc(&D.p[2], maxn * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc(&D.p[3], maxn * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&D.p[4], maxn * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&D.p[5], tmp_bytes ? tmp_bytes : 1);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return mfx_fail(MFX_E_NOMEM, "%s: the buffers of a key range of %lu k-mers (%.3f GB) do not fit the device: %s; lower MFX_WRITE_DB_RANGE", who,
                    (unsigned long)maxn, ((double)maxn * 24 + (double)tmp_bytes) / 1e9, hipGetErrorString(e));
  }
  uint64_t at = held;
  for (const auto &r : ranges) {
    MFX_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), nullptr));
    MFX_HIP(mfx_k_db_export(t, side, shift, r.bin_lo, r.bin_hi, (uint64_t *)D.p[1], (uint32_t *)D.p[3], maxn, d_count, nullptr));
    unsigned long long got = 0;
    MFX_HIP(hipMemcpyAsync(&got, d_count, sizeof(got), hipMemcpyDeviceToHost, nullptr));
    MFX_HIP(hipStreamSynchronize(nullptr));
    if (got != r.n)
      return mfx_fail(MFX_E_INVAL, "%s: the table changed while it was written (a key range held %lu k-mers, then %lu); nothing else may "
                      "use the index during the call", who, (unsigned long)r.n, (unsigned long)got);
    if (int rc = mfx_sort_db_pairs(D.p[5], tmp_bytes, (const uint64_t *)D.p[1], (uint64_t *)D.p[2], (const uint32_t *)D.p[3], (uint32_t *)D.p[4], r.n,
                                   key_bits, nullptr))
      return rc;
    MFX_HIP(hipMemcpyAsync(w->keys.data() + at, D.p[2], r.n * sizeof(uint64_t), hipMemcpyDeviceToHost, nullptr));
    MFX_HIP(hipMemcpyAsync(w->vals.data() + at, D.p[4], r.n * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
    MFX_HIP(hipStreamSynchronize(nullptr));
    if (at == held && held != 0 && w->keys[held] <= w->keys[held - 1])
      return mfx_fail(MFX_E_INVAL, "%s: the appended k-mers start at %llu, not above the writer's last k-mer %llu: tables are appended in ascending key order, "
                      "their key ranges apart", who, (unsigned long long)w->keys[held], (unsigned long long)w->keys[held - 1]);
    at += r.n;
  }
  undo.keep = true;
  if (n_added) *n_added = n;
  return MFX_OK;
}

extern "C" mfx_db_writer *mfx_db_writer_open(const char *path, int k) {
  if (!path) { mfx_fail(MFX_E_INVAL, "mfx_db_writer_open: null argument"); return nullptr; }
  if (k < 1 || k > MFX_MAX_K_NARROW) { mfx_fail(MFX_E_INVAL, "mfx_db_writer_open: the sorted form holds 1 <= k <= %d; k = %d", MFX_MAX_K_NARROW, k); return nullptr; }
  try {
    mfx_db_writer *w = new mfx_db_writer;
    w->path = path;
    w->k = k;
    return w;
  } catch (const std::bad_alloc &) { mfx_fail(MFX_E_NOMEM, "mfx_db_writer_open: out of memory"); return nullptr; }
}

extern "C" int mfx_db_writer_append_index(mfx_db_writer *w, const mfx_index *ix, int side, uint64_t *n_added) {
  if (!w || !ix) return mfx_fail(MFX_E_INVAL, "mfx_db_writer_append_index: null argument");
  try { return db_append_index(w, ix, side, n_added, "mfx_db_writer_append_index"); }     // (nothing leaves the C ABI as an exception)
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_writer_append_index: out of memory (12 bytes of host memory per k-mer held)"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_writer_append_index: %s", e.what()); }
}

static int db_open_streamed(const char *path, int k, mfx_db_writer **out) {
  *out = nullptr;
  if (!path) return mfx_fail(MFX_E_INVAL, "mfx_db_writer_open_streamed: null argument");
  if (k < 1 || k > MFX_MAX_K_NARROW) return mfx_fail(MFX_E_INVAL, "mfx_db_writer_open_streamed: the sorted form holds 1 <= k <= %d; k = %d", MFX_MAX_K_NARROW, k);
  if (const char *de = getenv("MFX_FLAT_DELTA"))
    if (atoi(de) == 0) return mfx_fail(MFX_E_INVAL, "mfx_db_writer_open_streamed: the streamed writer makes delta-coded blocks; MFX_FLAT_DELTA=0 asks for another form");
  try {
    std::unique_ptr<mfx_db_writer> w(new mfx_db_writer);
    w->path = path;
    w->k = k;
    w->streamed = true;
    if (const char *e = getenv("MFX_DB_BOUNCE")) {               // bytes of a bounce buffer: tests reach several pieces on small tables
      const long long v = atoll(e);
      if (v >= 8 && (uint64_t)v < w->bounce) w->bounce = (size_t)v & ~(size_t)7;
    }
    const std::string spool = w->path + ".blocks";
    w->fd = open(spool.c_str(), O_RDWR | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (w->fd < 0) return mfx_fail(MFX_E_IO, "mfx_db_writer_open_streamed: cannot create the spool '%s': %s", spool.c_str(), strerror(errno));
    w->spool = spool;                                            // (set once the file is this writer's: only then is it removed with it)
    *out = w.release();
    return MFX_OK;
  } catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_writer_open_streamed: out of memory"); }
}

extern "C" mfx_db_writer *mfx_db_writer_open_streamed(const char *path, int k) {
  mfx_db_writer *w = nullptr;
  (void)db_open_streamed(path, k, &w);
  return w;
}

static int db_append_sorted(mfx_db_writer *w, const uint64_t *kmers, const uint32_t *values, uint64_t n) {
  if (n == 0) return MFX_OK;
  const bool had = w->streamed ? w->n != 0 : !w->keys.empty();
  const uint64_t before = w->streamed ? w->last : (had ? w->keys.back() : 0);
  if (had && kmers[0] <= before)
    return mfx_fail(MFX_E_INVAL, "mfx_db_writer_append_sorted: the appended k-mers start at %llu, not above the writer's last k-mer %llu", (unsigned long long)kmers[0],
                    (unsigned long long)before);
  for (uint64_t i = 1; i < n; ++i)
    if (kmers[i] <= kmers[i - 1])
      return mfx_fail(MFX_E_INVAL, "mfx_db_writer_append_sorted: the k-mers are not strictly ascending (k-mer %lu is %llu, the one before it %llu)", (unsigned long)i,
                      (unsigned long long)kmers[i], (unsigned long long)kmers[i - 1]);
  if (w->streamed) return stream_append_host(w, kmers, values, n);
  const size_t held = w->keys.size();
  try {
    w->keys.insert(w->keys.end(), kmers, kmers + n);
    w->vals.insert(w->vals.end(), values, values + n);
  } catch (...) { w->keys.resize(held); w->vals.resize(held); throw; }
  return MFX_OK;
}

extern "C" int mfx_db_writer_append_sorted(mfx_db_writer *w, const uint64_t *kmers, const uint32_t *values, uint64_t n) {
  if (!w || (n && (!kmers || !values))) return mfx_fail(MFX_E_INVAL, "mfx_db_writer_append_sorted: null argument");
  try { return db_append_sorted(w, kmers, values, n); }
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_writer_append_sorted: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_writer_append_sorted: %s", e.what()); }
}

extern "C" int mfx_db_writer_info(const mfx_db_writer *w, uint64_t *kmers, uint64_t *blocks, uint64_t *escapes, uint64_t *spool_bytes, uint64_t *held_bytes) {
  if (!w) return mfx_fail(MFX_E_INVAL, "mfx_db_writer_info: null argument");
  if (kmers) *kmers = w->streamed ? w->n : w->keys.size();
  if (blocks) *blocks = w->dir.size() / 2;
  if (escapes) *escapes = w->ek.size();
  if (spool_bytes) *spool_bytes = w->spool_bytes;
  if (held_bytes)
    *held_bytes = w->streamed ? w->dir.size() * 8 + w->ek.size() * 8 + w->ev.size() * 4 + w->ck.size() * 8 + w->cv.size() * 4 : w->keys.size() * 8 + w->vals.size() * 4;
  return MFX_OK;
}

// the spool's bytes behind what `out` holds: copy_file_range where the file systems take it, else read and write
static int spool_to_file(mfx_db_writer *w, int out, const char *path) {
  uint64_t done = 0;
  off_t in_off = 0;
  while (done < w->spool_bytes) {
    const ssize_t r = copy_file_range(w->fd, &in_off, out, nullptr, (size_t)std::min<uint64_t>(w->spool_bytes - done, 1u << 30), 0);
    if (r <= 0) break;                                           // (not supported here, or the spool is short: the loop below says which)
    done += (uint64_t)r;
  }
  std::vector<char> buf(done < w->spool_bytes ? (8u << 20) : 0);
  while (done < w->spool_bytes) {
    const ssize_t r = pread(w->fd, buf.data(), (size_t)std::min<uint64_t>(buf.size(), w->spool_bytes - done), (off_t)done);
    if (r <= 0) return mfx_fail(MFX_E_IO, "reading '%s' failed", w->spool.c_str());
    for (ssize_t o = 0; o < r;) {
      const ssize_t x = write(out, buf.data() + o, (size_t)(r - o));
      if (x <= 0) return mfx_fail(MFX_E_IO, "short write to '%s'", path);
      o += x;
    }
    done += (uint64_t)r;
  }
  return MFX_OK;
}

static int db_close_streamed(mfx_db_writer *w) {
  const char *path = w->path.c_str();
  if (w->n == 0) return mfx_db_write_flat_impl(path, w->k, nullptr, nullptr, 0);
  const double t0 = db_now();
  if (!w->ck.empty()) {                                          // the last, partial block
    StreamHostOut out{w};
    int rc = out.add(w->ck.data(), w->cv.data(), (uint32_t)w->ck.size());
    if (rc == MFX_OK) rc = out.flush();
    if (rc) return rc;
  }
  const uint64_t nblocks = w->dir.size() / 2, base = sizeof(FlatHeader) + 8 + (nblocks + 1) * 16, at = base + w->spool_bytes;
  if (at >> 48) return mfx_fail(MFX_E_INVAL, "mfx_db_write_flat: the database is too large for the delta form");
  for (uint64_t b = 0; b < nblocks; ++b) w->dir[2 * b + 1] += base;      // (offsets below 2^48: the widths above them stay)
  w->dir.push_back(0);
  w->dir.push_back(at);
  FlatHeader h;
  memcpy(h.magic, "MFXKMER1", 8);
  h.k = (uint32_t)w->k;
  h.flags = FLAT_DELTA;
  h.n = w->n;
  h.n_escape = w->ek.size();
  FILE *f = fopen(path, "wb");
  if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", path);
  bool ok = fwrite(&h, sizeof(h), 1, f) == 1 && fwrite(&nblocks, 8, 1, f) == 1 && fwrite(w->dir.data(), 8, w->dir.size(), f) == w->dir.size() && fflush(f) == 0;
  int rc = ok ? spool_to_file(w, fileno(f), path) : mfx_fail(MFX_E_IO, "short write to '%s'", path);
  if (rc == MFX_OK) {
    ok = fseeko(f, 0, SEEK_END) == 0 &&
         (w->ek.empty() || (fwrite(w->ek.data(), 8, w->ek.size(), f) == w->ek.size() && fwrite(w->ev.data(), 4, w->ev.size(), f) == w->ev.size()));
    if (!ok) rc = mfx_fail(MFX_E_IO, "short write to '%s'", path);
  }
  if (fclose(f) != 0 && rc == MFX_OK) rc = mfx_fail(MFX_E_IO, "short write to '%s'", path);
  if (rc != MFX_OK) unlink(path);
  if (getenv("MFX_DB_TIMING") && w->merging)
    fprintf(stderr, "[mfx db] merge: read %.2f s, decode %.2f s, merge %.2f s, combine %.2f s, plan %.2f s, pack %.2f s, copy %.2f s, spool write %.2f s, close %.2f s "
            "(%lu blocks, %lu escapes)\n", w->t_read, w->t_decode, w->t_merge, w->t_combine, w->t_plan, w->t_pack, w->t_copy, w->t_spool, db_now() - t0,
            (unsigned long)nblocks, (unsigned long)w->ek.size());
  else if (getenv("MFX_DB_TIMING"))
    fprintf(stderr, "[mfx db] streamed writer: export %.2f s, sort %.2f s, plan %.2f s, pack %.2f s, copy %.2f s, spool write %.2f s, close %.2f s (%lu blocks, "
            "%lu escapes)\n", w->t_export, w->t_sort, w->t_plan, w->t_pack, w->t_copy, w->t_spool, db_now() - t0, (unsigned long)nblocks, (unsigned long)w->ek.size());
  return rc;
}

extern "C" int mfx_db_writer_close(mfx_db_writer *w, uint64_t *n_kmers) {
  if (!w) return mfx_fail(MFX_E_INVAL, "mfx_db_writer_close: null argument");
  int rc;
  try {
    if (n_kmers) *n_kmers = w->streamed ? w->n : w->keys.size();
    rc = w->streamed ? db_close_streamed(w) : mfx_db_write_flat_impl(w->path.c_str(), w->k, w->keys.data(), w->vals.data(), w->keys.size());
  }
  catch (const std::bad_alloc &) { rc = mfx_fail(MFX_E_NOMEM, "mfx_db_writer_close: out of memory"); }
  catch (const std::exception &e) { rc = mfx_fail(MFX_E_IO, "mfx_db_writer_close: %s", e.what()); }
  delete w;
  return rc;
}

extern "C" void mfx_db_writer_abort(mfx_db_writer *w) { delete w; }

static int mfx_index_write_db_impl(const mfx_index *ix, int side, const char *path, uint64_t *n_kmers) {
  if (!ix || !path) return mfx_fail(MFX_E_INVAL, "mfx_index_write_db: null argument");
  mfx_db_writer w;
  w.path = path;
  w.k = ix->k;
  if (int rc = db_append_index(&w, ix, side, nullptr, "mfx_index_write_db")) return rc;
  if (n_kmers) *n_kmers = w.keys.size();
  return mfx_db_write_flat_impl(path, ix->k, w.keys.data(), w.vals.data(), w.keys.size());
}

extern "C" int mfx_index_write_db_streamed(const mfx_index *ix, int side, const char *path, uint64_t *n_kmers) {
  if (!ix || !path) return mfx_fail(MFX_E_INVAL, "mfx_index_write_db_streamed: null argument");
  if (int rc = db_side_checks(ix, side, "mfx_index_write_db_streamed")) return rc;
  mfx_db_writer *w = nullptr;
  if (int rc = db_open_streamed(path, ix->k, &w)) return rc;
  int rc;
  try { rc = db_append_index(w, ix, side, nullptr, "mfx_index_write_db_streamed"); }
  catch (const std::bad_alloc &) { rc = mfx_fail(MFX_E_NOMEM, "mfx_index_write_db_streamed: out of memory"); }
  catch (const std::exception &e) { rc = mfx_fail(MFX_E_IO, "mfx_index_write_db_streamed: %s", e.what()); }
  if (rc) { mfx_db_writer_abort(w); return rc; }
  return mfx_db_writer_close(w, n_kmers);
}

extern "C" int mfx_index_write_db(const mfx_index *ix, int side, const char *path, uint64_t *n_kmers) {
  try { return mfx_index_write_db_impl(ix, side, path, n_kmers); }                     // (nothing leaves the C ABI as an exception)
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_index_write_db: out of memory (12 bytes of host memory per k-mer written)"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_index_write_db: %s", e.what()); }
}


// ---------------------------------------------------------------------------
// mfx_db_merge: sorted, delta-coded databases combined window by window (include/merfin_amd.h; the windows: mfx_merge.h; the kernels:
// mfx_merge.hip).  file blocks -> ascending runs on the device -> merged and combined -> stream_append_device; no table in between.
// ---------------------------------------------------------------------------
static_assert(MFX_MERGE_BLOCK == MFX_DELTA_BLOCK, "mfx_merge.h plans in blocks of the delta form");

namespace {
struct MergeIn {                                               // one input: header, directory and escapes on the host, the blocks in the file
  std::string path;
  int fd = -1;
  FlatHeader h;
  std::vector<uint64_t> dir;
  uint64_t nblocks = 0;
  std::vector<uint64_t> ek;
  std::vector<uint32_t> ev;
  MergeIn() = default;
  MergeIn(const MergeIn &) = delete;
  MergeIn &operator=(const MergeIn &) = delete;
  ~MergeIn() { if (fd >= 0) close(fd); }
  uint64_t off(uint64_t b) const { return dir[2 * b + 1] & 0xffffffffffffull; }
};
struct WriterAbort {                                           // the writer of a call that does not reach close: the spool goes with it
  mfx_db_writer *w = nullptr;
  ~WriterAbort() { if (w) mfx_db_writer_abort(w); }
};
}  // namespace

// header, directory and escape list of an input, by the loader's checks; every refusal names the file
static int merge_open_input(const char *path, MergeIn &in, const char *who = "mfx_db_merge") {
  in.path = path;
  const int fmt = detect(in.path);
  if (!fmt) return mfx_fail(MFX_E_IO, "%s: the input '%s' does not exist", who, path);
  if (fmt == MFX_DB_MERYL) return mfx_fail(MFX_E_FORMAT, "%s: '%s' is a meryl directory; the inputs are sorted flat databases: run `merfin -convert` first", who, path);
  if (fmt == MFX_DB_TEXT) return mfx_fail(MFX_E_FORMAT, "%s: '%s' is not a flat k-mer file (`meryl print` text?); the inputs are sorted flat databases: run `merfin -convert` first", who, path);
  in.fd = open(path, O_RDONLY | O_CLOEXEC);
  struct stat st;
  if (in.fd < 0 || fstat(in.fd, &st) != 0) return mfx_fail(MFX_E_IO, "cannot open '%s'", path);
  const uint64_t fsize = (uint64_t)st.st_size;
  if (fsize < sizeof(in.h) || pread(in.fd, &in.h, sizeof(in.h), 0) != (ssize_t)sizeof(in.h)) return mfx_fail(MFX_E_FORMAT, "'%s': truncated header", path);
  if (const char *why = flat_header_problem(in.h, fsize)) return mfx_fail(MFX_E_FORMAT, "'%s': %s", path, why);
  if (in.h.flags & FLAT_PLACED)
    return mfx_fail(MFX_E_FORMAT, "%s: '%s' is a placed database; the inputs are sorted by k-mer: merge those, then place the result (merfin -convert -placed)", who, path);
  if (in.h.n == 0) return MFX_OK;                               // (no k-mers: what mfx_db_write_flat writes for none has no blocks in any form)
  if (!(in.h.flags & FLAT_DELTA))
    return mfx_fail(MFX_E_FORMAT, "%s: '%s' is a %s flat file, not a sorted one: run `merfin -convert` first", who, path, (in.h.flags & FLAT_PACKED) ? "packed" : "plain");
  uint64_t expect = 0;
  if (int rc = read_delta_directory(in.fd, path, in.h, fsize, in.dir, &in.nblocks, &expect)) return rc;
  const uint64_t ne = in.h.n_escape;
  try { in.ek.resize(ne); in.ev.resize(ne); }
  catch (const std::exception &) { return mfx_fail(MFX_E_NOMEM, "'%s': no memory for %lu escapes", path, (unsigned long)ne); }
  if (ne && (pread(in.fd, in.ek.data(), ne * 8, (off_t)expect) != (ssize_t)(ne * 8) || pread(in.fd, in.ev.data(), ne * 4, (off_t)(expect + ne * 8)) != (ssize_t)(ne * 4)))
    return mfx_fail(MFX_E_IO, "reading '%s' failed", path);
  for (uint64_t i = 0; i < ne; ++i) {
    if (!flat_key_fits(in.ek[i], in.h.k)) return mfx_fail(MFX_E_FORMAT, "'%s': an escaped k-mer is wider than 2k bits", path);
    if (i && in.ek[i] <= in.ek[i - 1]) return mfx_fail(MFX_E_FORMAT, "'%s': the escape list of a sorted database does not ascend", path);
  }
  return MFX_OK;
}

// every check of mfx_db_merge that needs no device: the arguments, the inputs (opened into `ins`), their k, the output's identity
static int merge_check(const char *const *in_paths, uint32_t n_in, const char *out_path, const mfx_db_merge_opts *o, std::vector<std::unique_ptr<MergeIn>> &ins) {
  if (!in_paths || !out_path || !o) return mfx_fail(MFX_E_INVAL, "mfx_db_merge: null argument");
  if (n_in == 0 || n_in > MFX_MERGE_MAX_INPUTS) return mfx_fail(MFX_E_INVAL, "mfx_db_merge: %u inputs (1 to %u)", n_in, MFX_MERGE_MAX_INPUTS);
  if (o->op != MFX_MERGE_SUM && o->op != MFX_MERGE_MAX && o->op != MFX_MERGE_MIN && o->op != MFX_MERGE_INTERSECT)
    return mfx_fail(MFX_E_INVAL, "mfx_db_merge: unknown operation %d (MFX_MERGE_SUM, _MAX, _MIN, _INTERSECT)", o->op);
  if (o->minV > o->maxV) return mfx_fail(MFX_E_INVAL, "mfx_db_merge: the filter keeps nothing (min %llu > max %llu)", (unsigned long long)o->minV, (unsigned long long)o->maxV);
  for (uint32_t i = 0; i < n_in; ++i) {
    if (!in_paths[i]) return mfx_fail(MFX_E_INVAL, "mfx_db_merge: null argument");
    ins.emplace_back(new MergeIn);
    if (int rc = merge_open_input(in_paths[i], *ins.back())) return rc;
    if (ins[i]->h.k != ins[0]->h.k)
      return mfx_fail(MFX_E_INVAL, "mfx_db_merge: '%s' holds %u-mers, '%s' %u-mers: the inputs are of one k", in_paths[i], ins[i]->h.k, in_paths[0], ins[0]->h.k);
  }
  struct stat so;
  if (stat(out_path, &so) == 0)
    for (uint32_t i = 0; i < n_in; ++i) {
      struct stat si;
      if (fstat(ins[i]->fd, &si) == 0 && si.st_dev == so.st_dev && si.st_ino == so.st_ino)
        return mfx_fail(MFX_E_INVAL, "mfx_db_merge: the output '%s' is the input '%s'", out_path, in_paths[i]);
    }
  return MFX_OK;
}

// ---- what mfx_db_merge and mfx_db_join_* share: the windows of the opened inputs, and a window's blocks decoded into one dense run per input
namespace {
struct MergeWindows {                                          // the plan (mfx_merge.h) and what the largest window takes
  std::vector<mfx_merge_input> pin;
  std::vector<mfx_merge_window> win;
  std::vector<uint64_t> blk;
  uint64_t n_all = 0, max_pairs = 0, max_bytes = 0, max_tasks = 0, max_esc = 0;
};
struct MergeRun { uint64_t off, len; };
struct MergeDecoder {                                          // a window's way from the files to the runs; the caller owns the device buffers
  void *d_words = nullptr;                                     // max_bytes + 8: the window's blocks
  mfx_merge_task *d_tasks = nullptr;                           // max_tasks
  uint32_t *d_below = nullptr, *d_above = nullptr, *d_err = nullptr;      // max_tasks, max_tasks, one per input
  uint64_t *d_ek = nullptr;                                    // max_esc + 1: the window's escapes
  uint32_t *d_ev = nullptr;
  void *pinned = nullptr;                                      // max_bytes + 8 on the host: the blocks on their way to the device
  std::vector<mfx_merge_task> tasks;
  std::vector<uint64_t> hek, run_off, run_len, first_task;
  std::vector<uint32_t> hev, cnt, errs;
  std::vector<MergeRun> runs;                                  // per input: its dense run of the window in the decoded buffer
  double t_read = 0, t_decode = 0;                             // of the last window
  uint32_t zero_from = ~0u;                                    // mfx_db_merge_except: the inputs from this one on are subtracted
  MergeDecoder() = default;
  MergeDecoder(const MergeDecoder &) = delete;
  MergeDecoder &operator=(const MergeDecoder &) = delete;
  ~MergeDecoder() { if (pinned) (void)hipHostFree(pinned); }
};
}  // namespace

static uint64_t merge_range_knob() {
  uint64_t R = MFX_MERGE_RANGE_DEFAULT;
  if (const char *e = getenv("MFX_MERGE_RANGE")) {             // read per call: tests reach many windows on small files
    const long long v = atoll(e);
    if (v > 0 && (uint64_t)v < R) R = (uint64_t)v;
  }
  return R;
}

static int merge_plan_windows(const std::vector<std::unique_ptr<MergeIn>> &ins, int k, const char *who, MergeWindows &P) {
  const uint32_t n_in = (uint32_t)ins.size();
  P.pin.resize(n_in);
  for (uint32_t i = 0; i < n_in; ++i) { P.pin[i] = mfx_merge_input{ins[i]->dir.data(), 2u, ins[i]->nblocks, ins[i]->h.n}; P.n_all += ins[i]->h.n; }
  mfx_merge_plan(P.pin.data(), n_in, k, merge_range_knob(), P.win, P.blk);
  for (size_t w = 0; w < P.win.size(); ++w) {
    uint64_t bytes = 0, tasks = 0, esc = 0;
    for (uint32_t i = 0; i < n_in; ++i) {
      const uint64_t b0 = P.blk[2 * (w * n_in + i)], b1 = P.blk[2 * (w * n_in + i) + 1];
      if (b1 <= b0) continue;
      bytes += ins[i]->off(b1) - ins[i]->off(b0);
      tasks += b1 - b0;
      uint64_t e0, e1;
      mfx_merge_escape_slice(ins[i]->ek.data(), ins[i]->ek.size(), P.win[w].lo, P.win[w].hi, &e0, &e1);
      esc += e1 - e0;
    }
    P.max_pairs = std::max(P.max_pairs, P.win[w].pairs); P.max_bytes = std::max(P.max_bytes, bytes);
    P.max_tasks = std::max(P.max_tasks, tasks); P.max_esc = std::max(P.max_esc, esc);
  }
  if (P.max_pairs > 0x7fffffffull || P.max_esc > 0x7fffffffull)
    return mfx_fail(MFX_E_INVAL, "%s: a window of %lu pairs (at most 2^31 - 1); lower MFX_MERGE_RANGE", who, (unsigned long)P.max_pairs);
  return MFX_OK;
}

// window wi: its blocks read (pread) and decoded on the device into keys / vals, D.runs the inputs' dense runs in them.  A block that decodes
// what no writer makes ends in MFX_E_FORMAT, naming the file.
static int merge_decode_window(const std::vector<std::unique_ptr<MergeIn>> &ins, const MergeWindows &P, size_t wi, int k, const char *who, MergeDecoder &D,
                               uint64_t *keys, uint32_t *vals) {
  const uint32_t n_in = (uint32_t)ins.size();
  const uint64_t lo = P.win[wi].lo, hi = P.win[wi].hi, END = mfx_merge_end(k);
  uint64_t *words = (uint64_t *)D.pinned;
  D.run_off.resize(n_in); D.run_len.resize(n_in); D.first_task.resize(n_in); D.errs.resize(n_in);
  D.t_read = D.t_decode = 0;
  double t0 = db_now();
  // ---- the window's blocks and escapes, input after input
  D.tasks.clear(); D.hek.clear(); D.hev.clear();
  uint64_t nwords = 0, npairs = 0;
  for (uint32_t i = 0; i < n_in; ++i) {
    const MergeIn &in = *ins[i];
    const uint64_t b0 = P.blk[2 * (wi * n_in + i)], b1 = P.blk[2 * (wi * n_in + i) + 1];
    D.run_off[i] = npairs; D.run_len[i] = 0; D.first_task[i] = D.tasks.size();
    if (b1 <= b0) continue;
    const uint64_t from = in.off(b0), bytes = in.off(b1) - from;
    if ((nwords * 8 + bytes) > P.max_bytes) return mfx_fail(MFX_E_INVAL, "%s: a window does not match its plan", who);      // (nothing is read beyond the buffer)
    for (uint64_t got = 0; got < bytes;) {
      const ssize_t r = pread(in.fd, (char *)(words + nwords) + got, bytes - got, (off_t)(from + got));
      if (r <= 0) return mfx_fail(MFX_E_IO, "reading '%s' failed", in.path.c_str());
      got += (uint64_t)r;
    }
    uint64_t e0, e1;
    mfx_merge_escape_slice(in.ek.data(), in.ek.size(), lo, hi, &e0, &e1);
    const uint32_t esc_lo = (uint32_t)D.hek.size(), esc_hi = esc_lo + (uint32_t)(e1 - e0);
    D.hek.insert(D.hek.end(), in.ek.begin() + e0, in.ek.begin() + e1);
    D.hev.insert(D.hev.end(), in.ev.begin() + e0, in.ev.begin() + e1);
    for (uint64_t b = b0; b < b1; ++b) {
      mfx_merge_task t;
      t.word_off = nwords + (in.off(b) - from) / 8;
      t.first = in.dir[2 * b];
      t.limit = b + 1 < in.nblocks ? in.dir[2 * (b + 1)] : END;
      t.out = npairs + (b - b0) * MFX_DELTA_BLOCK;
      t.kb = (uint32_t)(in.dir[2 * b + 1] >> 48) & 0xffu;
      t.vb = (uint32_t)(in.dir[2 * b + 1] >> 56) & 0xffu;
      t.cnt = (uint32_t)std::min<uint64_t>(MFX_DELTA_BLOCK, in.h.n - b * MFX_DELTA_BLOCK);
      t.esc_lo = esc_lo; t.esc_hi = esc_hi; t.input = i;
      D.tasks.push_back(t);
    }
    D.run_len[i] = mfx_merge_block_pairs(P.pin[i], b0, b1);
    npairs += D.run_len[i];
    nwords += bytes / 8;
  }
  const uint32_t nt = (uint32_t)D.tasks.size();
  if (npairs != P.win[wi].pairs || npairs > P.max_pairs || nwords * 8 > P.max_bytes || nt > P.max_tasks || D.hek.size() > P.max_esc)
    return mfx_fail(MFX_E_INVAL, "%s: a window does not match its plan", who);      // (nothing is decoded beyond the buffers)
  MFX_HIP(hipMemcpyAsync(D.d_words, words, nwords * 8, hipMemcpyHostToDevice, nullptr));
  MFX_HIP(hipMemcpyAsync(D.d_tasks, D.tasks.data(), nt * sizeof(mfx_merge_task), hipMemcpyHostToDevice, nullptr));
  if (!D.hek.empty()) {
    MFX_HIP(hipMemcpyAsync(D.d_ek, D.hek.data(), D.hek.size() * 8, hipMemcpyHostToDevice, nullptr));
    MFX_HIP(hipMemcpyAsync(D.d_ev, D.hev.data(), D.hev.size() * 4, hipMemcpyHostToDevice, nullptr));
  }
  MFX_HIP(hipMemsetAsync(D.d_err, 0, n_in * 4, nullptr));
  MFX_HIP(hipStreamSynchronize(nullptr));                      // (the host arrays are filled again for the next window)
  double t1 = db_now();
  D.t_read = t1 - t0;
  // ---- decode: one ascending run per input
  MFX_HIP(mfx_k_delta_decode(D.d_tasks, nt, (const uint64_t *)D.d_words, D.d_ek, D.d_ev, lo, hi, keys, vals, D.d_below, D.d_above, D.d_err, nullptr, D.zero_from));
  D.cnt.resize(2 * (size_t)nt);
  MFX_HIP(hipMemcpyAsync(D.cnt.data(), D.d_below, nt * 4, hipMemcpyDeviceToHost, nullptr));
  MFX_HIP(hipMemcpyAsync(D.cnt.data() + nt, D.d_above, nt * 4, hipMemcpyDeviceToHost, nullptr));
  MFX_HIP(hipMemcpyAsync(D.errs.data(), D.d_err, n_in * 4, hipMemcpyDeviceToHost, nullptr));
  MFX_HIP(hipStreamSynchronize(nullptr));
  D.t_decode = db_now() - t1;
  for (uint32_t i = 0; i < n_in; ++i)
    if (D.errs[i])
      return mfx_fail(MFX_E_FORMAT, "'%s': a block holds what no writer makes (%s%s%s): the file is damaged", ins[i]->path.c_str(),
                      (D.errs[i] & MFX_MERGE_ERR_ORDER) ? "k-mers that do not ascend below the next block's first; " : "",
                      (D.errs[i] & MFX_MERGE_ERR_ESCAPE) ? "an escaped count that is not in the escape list; " : "", (D.errs[i] & MFX_MERGE_ERR_ZERO) ? "a count of zero; " : "");
  D.runs.clear();
  for (uint32_t i = 0; i < n_in; ++i) {
    const uint64_t f = D.first_task[i], l = (i + 1 < n_in ? D.first_task[i + 1] : nt);
    MergeRun r{0, 0};
    // (ascending k-mers below every block's limit: only an input's first block reaches under lo, only its last to hi and beyond)
    if (!mfx_join_trim(D.run_off[i], D.run_len[i], D.cnt.data() + f, D.cnt.data() + nt + f, l - f, &r.off, &r.len))
      return mfx_fail(MFX_E_FORMAT, "'%s': the k-mers of a block lie outside its place in the directory", ins[i]->path.c_str());
    D.runs.push_back(r);
  }
  return MFX_OK;
}

// not_paths: the databases whose k-mers are not written (mfx_db_merge_except); they are opened behind the inputs, share their windows and are
// decoded with counts of 0, which the combine kernel takes as "this k-mer is barred".  n_not == 0: mfx_db_merge.
static int mfx_db_merge_impl(const char *const *in_paths, uint32_t n_in, const char *const *not_paths, uint32_t n_not, const char *out_path, const mfx_db_merge_opts *o,
                             mfx_db_merge_stats *st, uint64_t *n_subtracted) {
  const char *who = n_not ? "mfx_db_merge_except" : "mfx_db_merge";
  if (st) memset(st, 0, sizeof(*st));
  if (n_subtracted) *n_subtracted = 0;
  std::vector<std::unique_ptr<MergeIn>> ins;
  if (n_not && (!not_paths || (uint64_t)n_in + n_not > MFX_MERGE_MAX_INPUTS))
    return not_paths ? mfx_fail(MFX_E_INVAL, "mfx_db_merge_except: %u inputs and %u to subtract (%u files at the most)", n_in, n_not, MFX_MERGE_MAX_INPUTS)
                     : mfx_fail(MFX_E_INVAL, "mfx_db_merge_except: null argument");
  if (int rc = merge_check(in_paths, n_in, out_path, o, ins)) return rc;
  const int k = (int)ins[0]->h.k;
  uint64_t n_read = 0;
  for (uint32_t i = 0; i < n_in; ++i) n_read += ins[i]->h.n;
  for (uint32_t j = 0; j < n_not; ++j) {
    if (!not_paths[j]) return mfx_fail(MFX_E_INVAL, "mfx_db_merge_except: null argument");
    ins.emplace_back(new MergeIn);
    if (int rc = merge_open_input(not_paths[j], *ins.back(), who)) return rc;
    if ((int)ins.back()->h.k != k)
      return mfx_fail(MFX_E_INVAL, "mfx_db_merge_except: '%s' holds %u-mers, '%s' %u-mers: the inputs and what is subtracted are of one k", not_paths[j], ins.back()->h.k,
                      in_paths[0], ins[0]->h.k);
    struct stat so, si;
    if (stat(out_path, &so) == 0 && fstat(ins.back()->fd, &si) == 0 && si.st_dev == so.st_dev && si.st_ino == so.st_ino)
      return mfx_fail(MFX_E_INVAL, "mfx_db_merge_except: the output '%s' is the subtracted database '%s'", out_path, not_paths[j]);
  }
  const uint32_t n_all_in = n_in + n_not;
  // ---- the windows, and what the largest of them takes
  MergeWindows P;
  if (int rc = merge_plan_windows(ins, k, who, P)) return rc;
  const std::vector<mfx_merge_window> &win = P.win;
  const uint64_t n_all = n_read, max_pairs = P.max_pairs, max_bytes = P.max_bytes, max_tasks = P.max_tasks, max_esc = P.max_esc;
  mfx_db_writer *w = nullptr;
  if (int rc = db_open_streamed(out_path, k, &w)) return rc;
  WriterAbort guard{w};
  w->merging = true;
  if (max_pairs) {
    DeviceBack back;
    MFX_HIP(hipSetDevice(o->device));
    // p[0], p[1]: two buffers of cap pairs, the k-mers in front of the counts: decoded runs, merge levels, combined pairs behind the writer's carry,
    // and the packed words of the one that is free by then.  p[2]: the window's blocks.  p[3]: tasks, their below / above, the inputs' error words,
    // the stats, the combine's tile offsets.  p[4], p[5]: the window's escapes.
    const uint64_t cap = max_pairs + MFX_DELTA_BLOCK, tiles = mfx_combine_tiles(max_pairs);
    const uint64_t small = max_tasks * (sizeof(mfx_merge_task) + 8) + (tiles + 1 + 3) * 8 + n_all_in * 4 + 64;
    DbDev D;
    hipError_t e = hipMalloc(&D.p[0], cap * 12);
    if (e == hipSuccess) e = hipMalloc(&D.p[1], cap * 12);
    if (e == hipSuccess) e = hipMalloc(&D.p[2], max_bytes + 8);
    if (e == hipSuccess) e = hipMalloc(&D.p[3], small);
    if (e == hipSuccess) e = hipMalloc(&D.p[4], (max_esc + 1) * 8);
    if (e == hipSuccess) e = hipMalloc(&D.p[5], (max_esc + 1) * 4);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return mfx_fail(MFX_E_NOMEM, "%s: the buffers of a window of %lu pairs (%.3f GB) do not fit the device: %s; lower MFX_MERGE_RANGE", who, (unsigned long)max_pairs,
                      ((double)cap * 24 + (double)max_bytes + (double)max_esc * 12 + (double)small) / 1e9, hipGetErrorString(e));
    }
    uint64_t *bk[2] = {(uint64_t *)D.p[0], (uint64_t *)D.p[1]};
    uint32_t *bv[2] = {(uint32_t *)((char *)D.p[0] + cap * 8), (uint32_t *)((char *)D.p[1] + cap * 8)};
    uint64_t *d_tile = (uint64_t *)D.p[3], *d_stats = d_tile + tiles + 1;
    mfx_merge_task *d_tasks = (mfx_merge_task *)(d_stats + 3);
    uint32_t *d_below = (uint32_t *)(d_tasks + max_tasks), *d_above = d_below + max_tasks, *d_err = d_above + max_tasks;
    MFX_HIP(mfx_memset_now(d_stats, 0, 24));
    StreamDev S;
    if (int rc = stream_dev_init(S, w, cap, who, "MFX_MERGE_RANGE")) return rc;
    const bool timing = getenv("MFX_DB_TIMING") != nullptr;
    MergeDecoder dec;
    if (n_not) dec.zero_from = n_in;
    dec.d_words = D.p[2]; dec.d_tasks = d_tasks; dec.d_below = d_below; dec.d_above = d_above; dec.d_err = d_err;
    dec.d_ek = (uint64_t *)D.p[4]; dec.d_ev = (uint32_t *)D.p[5];
    MFX_HIP(hipHostMalloc(&dec.pinned, max_bytes + 8, hipHostMallocDefault));
    typedef MergeRun Run;
    std::vector<Run> &runs = dec.runs, next;
    for (size_t wi = 0; wi < win.size(); ++wi) {
      if (win[wi].pairs == 0) continue;
      // ---- read and decode: one ascending run per input in buffer 0
      const int rc_dec = merge_decode_window(ins, P, wi, k, who, dec, bk[0], bv[0]);
      w->t_read += dec.t_read; w->t_decode += dec.t_decode;
      if (rc_dec) return rc_dec;
      double t0 = db_now(), t1;
      // ---- merge: a pairwise tree, from one buffer to the other
      int cur = 0;
      while (runs.size() > 1) {
        next.clear();
        uint64_t at = 0;
        for (size_t j = 0; j < runs.size(); j += 2) {
          const Run a = runs[j], b = j + 1 < runs.size() ? runs[j + 1] : Run{0, 0};
          MFX_HIP(mfx_k_merge_pairs(bk[cur] + a.off, bv[cur] + a.off, a.len, bk[cur] + b.off, bv[cur] + b.off, b.len, bk[cur ^ 1] + at, bv[cur ^ 1] + at, nullptr));
          next.push_back(Run{at, a.len + b.len});
          at += a.len + b.len;
        }
        runs.swap(next);
        cur ^= 1;
      }
      if (timing) MFX_HIP(hipStreamSynchronize(nullptr));
      t1 = db_now();
      w->t_merge += t1 - t0;
      // ---- combine and filter: behind the place of the writer's carry in the other buffer
      const uint64_t M = runs[0].len, c = w->ck.size();
      uint64_t n_out = 0;
      if (M) {
        const uint64_t mt = mfx_combine_tiles(M);
        MFX_HIP(mfx_k_combine(bk[cur] + runs[0].off, bv[cur] + runs[0].off, M, n_in, o->op, o->minV, o->maxV, d_tile, bk[cur ^ 1] + c, bv[cur ^ 1] + c, d_stats, nullptr));
        MFX_HIP(hipMemcpyAsync(&n_out, d_tile + mt, 8, hipMemcpyDeviceToHost, nullptr));
        MFX_HIP(hipStreamSynchronize(nullptr));
      }
      w->t_combine += db_now() - t1;
      if (st) ++st->windows;
      if (n_out > M) return mfx_fail(MFX_E_HIP, "%s: the combined pairs of a window are damaged", who);
      if (n_out)
        if (int rc = stream_append_device(w, S, bk[cur ^ 1], bv[cur ^ 1], n_out, bk[cur], cap * 12, who, "MFX_MERGE_RANGE")) return rc;
    }
    uint64_t stats[3] = {0, 0, 0};
    MFX_HIP(hipMemcpy(stats, d_stats, 24, hipMemcpyDeviceToHost));
    if (st) { st->n_saturated = stats[0]; st->n_filtered = stats[1]; }
    if (n_subtracted) *n_subtracted = stats[2];
  }
  guard.w = nullptr;
  uint64_t n = 0;
  if (int rc = mfx_db_writer_close(w, &n)) return rc;
  if (st) { st->n_in = n_all; st->n_out = n; }
  return MFX_OK;
}

extern "C" int mfx_db_merge(const char *const *in_paths, uint32_t n_in, const char *out_path, const mfx_db_merge_opts *o, mfx_db_merge_stats *st) {
  try { return mfx_db_merge_impl(in_paths, n_in, nullptr, 0, out_path, o, st, nullptr); }      // (nothing leaves the C ABI as an exception)
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_merge: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_merge: %s", e.what()); }
}

extern "C" int mfx_db_merge_except(const char *const *in_paths, uint32_t n_in, const char *const *not_paths, uint32_t n_not, const char *out_path,
                                   const mfx_db_merge_opts *o, mfx_db_merge_stats *st, uint64_t *n_subtracted) {
  try { return mfx_db_merge_impl(in_paths, n_in, not_paths, n_not, out_path, o, st, n_subtracted); }
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_merge_except: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_merge_except: %s", e.what()); }
}

// ---------------------------------------------------------------------------
// mfx_db_join_*: -completeness and -spectrum from two sorted databases, window by window (include/merfin_amd.h).  mfx_db_merge's windows and
// decode, then mfx_join_kernel (mfx_join.hip): the join ends in the piece sums or in the image, nothing is merged into memory or written.
// ---------------------------------------------------------------------------
namespace { enum JoinKind { JOIN_COMPLETENESS, JOIN_SPECTRUM }; }

static int db_join_impl(const char *read_path, const char *asm_path, const mfx_db_join_opts *o, JoinKind kind, double *total64, double *undrcpy64, uint64_t *img,
                        uint64_t *n_entries, mfx_db_join_stats *st) {
  const char *who = kind == JOIN_COMPLETENESS ? "mfx_db_join_completeness" : "mfx_db_join_spectrum";
  const double t_begin = db_now();
  if (st) memset(st, 0, sizeof(*st));
  // ---- every check that needs no device
  if (!read_path || !asm_path || !o || (kind == JOIN_COMPLETENESS ? (!total64 || !undrcpy64) : (!img || !n_entries))) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (kind == JOIN_COMPLETENESS && o->n_prob && (!o->probK || !o->probP)) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (kind == JOIN_SPECTRUM) {                                 // (mfx_spectrum_run's bounds and texts)
    if (o->copies < MFX_SPEC_MIN_COPIES || o->copies > MFX_SPEC_MAX_COPIES)
      return mfx_fail(MFX_E_INVAL, "%s: copies = %u is outside [%u, %u]", who, o->copies, MFX_SPEC_MIN_COPIES, MFX_SPEC_MAX_COPIES);
    if (o->max_mult < MFX_SPEC_MIN_MULT || o->max_mult > MFX_SPEC_MAX_MULT)
      return mfx_fail(MFX_E_INVAL, "%s: max_mult = %u is outside [%u, %u]", who, o->max_mult, MFX_SPEC_MIN_MULT, MFX_SPEC_MAX_MULT);
  }
  std::vector<std::unique_ptr<MergeIn>> ins;
  const char *paths[2] = {read_path, asm_path};
  for (int i = 0; i < 2; ++i) {
    ins.emplace_back(new MergeIn);
    mfx_db_info info;                                            // (k > 31 has no sorted form: said as that, not as "a plain flat file")
    if (detect(paths[i]) == MFX_DB_FLAT && mfx_db_probe_impl(paths[i], &info) == MFX_OK && info.k > MFX_MAX_K_NARROW)
      return mfx_fail(MFX_E_INVAL, "mfx_db_join: '%s' holds %d-mers: the sorted join takes k <= %d", paths[i], info.k, MFX_MAX_K_NARROW);
    if (int rc = merge_open_input(paths[i], *ins.back(), "mfx_db_join")) return rc;
  }
  if (ins[1]->h.k != ins[0]->h.k)
    return mfx_fail(MFX_E_INVAL, "mfx_db_join: '%s' holds %u-mers, '%s' %u-mers: the inputs are of one k", paths[1], ins[1]->h.k, paths[0], ins[0]->h.k);
  const int k = (int)ins[0]->h.k;
  MergeWindows P;
  if (int rc = merge_plan_windows(ins, k, who, P)) return rc;
  const size_t cells = kind == JOIN_SPECTRUM ? (size_t)(o->copies + 2u) * (o->max_mult + 1u) : 0;
  // res: stats word [0] (the k-mers of both), then the 128 piece sums or the image and its entry counter
  const size_t res_words = 2 + (kind == JOIN_COMPLETENESS ? 128 : cells + 1);
  std::vector<uint64_t> res(res_words, 0);
  uint64_t got[2] = {0, 0}, windows = 0;
  double t_read = 0, t_decode = 0, t_join = 0;
  if (P.max_pairs) {
    DeviceBack back;
    MFX_HIP(hipSetDevice(o->device));
    // p[0]: one buffer of cap pairs, the k-mers in front of the counts: the decoded runs.  p[1]: the window's blocks.  p[2]: tasks, their below /
    // above, the inputs' error words.  p[3], p[4]: the window's escapes.  p[5]: the result.  p[6], p[7]: the -prob table.
    const uint64_t cap = P.max_pairs + 1, small = P.max_tasks * (sizeof(mfx_merge_task) + 8) + 2 * 4 + 64;
    const size_t np = o->n_prob && kind == JOIN_COMPLETENESS ? o->n_prob : 1;
    DbDev D;
    hipError_t e = hipMalloc(&D.p[0], cap * 12);
    if (e == hipSuccess) e = hipMalloc(&D.p[1], P.max_bytes + 8);
    if (e == hipSuccess) e = hipMalloc(&D.p[2], small);
    if (e == hipSuccess) e = hipMalloc(&D.p[3], (P.max_esc + 1) * 8);
    if (e == hipSuccess) e = hipMalloc(&D.p[4], (P.max_esc + 1) * 4);
    if (e == hipSuccess) e = hipMalloc(&D.p[5], res_words * 8);
    if (e == hipSuccess) e = hipMalloc(&D.p[6], np * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&D.p[7], np * sizeof(double));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return mfx_fail(MFX_E_NOMEM, "%s: the buffers of a window of %lu pairs (%.3f GB) do not fit the device: %s; lower MFX_MERGE_RANGE", who, (unsigned long)P.max_pairs,
                      ((double)cap * 12 + (double)P.max_bytes + (double)P.max_esc * 12 + (double)small + (double)res_words * 8) / 1e9, hipGetErrorString(e));
    }
    uint64_t *d_keys = (uint64_t *)D.p[0], *d_res = (uint64_t *)D.p[5];
    uint32_t *d_vals = (uint32_t *)((char *)D.p[0] + cap * 8);
    MergeDecoder dec;
    dec.d_words = D.p[1];
    dec.d_tasks = (mfx_merge_task *)D.p[2];
    dec.d_below = (uint32_t *)(dec.d_tasks + P.max_tasks); dec.d_above = dec.d_below + P.max_tasks; dec.d_err = dec.d_above + P.max_tasks;
    dec.d_ek = (uint64_t *)D.p[3]; dec.d_ev = (uint32_t *)D.p[4];
    MFX_HIP(hipHostMalloc(&dec.pinned, P.max_bytes + 8, hipHostMallocDefault));
    MFX_HIP(mfx_memset_now(d_res, 0, res_words * 8));
    if (kind == JOIN_COMPLETENESS && o->n_prob) {
      MFX_HIP(hipMemcpy(D.p[6], o->probK, o->n_prob * sizeof(uint32_t), hipMemcpyHostToDevice));
      MFX_HIP(hipMemcpy(D.p[7], o->probP, o->n_prob * sizeof(double), hipMemcpyHostToDevice));
    }
    int cus = 0;
    MFX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, o->device));
    const int grid = (cus > 0 ? cus : 256) * (kind == JOIN_COMPLETENESS ? 4 : 2);      // the workgroups a CU holds at once (mfx_join.hip: LDS)
    mfx_spectrum_args sa{};
    if (kind == JOIN_SPECTRUM) {
      sa.copies = o->copies;
      sa.max_mult = o->max_mult;
      sa.lds_cols = mfx_spec_lds_cols(o->copies, o->max_mult);
      const char *ag = getenv("MFX_SPECTRUM_AGG");                 // as mfx_spectrum_run reads it (docs/KNOBS.md)
      sa.aggregate = ag ? (atoi(ag) != 0) : MFX_SPEC_AGG_DEFAULT;
      sa.img = d_res + 2;
    }
    const bool timing = getenv("MFX_DB_TIMING") != nullptr;
    for (size_t wi = 0; wi < P.win.size(); ++wi) {
      if (P.win[wi].pairs == 0) continue;
      // ---- read and decode: the read run and the asm run of the window.  (One stream: the blocks of this window are copied behind the join of
      // the window before it, whose kernel runs while the host reads.)
      const int rc = merge_decode_window(ins, P, wi, k, who, dec, d_keys, d_vals);
      t_read += dec.t_read; t_decode += dec.t_decode;
      if (rc) return rc;
      const double t0 = db_now();
      const MergeRun a = dec.runs[0], b = dec.runs[1];
      got[0] += a.len; got[1] += b.len;
      if (kind == JOIN_COMPLETENESS)
        MFX_HIP(mfx_k_join_completeness(d_keys + a.off, d_vals + a.off, a.len, d_keys + b.off, d_vals + b.off, b.len, k, o->peak, o->n_prob, (const uint32_t *)D.p[6],
                                        (const double *)D.p[7], reinterpret_cast<double *>(d_res + 2), d_res, grid, nullptr));
      else
        MFX_HIP(mfx_k_join_spectrum(d_keys + a.off, d_vals + a.off, a.len, d_keys + b.off, d_vals + b.off, b.len, sa, o->minV, o->maxV, d_res, grid, nullptr));
      if (timing) MFX_HIP(hipStreamSynchronize(nullptr));
      t_join += db_now() - t0;
      ++windows;
    }
    MFX_HIP(hipMemcpy(res.data(), d_res, res_words * 8, hipMemcpyDeviceToHost));
  }
  // ---- what the windows held against what the files say, the image against its counter: no partial result is handed out
  for (int i = 0; i < 2; ++i)
    if (got[i] != ins[i]->h.n)
      return mfx_fail(MFX_E_FORMAT, "'%s': the windows hold %lu of its %lu k-mers: the directory does not describe the blocks", paths[i], (unsigned long)got[i], (unsigned long)ins[i]->h.n);
  const uint64_t n_both = res[0];
  if (n_both > got[0] || n_both > got[1]) return mfx_fail(MFX_E_HIP, "%s: %lu k-mers in both inputs, more than an input holds", who, (unsigned long)n_both);
  if (kind == JOIN_SPECTRUM) {
    uint64_t sum = 0;
    for (size_t i = 0; i < cells; ++i) sum += res[2 + i];
    if (sum != res[2 + cells]) return mfx_fail(MFX_E_HIP, "%s: the image sums to %lu, the join counted %lu entries", who, (unsigned long)sum, (unsigned long)res[2 + cells]);
    const bool filtered = o->minV > 1 || o->maxV < 0xffffffffull;      // (a count is 1 at the least: no other filter makes a pair (0, 0))
    if (!filtered && sum != got[0] + got[1] - n_both)
      return mfx_fail(MFX_E_HIP, "%s: the join counted %lu entries, the inputs hold %lu distinct k-mers", who, (unsigned long)sum, (unsigned long)(got[0] + got[1] - n_both));
    memcpy(img, res.data() + 2, cells * 8);
    *n_entries = sum;
  } else {
    memcpy(total64, res.data() + 2, 64 * sizeof(double));
    memcpy(undrcpy64, res.data() + 2 + 64, 64 * sizeof(double));
  }
  if (st) {
    st->n_read = got[0]; st->n_asm = got[1]; st->n_both = n_both; st->windows = windows;
    st->t_read = t_read; st->t_decode = t_decode; st->t_join = t_join; st->t_total = db_now() - t_begin;
  }
  return MFX_OK;
}

extern "C" int mfx_db_join_completeness(const char *read_path, const char *asm_path, const mfx_db_join_opts *o, double *total64, double *undrcpy64, mfx_db_join_stats *st) {
  try { return db_join_impl(read_path, asm_path, o, JOIN_COMPLETENESS, total64, undrcpy64, nullptr, nullptr, st); }      // (nothing leaves the C ABI as an exception)
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_join_completeness: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_join_completeness: %s", e.what()); }
}

extern "C" int mfx_db_join_spectrum(const char *read_path, const char *asm_path, const mfx_db_join_opts *o, uint64_t *img, uint64_t *n_entries, mfx_db_join_stats *st) {
  try { return db_join_impl(read_path, asm_path, o, JOIN_SPECTRUM, nullptr, nullptr, img, n_entries, st); }
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_join_spectrum: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_join_spectrum: %s", e.what()); }
}

extern "C" void mfx_db_join_grain(uint32_t *per_lane, uint32_t *tile) {
  if (per_lane) *per_lane = MFX_JOIN_PER;
  if (tile) *tile = MFX_JOIN_TILE;
}

extern "C" int mfx_db_join_host(const uint64_t *read_keys, const uint32_t *read_vals, uint64_t n_read, const uint64_t *asm_keys, const uint32_t *asm_vals, uint64_t n_asm,
                                uint64_t *keys, uint32_t *readV, uint32_t *asmV, uint64_t cap, uint64_t *n_pairs) {
  if ((n_read && (!read_keys || !read_vals)) || (n_asm && (!asm_keys || !asm_vals)) || !n_pairs || (cap && (!keys || !readV || !asmV)))
    return mfx_fail(MFX_E_INVAL, "mfx_db_join_host: null argument");
  uint64_t n = 0;
  try {
    mfx_join_host(read_keys, read_vals, n_read, asm_keys, asm_vals, n_asm, [&](bool have, uint64_t key, uint32_t rv, uint32_t av) {
      if (!have) return;
      if (n < cap) { keys[n] = key; readV[n] = rv; asmV[n] = av; }
      ++n;
    });
  } catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_join_host: out of memory"); }
  *n_pairs = n;
  return MFX_OK;
}

// ---------------------------------------------------------------------------
// mfx_db_diploid: two haplotype assemblies against the reads, window by window (include/merfin_amd.h; the rule: mfx_diploid.h; the kernels:
// mfx_diploid.hip).  mfx_db_merge's windows and decode over the three files; hap1's and hap2's runs are tagged, merged (mfx_merge_pairs_kernel)
// and compacted into the pair run; the read run stays where the decode left it and is joined against the pair run by mfx_join_kernel.
// ---------------------------------------------------------------------------
static void diploid_fill_stats(const uint64_t *c, mfx_db_diploid_stats *st) {
  mfx_diploid_counts *x[3] = {&st->hap1, &st->hap2, &st->both};
  for (int i = 0; i < 3; ++i) {
    const uint64_t *s = c + i * MFX_DIP_PER_X;
    x[i]->distinct = s[MFX_DIP_DISTINCT]; x[i]->total = s[MFX_DIP_TOTAL]; x[i]->only_distinct = s[MFX_DIP_ONLY_DISTINCT];
    x[i]->only_total = s[MFX_DIP_ONLY_TOTAL]; x[i]->found = s[MFX_DIP_FOUND];
  }
  st->solid = c[MFX_DIP_SOLID]; st->n_read = c[MFX_DIP_N_READ]; st->n_shared = c[MFX_DIP_N_SHARED];
}

static int diploid_check_opts(const char *who, const mfx_db_join_opts *o, const uint64_t *asm_img, const uint64_t *cn_img, const uint64_t *n_entries,
                              const mfx_db_diploid_stats *st, const double *total64, const double *undrcpy64) {
  if (!o || !asm_img || !cn_img || !n_entries || !st) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if ((total64 != nullptr) != (undrcpy64 != nullptr)) return mfx_fail(MFX_E_INVAL, "%s: total64 and undrcpy64 are given together or not at all", who);
  if (total64 && o->n_prob && (!o->probK || !o->probP)) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (o->copies < MFX_SPEC_MIN_COPIES || o->copies > MFX_SPEC_MAX_COPIES)      // (mfx_spectrum_run's bounds and texts)
    return mfx_fail(MFX_E_INVAL, "%s: copies = %u is outside [%u, %u]", who, o->copies, MFX_SPEC_MIN_COPIES, MFX_SPEC_MAX_COPIES);
  if (o->max_mult < MFX_SPEC_MIN_MULT || o->max_mult > MFX_SPEC_MAX_MULT)
    return mfx_fail(MFX_E_INVAL, "%s: max_mult = %u is outside [%u, %u]", who, o->max_mult, MFX_SPEC_MIN_MULT, MFX_SPEC_MAX_MULT);
  return MFX_OK;
}

static int db_diploid_impl(const char *read_path, const char *hap1_path, const char *hap2_path, const mfx_db_join_opts *o, uint64_t *asm_img, uint64_t *cn_img,
                           uint64_t *n_entries, mfx_db_diploid_stats *st, double *total64, double *undrcpy64) {
  const char *who = "mfx_db_diploid";
  const double t_begin = db_now();
  // ---- every check that needs no device
  if (!read_path || !hap1_path || !hap2_path) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (int rc = diploid_check_opts(who, o, asm_img, cn_img, n_entries, st, total64, undrcpy64)) return rc;
  const bool pieces = total64 != nullptr;
  std::vector<std::unique_ptr<MergeIn>> ins;
  const char *paths[3] = {read_path, hap1_path, hap2_path};
  for (int i = 0; i < 3; ++i) {
    ins.emplace_back(new MergeIn);
    mfx_db_info info;                                            // (k > 31 has no sorted form: said as that, not as "a plain flat file")
    if (detect(paths[i]) == MFX_DB_FLAT && mfx_db_probe_impl(paths[i], &info) == MFX_OK && info.k > MFX_MAX_K_NARROW)
      return mfx_fail(MFX_E_INVAL, "%s: '%s' holds %d-mers: the sorted join takes k <= %d", who, paths[i], info.k, MFX_MAX_K_NARROW);
    if (int rc = merge_open_input(paths[i], *ins.back(), who)) return rc;
    if (ins[i]->h.k != ins[0]->h.k)
      return mfx_fail(MFX_E_INVAL, "%s: '%s' holds %u-mers, '%s' %u-mers: the inputs are of one k", who, paths[i], ins[i]->h.k, paths[0], ins[0]->h.k);
  }
  const int k = (int)ins[0]->h.k;
  MergeWindows P;
  if (int rc = merge_plan_windows(ins, k, who, P)) return rc;
  uint64_t max_asm = 0;                                        // the most a window's blocks hold of the two assemblies together
  for (size_t w = 0; w < P.win.size(); ++w) {
    uint64_t a = 0;
    for (uint32_t i = 1; i < 3; ++i) a += mfx_merge_block_pairs(P.pin[i], P.blk[2 * (w * 3 + i)], P.blk[2 * (w * 3 + i) + 1]);
    max_asm = std::max(max_asm, a);
  }
  const uint64_t W = (uint64_t)o->max_mult + 1, cls_cells = MFX_DIP_ROWS * W, cn_cells = (uint64_t)(o->copies + 2u) * W;
  // res: [0] the k-mers of the reads and of an assembly, [1] spare; the class image and its counter word; the cn image and its counter word;
  // the 256 piece sums; the copies of the counters
  const size_t off_cls = 2, off_cn = off_cls + cls_cells + 1, off_sums = off_cn + cn_cells + 1, off_cnt = off_sums + 256, res_words = off_cnt + MFX_DIP_STAT_WORDS;
  std::vector<uint64_t> res(res_words, 0);
  uint64_t got[3] = {0, 0, 0}, windows = 0;
  double t_read = 0, t_decode = 0, t_pair = 0, t_join = 0;
  if (P.max_pairs) {
    DeviceBack back;
    MFX_HIP(hipSetDevice(o->device));
    // p[0]: one buffer of cap pairs, the k-mers in front of the counts: the decoded runs of the three inputs.  p[1]: the window's blocks.  p[2]: tasks,
    // their below / above, the inputs' error words, the pair kernel's tile offsets.  p[3], p[4]: the window's escapes.  p[5]: the result.  p[6], p[7]: the
    // -prob table.  E.p[0]: the tagged merged run of the two assemblies (acap pairs).  E.p[1]: the pair run (acap k-mers, acap words).
    const uint64_t cap = P.max_pairs + 1, acap = max_asm + 1, tiles = mfx_dip_tiles(max_asm);
    const uint64_t small = P.max_tasks * (sizeof(mfx_merge_task) + 8) + 3 * 4 + 64 + (tiles + 1) * 8;
    const size_t np = o->n_prob && pieces ? o->n_prob : 1;
    DbDev D, E;
    hipError_t e = hipMalloc(&D.p[0], cap * 12);
    if (e == hipSuccess) e = hipMalloc(&D.p[1], P.max_bytes + 8);
    if (e == hipSuccess) e = hipMalloc(&D.p[2], small);
    if (e == hipSuccess) e = hipMalloc(&D.p[3], (P.max_esc + 1) * 8);
    if (e == hipSuccess) e = hipMalloc(&D.p[4], (P.max_esc + 1) * 4);
    if (e == hipSuccess) e = hipMalloc(&D.p[5], res_words * 8);
    if (e == hipSuccess) e = hipMalloc(&D.p[6], np * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&D.p[7], np * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&E.p[0], acap * 12);
    if (e == hipSuccess) e = hipMalloc(&E.p[1], acap * 16);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return mfx_fail(MFX_E_NOMEM, "%s: the buffers of a window of %lu pairs, %lu of them the assemblies' (%.3f GB) do not fit the device: %s; lower MFX_MERGE_RANGE", who,
                      (unsigned long)P.max_pairs, (unsigned long)max_asm,
                      ((double)cap * 12 + (double)acap * 28 + (double)P.max_bytes + (double)P.max_esc * 12 + (double)small + (double)res_words * 8) / 1e9, hipGetErrorString(e));
    }
    uint64_t *d_keys = (uint64_t *)D.p[0], *d_res = (uint64_t *)D.p[5];
    uint32_t *d_vals = (uint32_t *)((char *)D.p[0] + cap * 8);
    uint64_t *m_keys = (uint64_t *)E.p[0], *p_keys = (uint64_t *)E.p[1], *p_vals = p_keys + acap;
    uint32_t *m_vals = (uint32_t *)((char *)E.p[0] + acap * 8);
    MergeDecoder dec;
    dec.d_words = D.p[1];
    uint64_t *d_tile = (uint64_t *)D.p[2];
    dec.d_tasks = (mfx_merge_task *)(d_tile + tiles + 1);
    dec.d_below = (uint32_t *)(dec.d_tasks + P.max_tasks); dec.d_above = dec.d_below + P.max_tasks; dec.d_err = dec.d_above + P.max_tasks;
    dec.d_ek = (uint64_t *)D.p[3]; dec.d_ev = (uint32_t *)D.p[4];
    MFX_HIP(hipHostMalloc(&dec.pinned, P.max_bytes + 8, hipHostMallocDefault));
    MFX_HIP(mfx_memset_now(d_res, 0, res_words * 8));
    if (pieces && o->n_prob) {
      MFX_HIP(hipMemcpy(D.p[6], o->probK, o->n_prob * sizeof(uint32_t), hipMemcpyHostToDevice));
      MFX_HIP(hipMemcpy(D.p[7], o->probP, o->n_prob * sizeof(double), hipMemcpyHostToDevice));
    }
    int cus = 0;
    MFX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, o->device));
    const int grid = (cus > 0 ? cus : 256) * 2;                  // the workgroups a CU holds at once (mfx_diploid.hip: LDS)
    mfx_spectrum_args cls{}, cn{};
    const char *ag = getenv("MFX_SPECTRUM_AGG");                 // as mfx_spectrum_run reads it (docs/KNOBS.md)
    cls.copies = MFX_DIP_ROWS - 2u; cn.copies = o->copies;
    cls.max_mult = cn.max_mult = o->max_mult;
    cls.lds_cols = cn.lds_cols = mfx_dip_lds_cols(o->copies, o->max_mult);
    cls.aggregate = cn.aggregate = ag ? (atoi(ag) != 0) : MFX_SPEC_AGG_DEFAULT;
    cls.img = d_res + off_cls; cn.img = d_res + off_cn;
    const bool timing = getenv("MFX_DB_TIMING") != nullptr;
    for (size_t wi = 0; wi < P.win.size(); ++wi) {
      if (P.win[wi].pairs == 0) continue;
      const int rc = merge_decode_window(ins, P, wi, k, who, dec, d_keys, d_vals);
      t_read += dec.t_read; t_decode += dec.t_decode;
      if (rc) return rc;
      double t0 = db_now();
      const MergeRun a = dec.runs[0], h1 = dec.runs[1], h2 = dec.runs[2];
      got[0] += a.len; got[1] += h1.len; got[2] += h2.len;
      // ---- a. the pair run: the role into the two low bits of the assemblies' k-mers, one merge, the head positions compacted
      const uint64_t M = h1.len + h2.len;
      uint64_t n_pairs = 0;
      if (M > max_asm) return mfx_fail(MFX_E_INVAL, "%s: a window does not match its plan", who);      // (nothing is merged beyond the buffers)
      if (M) {
        MFX_HIP(mfx_k_trio_tag(d_keys + h1.off, h1.len, MFX_DIP_HAP1, nullptr));
        MFX_HIP(mfx_k_trio_tag(d_keys + h2.off, h2.len, MFX_DIP_HAP2, nullptr));
        MFX_HIP(mfx_k_merge_pairs(d_keys + h1.off, d_vals + h1.off, h1.len, d_keys + h2.off, d_vals + h2.off, h2.len, m_keys, m_vals, nullptr));
        MFX_HIP(mfx_k_dip_pairs(m_keys, m_vals, M, d_tile, p_keys, p_vals, nullptr));
        MFX_HIP(hipMemcpyAsync(&n_pairs, d_tile + mfx_dip_tiles(M), 8, hipMemcpyDeviceToHost, nullptr));
        MFX_HIP(hipStreamSynchronize(nullptr));
      }
      if (n_pairs > M || 2 * n_pairs < M) return mfx_fail(MFX_E_HIP, "%s: the pair run of a window is damaged", who);
      double t1 = db_now();
      t_pair += t1 - t0;
      // ---- b. the join of the read run against it
      MFX_HIP(mfx_k_dip_join(d_keys + a.off, d_vals + a.off, a.len, p_keys, p_vals, n_pairs, cls, cn, o->minV, o->maxV, k, pieces ? 1 : 0, o->peak,
                             pieces ? o->n_prob : 0u, (const uint32_t *)D.p[6], (const double *)D.p[7], reinterpret_cast<double *>(d_res + off_sums), d_res + off_cnt,
                             d_res, grid, nullptr));
      if (timing) MFX_HIP(hipStreamSynchronize(nullptr));
      t_join += db_now() - t1;
      ++windows;
    }
    MFX_HIP(hipMemcpy(res.data(), d_res, res_words * 8, hipMemcpyDeviceToHost));
  }
  // ---- what the windows held against what the files say, the counters against the files, the images against their counters: no partial result
  for (int i = 0; i < 3; ++i)
    if (got[i] != ins[i]->h.n)
      return mfx_fail(MFX_E_FORMAT, "'%s': the windows hold %lu of its %lu k-mers: the directory does not describe the blocks", paths[i], (unsigned long)got[i], (unsigned long)ins[i]->h.n);
  uint64_t c[MFX_DIP_NSTATS];
  for (uint32_t s = 0; s < MFX_DIP_NSTATS; ++s) {
    c[s] = 0;
    for (uint32_t j = 0; j < MFX_DIP_STAT_SHARDS; ++j) c[s] += res[off_cnt + j * MFX_DIP_STAT_STRIDE + s];
  }
  const uint64_t d1 = c[MFX_DIP_DISTINCT], d2 = c[MFX_DIP_PER_X + MFX_DIP_DISTINCT], db = c[2 * MFX_DIP_PER_X + MFX_DIP_DISTINCT];
  if (d1 != got[1] || d2 != got[2] || c[MFX_DIP_N_READ] != got[0] || d1 + d2 - c[MFX_DIP_N_SHARED] != db ||
      res[0] != db - c[2 * MFX_DIP_PER_X + MFX_DIP_ONLY_DISTINCT])
    return mfx_fail(MFX_E_HIP, "%s: the join counted %lu, %lu and %lu k-mers of the reads, hap1 and hap2 (%lu shared, %lu of either, %lu of the reads and an assembly): "
                    "not what databases of %lu, %lu and %lu k-mers give", who, (unsigned long)c[MFX_DIP_N_READ], (unsigned long)d1, (unsigned long)d2,
                    (unsigned long)c[MFX_DIP_N_SHARED], (unsigned long)db, (unsigned long)res[0], (unsigned long)got[0], (unsigned long)got[1], (unsigned long)got[2]);
  uint64_t sum_cls = 0, sum_cn = 0;
  for (size_t i = 0; i < cls_cells; ++i) sum_cls += res[off_cls + i];
  for (size_t i = 0; i < cn_cells; ++i) sum_cn += res[off_cn + i];
  if (sum_cls != res[off_cls + cls_cells] || sum_cn != res[off_cn + cn_cells] || sum_cls != sum_cn)
    return mfx_fail(MFX_E_HIP, "%s: the images sum to %lu and %lu, the join counted %lu and %lu entries", who, (unsigned long)sum_cls, (unsigned long)sum_cn,
                    (unsigned long)res[off_cls + cls_cells], (unsigned long)res[off_cn + cn_cells]);
  const bool filtered = o->minV > 1 || o->maxV < 0xffffffffull;      // (a count is 1 at the least: no other filter makes an entry vanish)
  if (!filtered && sum_cn != got[0] + db - res[0])
    return mfx_fail(MFX_E_HIP, "%s: the join counted %lu entries, the inputs hold %lu distinct k-mers", who, (unsigned long)sum_cn, (unsigned long)(got[0] + db - res[0]));
  memcpy(asm_img, res.data() + off_cls, cls_cells * 8);
  memcpy(cn_img, res.data() + off_cn, cn_cells * 8);
  *n_entries = sum_cn;
  if (pieces) {
    memcpy(total64, res.data() + off_sums, 64 * sizeof(double));
    memcpy(undrcpy64, res.data() + off_sums + 64, 3 * 64 * sizeof(double));
  }
  memset(st, 0, sizeof(*st));
  diploid_fill_stats(c, st);
  st->n_hap1 = got[1]; st->n_hap2 = got[2]; st->windows = windows;
  st->t_read = t_read; st->t_decode = t_decode; st->t_pair = t_pair; st->t_join = t_join; st->t_total = db_now() - t_begin;
  return MFX_OK;
}

extern "C" int mfx_db_diploid(const char *read_path, const char *hap1_path, const char *hap2_path, const mfx_db_join_opts *o, uint64_t *asm_img, uint64_t *cn_img,
                              uint64_t *n_entries, mfx_db_diploid_stats *st, double *total64, double *undrcpy64) {
  try { return db_diploid_impl(read_path, hap1_path, hap2_path, o, asm_img, cn_img, n_entries, st, total64, undrcpy64); }      // (nothing leaves the C ABI as an exception)
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_diploid: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_diploid: %s", e.what()); }
}

extern "C" int mfx_db_diploid_host(const uint64_t *read_keys, const uint32_t *read_vals, uint64_t n_read, const uint64_t *hap1_keys, const uint32_t *hap1_vals,
                                   uint64_t n_hap1, const uint64_t *hap2_keys, const uint32_t *hap2_vals, uint64_t n_hap2, int k, const mfx_db_join_opts *o, uint64_t *keys,
                                   uint32_t *readV, uint32_t *c1V, uint32_t *c2V, uint64_t cap, uint64_t *n_kmers, uint64_t *asm_img, uint64_t *cn_img, uint64_t *n_entries,
                                   mfx_db_diploid_stats *st, double *total64, double *undrcpy64) {
  const char *who = "mfx_db_diploid_host";
  if ((n_read && (!read_keys || !read_vals)) || (n_hap1 && (!hap1_keys || !hap1_vals)) || (n_hap2 && (!hap2_keys || !hap2_vals)) || !n_kmers ||
      (cap && (!keys || !readV || !c1V || !c2V)))
    return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (int rc = diploid_check_opts(who, o, asm_img, cn_img, n_entries, st, total64, undrcpy64)) return rc;
  if (k < 1 || k > MFX_MAX_K_NARROW) return mfx_fail(MFX_E_INVAL, "%s: k = %d is outside [1, %d]", who, k, MFX_MAX_K_NARROW);
  try {
    mfx_dip_host_result R;
    uint64_t n = 0;
    mfx_dip_host(read_keys, read_vals, n_read, hap1_keys, hap1_vals, n_hap1, hap2_keys, hap2_vals, n_hap2, k, o->minV, o->maxV, o->copies, o->max_mult, total64 != nullptr,
                 [&](uint32_t r) { double rk, pr; mfx_getK_core(o->peak, o->n_prob, o->probK, o->probP, r, rk, pr); return rk; },
                 [&](uint64_t key, uint32_t r, uint32_t c1, uint32_t c2) {
                   if (n < cap) { keys[n] = key; readV[n] = r; c1V[n] = c1; c2V[n] = c2; }
                   ++n;
                 }, R);
    if (R.stats[MFX_DIP_DISTINCT] != n_hap1 || R.stats[MFX_DIP_PER_X + MFX_DIP_DISTINCT] != n_hap2 || R.stats[MFX_DIP_N_READ] != n_read)
      return mfx_fail(MFX_E_INVAL, "%s: the runs do not ascend strictly, or hold a count of 0", who);
    *n_kmers = n;
    memcpy(asm_img, R.asm_img.data(), R.asm_img.size() * 8);
    memcpy(cn_img, R.cn_img.data(), R.cn_img.size() * 8);
    *n_entries = R.n_entries;
    if (total64) { memcpy(total64, R.tot, sizeof(R.tot)); memcpy(undrcpy64, R.und, sizeof(R.und)); }
    memset(st, 0, sizeof(*st));
    diploid_fill_stats(R.stats, st);
    st->n_hap1 = n_hap1; st->n_hap2 = n_hap2;
    return MFX_OK;
  } catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "%s: out of memory", who); }
}

extern "C" int mfx_diploid_write_asm(const uint64_t *img, uint32_t max_mult, const char *path) {
  if (!img || !path) return mfx_fail(MFX_E_INVAL, "mfx_diploid_write_asm: null argument");
  if (max_mult < MFX_SPEC_MIN_MULT || max_mult > MFX_SPEC_MAX_MULT)
    return mfx_fail(MFX_E_INVAL, "mfx_diploid_write_asm: max_mult = %u is outside [%u, %u]", max_mult, MFX_SPEC_MIN_MULT, MFX_SPEC_MAX_MULT);
  static const char *const label[MFX_DIP_ROWS] = {"read-only", "hap1-only", "hap2-only", "shared"};
  mfx_file fh = mfx_open_writer(path, false);                    // compressor chosen by suffix (mfx_pipe.h)
  if (!fh.f) return mfx_fail(MFX_E_IO, "mfx_diploid_write_asm: cannot open '%s' for writing", path);
  fprintf(fh.f, "Assembly\tkmer_multiplicity\tCount\n");
  for (uint32_t r = 0; r < MFX_DIP_ROWS; ++r)
    for (uint32_t m = 0; m <= max_mult; ++m)
      if (img[(size_t)r * (max_mult + 1u) + m]) fprintf(fh.f, "%s\t%u\t%llu\n", label[r], m, (unsigned long long)img[(size_t)r * (max_mult + 1u) + m]);
  if (mfx_close(fh)) return mfx_fail(MFX_E_IO, "mfx_diploid_write_asm: writing '%s' failed", path);
  return MFX_OK;
}

extern "C" int mfx_db_merge_plan(const uint64_t *const *first, const uint64_t *n, uint32_t n_in, int k, uint64_t R, uint64_t *out, uint64_t cap, uint64_t *n_windows) {
  if (!first || !n || !n_windows || n_in == 0 || n_in > MFX_MERGE_MAX_INPUTS || k < 1 || k > MFX_MAX_K_NARROW) return mfx_fail(MFX_E_INVAL, "mfx_db_merge_plan: bad argument");
  try {
    std::vector<mfx_merge_input> in(n_in);
    for (uint32_t i = 0; i < n_in; ++i) in[i] = mfx_merge_input{first[i], 1u, (n[i] + MFX_MERGE_BLOCK - 1) / MFX_MERGE_BLOCK, n[i]};
    std::vector<mfx_merge_window> win;
    std::vector<uint64_t> blk;
    mfx_merge_plan(in.data(), n_in, k, R, win, blk);
    *n_windows = win.size();
    const uint64_t row = 3 + 2 * (uint64_t)n_in;
    for (uint64_t w = 0; out && w < win.size() && w < cap; ++w) {
      out[w * row] = win[w].lo; out[w * row + 1] = win[w].hi; out[w * row + 2] = win[w].pairs;
      for (uint64_t j = 0; j < 2 * (uint64_t)n_in; ++j) out[w * row + 3 + j] = blk[w * 2 * n_in + j];
    }
    return MFX_OK;
  } catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_merge_plan: out of memory"); }
}

// ---------------------------------------------------------------------------
// mfx_db_trio, mfx_db_trio_hist, mfx_db_histogram: the hap-mer sets of a trio and the k-mer histograms their cutoffs are read off
// (include/merfin_amd.h; the rule: mfx_trio.h; the kernels: mfx_trio.hip).  mfx_db_merge's windows, pread loop, decode and pairwise merge as
// they are; between decode and merge every input's k-mers take its role into their two low bits, so that the merged run knows its inputs.
// Pass 1 (only where a cutoff is automatic, and for the two histogram calls) ends in the image; pass 2 in two compacted outputs, each behind
// the carry of a streamed writer of its own.
// ---------------------------------------------------------------------------
namespace {
enum TrioKind { TRIO_FULL, TRIO_HIST, TRIO_HISTOGRAM };
struct TrioTimes { double read = 0, decode = 0, merge = 0, hist = 0, classify = 0, write = 0; };
}  // namespace

static int trio_impl(TrioKind kind, const char *mat_path, const char *pat_path, const char *child_path, const char *out_a, const char *out_b, const mfx_db_trio_opts *o,
                     uint64_t *img, mfx_db_trio_stats *st) {
  const char *who = kind == TRIO_FULL ? "mfx_db_trio" : kind == TRIO_HIST ? "mfx_db_trio_hist" : "mfx_db_histogram";
  const double t_begin = db_now();
  if (st) memset(st, 0, sizeof(*st));
  // ---- every check that needs no device
  if (!o || (kind != TRIO_HISTOGRAM && (!mat_path || !pat_path)) || (kind == TRIO_HISTOGRAM && !child_path) || (kind == TRIO_FULL ? (!out_a || !out_b) : !img))
    return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (o->max_mult < MFX_SPEC_MIN_MULT || o->max_mult > MFX_SPEC_MAX_MULT)
    return mfx_fail(MFX_E_INVAL, "%s: max_mult = %u is outside [%u, %u]", who, o->max_mult, MFX_SPEC_MIN_MULT, MFX_SPEC_MAX_MULT);
  if (kind == TRIO_FULL && o->cut_child != 0 && !child_path)
    return mfx_fail(MFX_E_INVAL, "mfx_db_trio: cut_child = %u without a child database: the child's cutoff has nothing to act on", o->cut_child);
  const bool has_child = child_path != nullptr;
  std::vector<const char *> paths;
  std::vector<uint32_t> roles;
  if (kind != TRIO_HISTOGRAM) { paths.push_back(mat_path); roles.push_back(MFX_TRIO_MAT); paths.push_back(pat_path); roles.push_back(MFX_TRIO_PAT); }
  if (has_child) { paths.push_back(child_path); roles.push_back(MFX_TRIO_CHILD); }
  const uint32_t n_in = (uint32_t)paths.size();
  std::vector<std::unique_ptr<MergeIn>> ins;
  for (uint32_t i = 0; i < n_in; ++i) {
    ins.emplace_back(new MergeIn);
    mfx_db_info info;                                            // (k > 31 has no sorted form: said as that, not as "a plain flat file")
    if (detect(paths[i]) == MFX_DB_FLAT && mfx_db_probe_impl(paths[i], &info) == MFX_OK && info.k > MFX_MAX_K_NARROW)
      return mfx_fail(MFX_E_INVAL, "%s: '%s' holds %d-mers: the sorted databases of this call hold k <= %d", who, paths[i], info.k, MFX_MAX_K_NARROW);
    if (int rc = merge_open_input(paths[i], *ins.back(), who)) return rc;
    if (ins[i]->h.k != ins[0]->h.k)
      return mfx_fail(MFX_E_INVAL, "%s: '%s' holds %u-mers, '%s' %u-mers: the inputs are of one k", who, paths[i], ins[i]->h.k, paths[0], ins[0]->h.k);
  }
  const int k = (int)ins[0]->h.k;
  if (kind == TRIO_FULL) {
    const char *outs[2] = {out_a, out_b};
    struct stat so[2];
    bool have[2];
    for (int j = 0; j < 2; ++j) {
      have[j] = stat(outs[j], &so[j]) == 0;
      for (uint32_t i = 0; have[j] && i < n_in; ++i) {
        struct stat si;
        if (fstat(ins[i]->fd, &si) == 0 && si.st_dev == so[j].st_dev && si.st_ino == so[j].st_ino)
          return mfx_fail(MFX_E_INVAL, "mfx_db_trio: the output '%s' is the input '%s'", outs[j], paths[i]);
      }
    }
    if (strcmp(out_a, out_b) == 0 || (have[0] && have[1] && so[0].st_dev == so[1].st_dev && so[0].st_ino == so[1].st_ino))
      return mfx_fail(MFX_E_INVAL, "mfx_db_trio: the two outputs '%s' and '%s' are the same file", out_a, out_b);
  }
  MergeWindows P;
  if (int rc = merge_plan_windows(ins, k, who, P)) return rc;
  uint32_t cuts[3] = {o->cut_mat, o->cut_pat, has_child ? o->cut_child : 1u};
  const bool need_hist = kind != TRIO_FULL || cuts[0] == 0 || cuts[1] == 0 || cuts[2] == 0;
  const uint64_t W = (uint64_t)o->max_mult + 1, cells = 3 * W;
  std::vector<uint64_t> image(cells + 1, 0);
  uint64_t dstats[MFX_TRIO_NSTATS] = {0, 0, 0, 0, 0, 0}, windows = 0;
  TrioTimes T;
  // ---- the device: the buffers of the largest window, for both passes
  std::unique_ptr<DeviceBack> back;
  DbDev D;
  StreamDev SA, SB;
  MergeDecoder dec;
  mfx_db_writer *wa = nullptr, *wb = nullptr;
  WriterAbort ga, gb;
  const uint64_t cap = P.max_pairs + MFX_DELTA_BLOCK, tiles = mfx_trio_tiles(P.max_pairs);
  uint64_t *bk[2] = {nullptr, nullptr}, *xk = nullptr, *d_tile = nullptr, *d_stats = nullptr, *d_img = nullptr;
  uint32_t *bv[2] = {nullptr, nullptr}, *xv = nullptr;
  int grid = 1;
  mfx_spectrum_args sa{};
  if (P.max_pairs) {
    back.reset(new DeviceBack);
    MFX_HIP(hipSetDevice(o->device));
    // p[0], p[1]: two buffers of cap pairs, the k-mers in front of the counts: decoded runs, merge levels, set A behind its writer's carry, and
    // the packed words of the one that is free by then (p[1] only where something is merged or written).  p[2]: the window's blocks.  p[3]: the
    // classify's tile offsets (two per tile), the copies of the stats, tasks, their below / above, the inputs' error words.  p[4], p[5]: the window's escapes.
    // p[6]: set B behind its writer's carry.  p[7]: the image and its counter word.
    const uint64_t small = 2 * (tiles + 1) * 8 + MFX_TRIO_STAT_WORDS * 8 + P.max_tasks * (sizeof(mfx_merge_task) + 8) + n_in * 4 + 64;
    const bool two = kind == TRIO_FULL || n_in > 1;
    hipError_t e = hipMalloc(&D.p[0], cap * 12);
    if (e == hipSuccess && two) e = hipMalloc(&D.p[1], cap * 12);
    if (e == hipSuccess) e = hipMalloc(&D.p[2], P.max_bytes + 8);
    if (e == hipSuccess) e = hipMalloc(&D.p[3], small);
    if (e == hipSuccess) e = hipMalloc(&D.p[4], (P.max_esc + 1) * 8);
    if (e == hipSuccess) e = hipMalloc(&D.p[5], (P.max_esc + 1) * 4);
    if (e == hipSuccess && kind == TRIO_FULL) e = hipMalloc(&D.p[6], cap * 12);
    if (e == hipSuccess && need_hist) e = hipMalloc(&D.p[7], (cells + 1) * 8);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      const double nbuf = kind == TRIO_FULL ? 3 : two ? 2 : 1;
      // (a writer's own: the plan and offsets of its blocks, 28 bytes per 4096 k-mers, and what a window escapes)
      return mfx_fail(MFX_E_NOMEM, "%s: the buffers of a window of %lu pairs (%.3f GB: %d of %lu pairs, the second output's among them; the blocks; the block plans "
                      "of both writers) do not fit the device: %s; lower MFX_MERGE_RANGE", who, (unsigned long)P.max_pairs,
                      (nbuf * (double)cap * 12 + (double)P.max_bytes + (double)P.max_esc * 12 + (double)small + (double)(cells + 1) * 8 +
                       (kind == TRIO_FULL ? 2.0 * (double)(cap / MFX_DELTA_BLOCK + 1) * (sizeof(mfx_delta_plan) + 12) : 0.0)) / 1e9,
                      (int)nbuf, (unsigned long)cap, hipGetErrorString(e));
    }
    for (int i = 0; i < 2; ++i) { bk[i] = (uint64_t *)D.p[i]; bv[i] = D.p[i] ? (uint32_t *)((char *)D.p[i] + cap * 8) : nullptr; }
    xk = (uint64_t *)D.p[6]; xv = D.p[6] ? (uint32_t *)((char *)D.p[6] + cap * 8) : nullptr;
    d_tile = (uint64_t *)D.p[3]; d_stats = d_tile + 2 * (tiles + 1); d_img = (uint64_t *)D.p[7];
    dec.d_tasks = (mfx_merge_task *)(d_stats + MFX_TRIO_STAT_WORDS);
    dec.d_below = (uint32_t *)(dec.d_tasks + P.max_tasks); dec.d_above = dec.d_below + P.max_tasks; dec.d_err = dec.d_above + P.max_tasks;
    dec.d_words = D.p[2]; dec.d_ek = (uint64_t *)D.p[4]; dec.d_ev = (uint32_t *)D.p[5];
    MFX_HIP(hipHostMalloc(&dec.pinned, P.max_bytes + 8, hipHostMallocDefault));
    MFX_HIP(mfx_memset_now(d_stats, 0, MFX_TRIO_STAT_WORDS * 8));
    if (d_img) MFX_HIP(mfx_memset_now(d_img, 0, (cells + 1) * 8));
    int cus = 0;
    MFX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, o->device));
    grid = (cus > 0 ? cus : 256) * 4;                            // 32 KB of LDS bins per workgroup: four workgroups of four waves per CU
    sa.copies = 1;                                               // an image of copies + 2 = 3 rows
    sa.max_mult = o->max_mult;
    sa.lds_cols = mfx_spec_lds_cols(1, o->max_mult);
    const char *ag = getenv("MFX_SPECTRUM_AGG");                 // as mfx_spectrum_run reads it (docs/KNOBS.md)
    sa.aggregate = ag ? (atoi(ag) != 0) : MFX_SPEC_AGG_DEFAULT;
    sa.img = d_img;
  }
  const bool timing = getenv("MFX_DB_TIMING") != nullptr;
  // one pass over the windows: decode, tag, merge, then the histogram (classify == false) or the two sets behind their writers
  auto run_pass = [&](bool classify) -> int {
    std::vector<MergeRun> &runs = dec.runs, next;
    std::vector<uint64_t> got(n_in, 0);
    const mfx_trio_cuts tc{cuts[0], cuts[1], cuts[2], has_child};
    windows = 0;
    for (size_t wi = 0; wi < P.win.size(); ++wi) {
      if (P.win[wi].pairs == 0) continue;
      const int rc_dec = merge_decode_window(ins, P, wi, k, who, dec, bk[0], bv[0]);
      T.read += dec.t_read; T.decode += dec.t_decode;
      if (rc_dec) return rc_dec;
      double t0 = db_now(), t1;
      for (uint32_t i = 0; i < n_in; ++i) {                      // the role into the key's two low bits (mfx_trio.h)
        got[i] += runs[i].len;
        MFX_HIP(mfx_k_trio_tag(bk[0] + runs[i].off, runs[i].len, roles[i], nullptr));
      }
      int cur = 0;
      while (runs.size() > 1) {                                  // mfx_db_merge's pairwise tree, from one buffer to the other
        next.clear();
        uint64_t at = 0;
        for (size_t j = 0; j < runs.size(); j += 2) {
          const MergeRun a = runs[j], b = j + 1 < runs.size() ? runs[j + 1] : MergeRun{0, 0};
          MFX_HIP(mfx_k_merge_pairs(bk[cur] + a.off, bv[cur] + a.off, a.len, bk[cur] + b.off, bv[cur] + b.off, b.len, bk[cur ^ 1] + at, bv[cur ^ 1] + at, nullptr));
          next.push_back(MergeRun{at, a.len + b.len});
          at += a.len + b.len;
        }
        runs.swap(next);
        cur ^= 1;
      }
      if (timing) MFX_HIP(hipStreamSynchronize(nullptr));
      t1 = db_now();
      T.merge += t1 - t0;
      const uint64_t M = runs[0].len;
      ++windows;
      if (!classify) {
        MFX_HIP(mfx_k_trio_hist(bk[cur] + runs[0].off, bv[cur] + runs[0].off, M, sa, grid, nullptr));
        if (timing) MFX_HIP(hipStreamSynchronize(nullptr));
        T.hist += db_now() - t1;
        continue;
      }
      // ---- classify: set A behind the place of its writer's carry in the other buffer, set B behind its writer's in a buffer of its own
      const uint64_t ca = wa->ck.size(), cb = wb->ck.size();
      uint64_t n_out[2] = {0, 0};
      if (M) {
        const uint64_t mt = mfx_trio_tiles(M);
        MFX_HIP(mfx_k_trio_classify(bk[cur] + runs[0].off, bv[cur] + runs[0].off, M, tc, d_tile, bk[cur ^ 1] + ca, bv[cur ^ 1] + ca, xk + cb, xv + cb, d_stats, nullptr));
        MFX_HIP(hipMemcpyAsync(n_out, d_tile + 2 * mt, 16, hipMemcpyDeviceToHost, nullptr));
        MFX_HIP(hipStreamSynchronize(nullptr));
      }
      t0 = db_now();
      T.classify += t0 - t1;
      if (n_out[0] + n_out[1] > M) return mfx_fail(MFX_E_HIP, "%s: the classified pairs of a window are damaged", who);
      // (the merged run is read by now: its buffer is the scratch of both appends, one after the other -- an append has left the device when it returns)
      if (n_out[0])
        if (int rc = stream_append_device(wa, SA, bk[cur ^ 1], bv[cur ^ 1], n_out[0], bk[cur], cap * 12, who, "MFX_MERGE_RANGE")) return rc;
      if (n_out[1])
        if (int rc = stream_append_device(wb, SB, xk, xv, n_out[1], bk[cur], cap * 12, who, "MFX_MERGE_RANGE")) return rc;
      T.write += db_now() - t0;
    }
    // what the windows held against what the files say: no partial result is handed out
    for (uint32_t i = 0; i < n_in; ++i)
      if (got[i] != ins[i]->h.n)
        return mfx_fail(MFX_E_FORMAT, "'%s': the windows hold %lu of its %lu k-mers: the directory does not describe the blocks", paths[i], (unsigned long)got[i],
                        (unsigned long)ins[i]->h.n);
    return MFX_OK;
  };
  const uint64_t n_of[3] = {kind != TRIO_HISTOGRAM ? ins[0]->h.n : 0, kind != TRIO_HISTOGRAM ? ins[1]->h.n : 0, has_child ? ins[n_in - 1]->h.n : 0};
  // ---- pass 1: the image
  if (need_hist) {
    if (P.max_pairs) {
      if (int rc = run_pass(false)) return rc;
      MFX_HIP(hipMemcpy(image.data(), d_img, (cells + 1) * 8, hipMemcpyDeviceToHost));
    }
    uint64_t sum = 0, row[3] = {0, 0, 0};
    for (size_t i = 0; i < cells; ++i) { sum += image[i]; row[i / W] += image[i]; }
    if (sum != image[cells]) return mfx_fail(MFX_E_HIP, "%s: the image sums to %lu, the pass counted %lu entries", who, (unsigned long)sum, (unsigned long)image[cells]);
    if (row[2] != n_of[2] || row[0] > n_of[0] || row[1] > n_of[1] || n_of[0] - row[0] != n_of[1] - row[1])
      return mfx_fail(MFX_E_HIP, "%s: the rows of the image hold %lu, %lu and %lu k-mers: not what databases of %lu, %lu and %lu k-mers give", who, (unsigned long)row[0],
                      (unsigned long)row[1], (unsigned long)row[2], (unsigned long)n_of[0], (unsigned long)n_of[1], (unsigned long)n_of[2]);
    dstats[MFX_TRIO_S_MAT_ONLY] = row[0]; dstats[MFX_TRIO_S_PAT_ONLY] = row[1]; dstats[MFX_TRIO_S_BOTH] = n_of[0] - row[0];
  }
  uint32_t autos[3] = {0, 0, 0};
  uint64_t n_a = 0, n_b = 0;
  double t_close = 0;
  if (kind == TRIO_FULL) {
    // ---- the automatic cutoffs: the valley of each row, by the rule -peak auto reads its peak with
    static const char *const what[3] = {"cut_mat (merfin -cutmat <n>)", "cut_pat (merfin -cutpat <n>)", "cut_child (merfin -cutchild <n>)"};
    for (uint32_t r = 0; r < 3; ++r) {
      if (cuts[r] != 0) continue;
      mfx_spectrum_peak_t pk;
      const int rc = mfx_spectrum_peak(image.data() + r * W, o->max_mult, &pk);
      if (rc == MFX_E_NODATA) {
        const std::string why = mfx_last_error();
        return mfx_fail(MFX_E_NODATA, "mfx_db_trio: no automatic cutoff for '%s': the histogram of %s shows no valley (%s); give %s", paths[r],
                        r == 2 ? "its k-mers" : "the k-mers the other parent does not hold", why.c_str(), what[r]);
      }
      if (rc) return rc;
      cuts[r] = pk.valley;
      autos[r] = 1;
    }
    // ---- pass 2: the two sets
    if (int rc = db_open_streamed(out_a, k, &wa)) return rc;
    ga.w = wa;
    if (int rc = db_open_streamed(out_b, k, &wb)) return rc;
    gb.w = wb;
    if (P.max_pairs) {
      if (int rc = stream_dev_init(SA, wa, cap, who, "MFX_MERGE_RANGE")) return rc;
      if (int rc = stream_dev_init(SB, wb, cap, who, "MFX_MERGE_RANGE")) return rc;
      if (int rc = run_pass(true)) return rc;
      std::vector<uint64_t> shards(MFX_TRIO_STAT_WORDS);      // the counters' copies, added up
      MFX_HIP(hipMemcpy(shards.data(), d_stats, MFX_TRIO_STAT_WORDS * 8, hipMemcpyDeviceToHost));
      for (uint32_t s = 0; s < (uint32_t)MFX_TRIO_NSTATS; ++s) {
        dstats[s] = 0;
        for (uint32_t c = 0; c < MFX_TRIO_STAT_SHARDS; ++c) dstats[s] += shards[c * MFX_TRIO_STAT_STRIDE + s];
      }
      if (dstats[MFX_TRIO_S_BOTH] + dstats[MFX_TRIO_S_MAT_ONLY] != n_of[0] || dstats[MFX_TRIO_S_BOTH] + dstats[MFX_TRIO_S_PAT_ONLY] != n_of[1])
        return mfx_fail(MFX_E_HIP, "mfx_db_trio: %lu k-mers of both parents, %lu and %lu of one alone: not what databases of %lu and %lu k-mers give",
                        (unsigned long)dstats[MFX_TRIO_S_BOTH], (unsigned long)dstats[MFX_TRIO_S_MAT_ONLY], (unsigned long)dstats[MFX_TRIO_S_PAT_ONLY],
                        (unsigned long)n_of[0], (unsigned long)n_of[1]);
    }
    const double tc0 = db_now();
    ga.w = nullptr;
    if (int rc = mfx_db_writer_close(wa, &n_a)) return rc;       // (gb: the second writer goes with its spool)
    gb.w = nullptr;
    if (int rc = mfx_db_writer_close(wb, &n_b)) { unlink(out_a); return rc; }
    t_close = db_now() - tc0;
    if (img && need_hist) memcpy(img, image.data(), cells * 8);
  } else if (kind == TRIO_HIST) {
    memcpy(img, image.data(), cells * 8);
  } else {
    memcpy(img, image.data() + MFX_TRIO_CHILD * W, W * 8);       // (one row: the file stood in the child's role)
  }
  if (st) {
    st->n_mat = n_of[0]; st->n_pat = n_of[1]; st->n_child = n_of[2];
    st->n_both = dstats[MFX_TRIO_S_BOTH]; st->n_mat_only = dstats[MFX_TRIO_S_MAT_ONLY]; st->n_pat_only = dstats[MFX_TRIO_S_PAT_ONLY];
    st->n_mat_only_cut = dstats[MFX_TRIO_S_MAT_CUT]; st->n_pat_only_cut = dstats[MFX_TRIO_S_PAT_CUT]; st->n_child_cut = dstats[MFX_TRIO_S_CHILD_CUT];
    st->n_a = n_a; st->n_b = n_b; st->windows = windows;
    if (kind == TRIO_FULL) {
      st->cut_mat = cuts[0]; st->cut_pat = cuts[1]; st->cut_child = has_child ? cuts[2] : 0;
      st->auto_mat = autos[0]; st->auto_pat = autos[1]; st->auto_child = has_child ? autos[2] : 0;
    }
    st->hist_pass = need_hist ? 1u : 0u;
    st->t_read = T.read; st->t_decode = T.decode; st->t_merge = T.merge; st->t_hist = T.hist; st->t_classify = T.classify; st->t_write = T.write;
    st->t_close = t_close; st->t_total = db_now() - t_begin;
  }
  return MFX_OK;
}

extern "C" int mfx_db_trio(const char *mat_path, const char *pat_path, const char *child_path, const char *out_a, const char *out_b, const mfx_db_trio_opts *o, uint64_t *img,
                           mfx_db_trio_stats *st) {
  try { return trio_impl(TRIO_FULL, mat_path, pat_path, child_path, out_a, out_b, o, img, st); }      // (nothing leaves the C ABI as an exception)
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_trio: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_trio: %s", e.what()); }
}

extern "C" int mfx_db_trio_hist(const char *mat_path, const char *pat_path, const char *child_path, uint32_t max_mult, uint64_t *img, mfx_db_trio_stats *st, int device) {
  const mfx_db_trio_opts o{0, 0, 0, max_mult, device};
  try { return trio_impl(TRIO_HIST, mat_path, pat_path, child_path, nullptr, nullptr, &o, img, st); }
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_trio_hist: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_trio_hist: %s", e.what()); }
}

extern "C" int mfx_db_histogram(const char *path, uint32_t max_mult, uint64_t *row, uint64_t *n_kmers, int device) {
  const mfx_db_trio_opts o{0, 0, 0, max_mult, device};
  mfx_db_trio_stats st;
  if (n_kmers) *n_kmers = 0;
  try {
    if (int rc = trio_impl(TRIO_HISTOGRAM, nullptr, nullptr, path, nullptr, nullptr, &o, row, &st)) return rc;
    if (n_kmers) *n_kmers = st.n_child;
    return MFX_OK;
  }
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_histogram: out of memory"); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "mfx_db_histogram: %s", e.what()); }
}

extern "C" int mfx_db_histogram_write(const uint64_t *row, uint32_t max_mult, const char *path) {
  if (!row || !path) return mfx_fail(MFX_E_INVAL, "mfx_db_histogram_write: null argument");
  if (max_mult < MFX_SPEC_MIN_MULT || max_mult > MFX_SPEC_MAX_MULT)
    return mfx_fail(MFX_E_INVAL, "mfx_db_histogram_write: max_mult = %u is outside [%u, %u]", max_mult, MFX_SPEC_MIN_MULT, MFX_SPEC_MAX_MULT);
  mfx_file fh = mfx_open_writer(path, false);                    // compressor chosen by suffix (mfx_pipe.h)
  if (!fh.f) return mfx_fail(MFX_E_IO, "mfx_db_histogram_write: cannot open '%s' for writing", path);
  for (uint32_t m = 0; m <= max_mult; ++m)
    if (row[m]) fprintf(fh.f, "%u\t%llu\n", m, (unsigned long long)row[m]);
  if (mfx_close(fh)) return mfx_fail(MFX_E_IO, "mfx_db_histogram_write: writing '%s' failed", path);
  return MFX_OK;
}

extern "C" int mfx_db_trio_host(const uint64_t *mat_keys, const uint32_t *mat_vals, uint64_t n_mat, const uint64_t *pat_keys, const uint32_t *pat_vals, uint64_t n_pat,
                                const uint64_t *child_keys, const uint32_t *child_vals, uint64_t n_child, int has_child, uint32_t cut_mat, uint32_t cut_pat,
                                uint32_t cut_child, uint32_t max_mult, uint64_t *a_keys, uint32_t *a_vals, uint64_t *n_a, uint64_t *b_keys, uint32_t *b_vals, uint64_t *n_b,
                                uint64_t *img, mfx_db_trio_stats *st) {
  if ((n_mat && (!mat_keys || !mat_vals || !a_keys || !a_vals)) || (n_pat && (!pat_keys || !pat_vals || !b_keys || !b_vals)) || (n_child && (!child_keys || !child_vals)) ||
      !n_a || !n_b || !img || !st)
    return mfx_fail(MFX_E_INVAL, "mfx_db_trio_host: null argument");
  if (max_mult < MFX_SPEC_MIN_MULT || max_mult > MFX_SPEC_MAX_MULT)
    return mfx_fail(MFX_E_INVAL, "mfx_db_trio_host: max_mult = %u is outside [%u, %u]", max_mult, MFX_SPEC_MIN_MULT, MFX_SPEC_MAX_MULT);
  if (cut_mat == 0 || cut_pat == 0 || (has_child && cut_child == 0) || (!has_child && n_child))
    return mfx_fail(MFX_E_INVAL, "mfx_db_trio_host: the cutoffs are 1 at the least, and there are no child k-mers without a child");
  try {
    const uint64_t *const keys[3] = {mat_keys, pat_keys, child_keys};
    const uint32_t *const vals[3] = {mat_vals, pat_vals, child_vals};
    const uint64_t n[3] = {n_mat, n_pat, n_child};
    mfx_trio_host_result R;
    mfx_trio_host(keys, vals, n, mfx_trio_cuts{cut_mat, cut_pat, has_child ? cut_child : 1u, has_child != 0}, max_mult, R);
    if (R.ak.size() > n_mat || R.bk.size() > n_pat) return mfx_fail(MFX_E_INVAL, "mfx_db_trio_host: the runs do not ascend strictly");
    if (!R.ak.empty()) { memcpy(a_keys, R.ak.data(), R.ak.size() * 8); memcpy(a_vals, R.av.data(), R.av.size() * 4); }
    if (!R.bk.empty()) { memcpy(b_keys, R.bk.data(), R.bk.size() * 8); memcpy(b_vals, R.bv.data(), R.bv.size() * 4); }
    memcpy(img, R.img.data(), R.img.size() * 8);
    memset(st, 0, sizeof(*st));
    st->n_mat = n_mat; st->n_pat = n_pat; st->n_child = n_child;
    st->n_both = R.stats[MFX_TRIO_S_BOTH]; st->n_mat_only = R.stats[MFX_TRIO_S_MAT_ONLY]; st->n_pat_only = R.stats[MFX_TRIO_S_PAT_ONLY];
    st->n_mat_only_cut = R.stats[MFX_TRIO_S_MAT_CUT]; st->n_pat_only_cut = R.stats[MFX_TRIO_S_PAT_CUT]; st->n_child_cut = R.stats[MFX_TRIO_S_CHILD_CUT];
    st->n_a = *n_a = R.ak.size(); st->n_b = *n_b = R.bk.size();
    st->cut_mat = cut_mat; st->cut_pat = cut_pat; st->cut_child = has_child ? cut_child : 0;
    return MFX_OK;
  } catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "mfx_db_trio_host: out of memory"); }
}


// ---------------------------------------------------------------------------
// Device-format index image: the built table written to / read from disk as is,
// so that repeated runs (-hist, then -dump, then -polish on the same databases)
// skip the decode + insert of the k-mer databases.  Layout: IndexImageHeader,
// then the table lines (128 bytes each) in order.
// ---------------------------------------------------------------------------
struct IndexImageHeader {
  char     magic[8];         // "MFXINDX2"
  uint32_t k, mz_w;
  uint32_t shard_rank, shard_n;
  uint64_t nlines, capacity_kmers;
  uint64_t minV, maxV;
  uint64_t meta[4];          // distinct, non-canonical inserts, probe failures, reserved
  uint32_t slot_bytes, line_slots;
  uint32_t filter_set, layout;   // layout = MFX_LAYOUT_VERSION of the build that wrote the image
  uint64_t fingerprint;          // caller's digest of the inputs the table was built from (mfx_index_set_fingerprint)
  uint64_t side_nlines;          // compact layout: lines of the side table that follow the nlines main lines
  uint32_t flags, seq_digest;    // bit 0: sequence-only index, bit 1: compact layout, bit 2: frozen (counts were added), bit 3: quotient key fields; digest of the claimed sequence (0: none)
};

static_assert(sizeof(IndexImageHeader) <= MFX_INDEX_HEADER_BYTES, "index image header outgrew its public size");

static int fill_header(const mfx_index *ix, IndexImageHeader &h) {
  if (hipSetDevice(ix->device) != hipSuccess) return mfx_fail(MFX_E_HIP, "hipSetDevice(%d) failed", ix->device);
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, "MFXINDX2", 8);
  h.k = (uint32_t)ix->k; h.mz_w = (uint32_t)ix->mz_w | ((uint32_t)ix->mz_t << 8);   // (the sampling t-mer length rides in the second byte)
  h.shard_rank = ix->shard_rank; h.shard_n = ix->shard_n;
  h.nlines = ix->nlines; h.capacity_kmers = ix->capacity_kmers;
  h.minV = ix->minV; h.maxV = ix->maxV;
  h.slot_bytes = MFX_ALIGN / ix->slots_per_line(); h.line_slots = ix->slots_per_line();
  h.filter_set = ix->filter_set ? 1u : 0u;
  h.layout = MFX_LAYOUT_VERSION;
  h.fingerprint = ix->fingerprint;
  h.side_nlines = ix->side_nlines;
  h.flags = (ix->seq_only ? 1u : 0u) | (ix->compact ? 2u : 0u) | (ix->frozen ? 4u : 0u) | (ix->quot ? 8u : 0u);
  h.seq_digest = ix->seq_digest;
  if (hipMemcpy(h.meta, ix->d_meta, sizeof(h.meta), hipMemcpyDeviceToHost) != hipSuccess) return mfx_fail(MFX_E_HIP, "reading index metadata failed");
  return MFX_OK;
}

static bool header_ok(const IndexImageHeader &h) {
  const bool wide = h.k > (uint32_t)MFX_MAX_K_NARROW, compact = (h.flags & 2u) != 0;
  if (compact && (!(h.flags & 1u) || wide || h.k > (uint32_t)MFX_MAX_K_COMPACT || h.side_nlines == 0)) return false;
  if (((h.flags & 8u) != 0) != (compact && h.k > (uint32_t)MFX_MAX_K_DIRECT)) return false;      // the quotient form is the compact layout of k > 21
  if ((h.flags & 8u) && h.nlines < (1ull << (2 * ((int)h.k - 3) - 31))) return false;
  if (!compact && h.side_nlines != 0) return false;
  const uint32_t line_slots = wide ? MFX_WSLOTS_LINE : compact ? MFX_CSLOTS_LINE : MFX_SLOTS_LINE;
  return memcmp(h.magic, "MFXINDX2", 8) == 0 && h.slot_bytes == MFX_ALIGN / line_slots && h.line_slots == line_slots && h.k >= 1 &&
         h.k <= (uint32_t)MFX_MAX_K && h.nlines != 0 && h.nlines < (1ull << 32) && h.side_nlines < (1ull << 32) && h.layout == MFX_LAYOUT_VERSION;
}

// an index of exactly the header's geometry; its lines are allocated but hold nothing yet
static mfx_index *index_from_header(const IndexImageHeader &h, double max_gb, int device) {
  mfx_index *ix = mfx_index_create((int)h.k, 1, 0.0, device);
  if (!ix) return nullptr;
  const uint64_t total_lines = h.nlines + h.side_nlines;
  if (max_gb > 0 && (double)total_lines * MFX_ALIGN / 1e9 > max_gb) {
    mfx_fail(MFX_E_NOMEM, "Not enough memory to load databases.  Increase -memory. (need %.3f GB, limit %.3f GB)", (double)total_lines * MFX_ALIGN / 1e9, max_gb);
    mfx_index_free(ix);
    return nullptr;
  }
  (void)hipSetDevice(device);
  (void)hipFree(ix->d_slots);
  ix->d_slots = nullptr;
  ix->nlines = h.nlines;
  ix->capacity_kmers = h.capacity_kmers;
  ix->mz_w = (int)(h.mz_w & 0xffu);
  ix->mz_t = (int)((h.mz_w >> 8) & 0xffu);
  ix->shard_rank = h.shard_rank; ix->shard_n = h.shard_n ? h.shard_n : 1;
  ix->minV = h.minV; ix->maxV = h.maxV; ix->filter_set = h.filter_set != 0;
  ix->fingerprint = h.fingerprint;
  ix->side_nlines = h.side_nlines;
  ix->seq_only = (h.flags & 1u) != 0; ix->compact = (h.flags & 2u) != 0; ix->frozen = (h.flags & 4u) != 0; ix->quot = (h.flags & 8u) != 0;
  ix->seq_digest = ix->seq_only ? h.seq_digest : 0u;
  if (hipMalloc((void **)&ix->d_slots, total_lines * MFX_ALIGN) != hipSuccess ||
      hipMemcpy(ix->d_meta, h.meta, sizeof(h.meta), hipMemcpyHostToDevice) != hipSuccess) {
    mfx_fail(MFX_E_NOMEM, "cannot allocate %.3f GB for the index image on device %d", (double)total_lines * MFX_ALIGN / 1e9, device);
    mfx_index_free(ix);
    return nullptr;
  }
  return ix;
}

extern "C" int mfx_index_image_header(const mfx_index *ix, void *hdr) {
  if (!ix || !hdr) return mfx_fail(MFX_E_INVAL, "mfx_index_image_header: null argument");
  IndexImageHeader h;
  int rc = fill_header(ix, h);
  if (rc) return rc;
  memset(hdr, 0, MFX_INDEX_HEADER_BYTES);
  memcpy(hdr, &h, sizeof(h));
  return MFX_OK;
}

extern "C" mfx_index *mfx_index_create_from_header(const void *hdr, double max_gb, int device) {
  if (!hdr) { mfx_fail(MFX_E_INVAL, "mfx_index_create_from_header: null argument"); return nullptr; }
  IndexImageHeader h;
  memcpy(&h, hdr, sizeof(h));
  if (!header_ok(h)) { mfx_fail(MFX_E_FORMAT, "not an index image header of this build"); return nullptr; }
  return index_from_header(h, max_gb, device);
}

extern "C" int mfx_index_device_image(mfx_index *ix, void **d_lines, uint64_t *line_bytes, void **d_meta, uint64_t *meta_bytes) {
  if (!ix || !d_lines || !line_bytes || !d_meta || !meta_bytes) return mfx_fail(MFX_E_INVAL, "mfx_index_device_image: null argument");
  *d_lines = ix->d_slots;
  *line_bytes = ix->total_lines() * MFX_ALIGN;
  *d_meta = ix->d_meta;
  *meta_bytes = 4 * sizeof(uint64_t);
  return MFX_OK;
}

extern "C" int mfx_index_commit(mfx_index *ix) {
  if (!ix) return mfx_fail(MFX_E_INVAL, "mfx_index_commit: null argument");
  ix->version++;                       // cached per-index facts (canonical or not) are re-read from the new contents
  return MFX_OK;
}

extern "C" int mfx_index_set_fingerprint(mfx_index *ix, uint64_t fingerprint) {
  if (!ix) return mfx_fail(MFX_E_INVAL, "mfx_index_set_fingerprint: null index");
  ix->fingerprint = fingerprint;
  return MFX_OK;
}

extern "C" int mfx_index_get_origin(const mfx_index *ix, uint64_t *fingerprint, uint64_t *minV, uint64_t *maxV) {
  if (!ix) return mfx_fail(MFX_E_INVAL, "mfx_index_get_origin: null index");
  if (fingerprint) *fingerprint = ix->fingerprint;
  if (minV) *minV = ix->filter_set ? ix->minV : 0;
  if (maxV) *maxV = ix->filter_set ? ix->maxV : ~0ull;
  return MFX_OK;
}

extern "C" int mfx_index_save(const mfx_index *ix, const char *path) {
  if (!ix || !path) return mfx_fail(MFX_E_INVAL, "mfx_index_save: null argument");
  IndexImageHeader h;
  int rc = fill_header(ix, h);
  if (rc) return rc;
  FILE *f = fopen(path, "wb");
  if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", path);
  if (fwrite(&h, sizeof(h), 1, f) != 1) rc = mfx_fail(MFX_E_IO, "short write to '%s'", path);
  const size_t CH = 256ull << 20;
  std::vector<char> buf(rc == MFX_OK ? CH : 1);
  const uint64_t total = ix->total_lines() * MFX_ALIGN;
  for (uint64_t o = 0; o < total && rc == MFX_OK; o += CH) {
    size_t m = (size_t)std::min<uint64_t>(CH, total - o);
    if (hipMemcpy(buf.data(), (const char *)ix->d_slots + o, m, hipMemcpyDeviceToHost) != hipSuccess) rc = mfx_fail(MFX_E_HIP, "D2H copy of the table failed");
    else if (fwrite(buf.data(), 1, m, f) != m) rc = mfx_fail(MFX_E_IO, "short write to '%s'", path);
  }
  fclose(f);
  return rc;
}

extern "C" mfx_index *mfx_index_load(const char *path, double max_gb, int device) {
  if (!path) { mfx_fail(MFX_E_INVAL, "mfx_index_load: null argument"); return nullptr; }
  FILE *f = fopen(path, "rb");
  if (!f) { mfx_fail(MFX_E_IO, "cannot open '%s'", path); return nullptr; }
  IndexImageHeader h;
  if (fread(&h, sizeof(h), 1, f) != 1 || !header_ok(h)) {
    fclose(f);
    mfx_fail(MFX_E_FORMAT, "'%s' is not an index image of this build", path);
    return nullptr;
  }
  mfx_index *ix = index_from_header(h, max_gb, device);
  if (!ix) { fclose(f); return nullptr; }
  bool ok = true;
  const size_t CH = 256ull << 20;
  std::vector<char> buf(ok ? CH : 1);
  const uint64_t total = (h.nlines + h.side_nlines) * MFX_ALIGN;
  for (uint64_t o = 0; o < total && ok; o += CH) {
    size_t m = (size_t)std::min<uint64_t>(CH, total - o);
    ok = fread(buf.data(), 1, m, f) == m && hipMemcpy((char *)ix->d_slots + o, buf.data(), m, hipMemcpyHostToDevice) == hipSuccess;
  }
  fclose(f);
  if (!ok) {
    mfx_fail(MFX_E_IO, "'%s': truncated image or device copy failed", path);
    mfx_index_free(ix);
    return nullptr;
  }
  ix->version++;
  return ix;
}
