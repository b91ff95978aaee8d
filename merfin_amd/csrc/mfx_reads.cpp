// mfx_reads.cpp -- the read k-mer counter (include/merfin_amd.h: mfx_reads_*): the read counts of a run straight from its
// reads, counted on the device into the k-mers the index already holds (mfx_kernels.hip: mfx_reads_kernel).
//
// Host side.  Records are copied back to back into a byte batch, one 'N' between two of them (no k-mer spans two reads);
// a record longer than the room left is cut, and its rest starts the next batch k-1 bases before the cut, so every k-mer
// is in exactly one batch.  A full batch is packed into 2-bit codes + validity bits (mfx_pack_bases) in one of two pinned
// stages, copied and counted on that stage's stream: the caller parses the next records while the device counts.
//
// The CLAIMING counter (mfx_reads_begin_all; a full table of 16-byte slots) claims every k-mer it meets, in a table that GROWS: nobody
// knows the reads' distinct k-mers beforehand.  No launch may overfill the table, so before a batch is enqueued the bound of mfx_grow.h
// is checked against the table's distinct count as last read and the positions enqueued since; when it fails the stages are settled and
// the count is read again, and when it still fails every entry moves into a larger table (mfx_table_rehash_kernel).
//
// The RANGED claiming counter (mfx_reads_begin_range) is the claiming counter for the k-mers of one key range: one pass of a count whose
// table does not fit the device.  The READ STORE (mfx_reads_store_*) keeps the packed batches of a read set on the host and mfx_reads_replay
// sends them through any counter, so that the passes after the first parse nothing; store and counter cut records into batches with the
// same code (batch_records, batch_pack).
#include "mfx_internal.h"
#include "mfx_kernels.h"
#include "mfx_grow.h"
#include "mfx_bin.h"

#include <chrono>

#include <string.h>

#include <algorithm>
#include <vector>

extern "C" void mfx_pack_bases(const uint8_t *src, uint64_t n, uint64_t *codes, uint32_t *valid);      // mfx_pack.cpp

namespace {
constexpr uint64_t MFX_READS_BATCH_DEFAULT = MFX_BATCH_BASES_DEFAULT;
constexpr int MFX_READS_STAGES = 2;
constexpr uint64_t MFX_TILE_WORDS_HOST = (MFX_TILE + 64) / 32;        // words a tile reads (mfx_device.h: MFX_TILE_WORDS)

struct DeviceScope {
  int prev = -1;
  bool ok = false;
  explicit DeviceScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// ---- records into batches: what mfx_reads_add and mfx_reads_store_add share ----------------------------------------------------
// The bytes of the batch being filled.  batch_records copies records in, one 'N' between two; a record longer than the room left is cut and
// its rest starts the next batch k-1 bases before the cut.  Whenever a batch is complete `flush` is called (it sends or keeps b.bytes[0, b.used)
// and sets b.used = 0; non-zero: its error, passed on).  batch_pack turns such a batch into the planes a launch reads.
typedef mfx_batch Batch;             // (csrc/mfx_bin.h: the cut is shared with -bin, which also asks for the pieces)

// planes of npos bases in nw words each (nw >= (npos + 31) / 32): the words beyond the bases are invalid (the halo of the last tile)
void batch_pack(const uint8_t *bytes, uint64_t npos, uint64_t nw, uint64_t *codes, uint32_t *valid) {
  const uint64_t packed = (npos + 31) / 32;
  mfx_pack_bases(bytes, npos, codes, valid);
  if (nw > packed) {
    memset(codes + packed, 0, (nw - packed) * sizeof(uint64_t));
    memset(valid + packed, 0, (nw - packed) * sizeof(uint32_t));
  }
}

template <class Flush>
int batch_records(Batch &b, uint64_t k, const char *const *bases, const uint64_t *lens, uint64_t n, uint64_t &n_reads, uint64_t &n_bases, const char *who,
                  Flush &&flush) {
  return mfx_batch_records(b, k, bases, lens, n, n_reads, n_bases,
                           [&](uint64_t i) { return mfx_fail(MFX_E_INVAL, "%s: record %llu has no bases", who, (unsigned long long)i); }, flush,
                           [](uint64_t, uint64_t, uint64_t, bool) {});
}

// the batch size both the counters and the store take; 0: refused (the text is set)
uint64_t batch_size_checked(uint64_t batch_bases, int k, const char *who) {
  const uint64_t min_batch = 2ull * (uint64_t)k + 2;
  if (batch_bases == 0) batch_bases = MFX_READS_BATCH_DEFAULT;
  if (batch_bases < min_batch) {
    mfx_fail(MFX_E_INVAL, "%s: a batch of %llu bases is too small for %d-mers (at least %llu)", who, (unsigned long long)batch_bases, k,
             (unsigned long long)min_batch);
    return 0;
  }
  if (batch_bases > (1ull << 34)) { mfx_fail(MFX_E_INVAL, "%s: batch of %llu bases is beyond 2^34", who, (unsigned long long)batch_bases); return 0; }
  return batch_bases;
}
}  // namespace

// the read store (mfx_reads_store_*): the packed batches of a read set, kept on the host so that a second pass parses nothing
struct mfx_reads_store {
  int k = 0;
  Batch b;                           // the batch being filled: the store's last batch while it holds bases
  uint64_t max_bytes = 0;            // 0: no limit
  struct Packed {
    std::vector<uint64_t> codes;     // (npos + 31) / 32 words of each plane: 3 bits per base
    std::vector<uint32_t> valid;
    uint64_t npos = 0, reads = 0, bases = 0;      // reads / bases: the records added since the batch before was complete
  };
  std::vector<Packed> batches;
  uint64_t bytes = 0;                // of the complete batches' planes
  uint64_t reads = 0, bases = 0;     // records and bases passed in
  uint64_t reads_kept = 0, bases_kept = 0;        // of those: in the statistics of a complete batch
  bool complete = true;
};

struct mfx_reads {
  mfx_index *ix = nullptr;
  Batch b;                           // the batch being filled
  uint64_t words = 0;                // plane words per stage (whole tiles + the halo)
  struct Stage {
    uint64_t *hc = nullptr, *dc = nullptr;
    uint32_t *hv = nullptr, *dv = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;    // copy starts, copy done / kernel starts, kernel done
    bool busy = false;
  } S[MFX_READS_STAGES];
  int cur = 0;
  uint64_t *d_stats = nullptr;       // [4] kmers, counted, dropped, saturated
  mfx_reads_stats stats{};
  bool failed = false;
  int  fail_code = MFX_OK;           // claiming counter: why it failed (MFX_E_NOMEM: the table could not grow)
  std::string fail_text;
  // claiming counter (mfx_reads_begin_all)
  bool claim = false;
  uint64_t distinct_known = 0;       // the table's meta[0] as last read
  uint64_t pending = 0;              // positions enqueued since that read: each may claim a k-mer
  // ranged claiming counter (mfx_reads_begin_range over less than [0, 4^k))
  bool ranged = false;
  uint64_t key_lo = 0, key_hi = 0;
};

static void reads_free(mfx_reads *r) {
  if (!r) return;
  DeviceScope g(r->ix->device);
  for (auto &s : r->S) {
    if (s.st) (void)hipStreamSynchronize(s.st);
    if (s.hc) (void)hipHostFree(s.hc);
    if (s.hv) (void)hipHostFree(s.hv);
    if (s.dc) (void)hipFree(s.dc);
    if (s.dv) (void)hipFree(s.dv);
    if (s.e0) (void)hipEventDestroy(s.e0);
    if (s.e1) (void)hipEventDestroy(s.e1);
    if (s.e2) (void)hipEventDestroy(s.e2);
    if (s.st) (void)hipStreamDestroy(s.st);
  }
  if (r->d_stats) (void)hipFree(r->d_stats);
  delete r;
}

// the stage's last batch is done: its times are added, its buffers free
static int stage_settle(mfx_reads *r, mfx_reads::Stage &s) {
  if (!s.busy) return MFX_OK;
  s.busy = false;
  MFX_HIP(hipEventSynchronize(s.e2));
  float mc = 0, mk = 0;
  MFX_HIP(hipEventElapsedTime(&mc, s.e0, s.e1));
  MFX_HIP(hipEventElapsedTime(&mk, s.e1, s.e2));
  r->stats.seconds_copy += mc * 1e-3;
  r->stats.seconds_kernel += mk * 1e-3;
  return MFX_OK;
}

// every entry of the table into one of new_lines lines; the index then holds the new table
static int table_grow(mfx_index *ix, uint64_t new_lines, uint64_t distinct) {
  const uint64_t old_bytes = ix->nlines * MFX_ALIGN;
  mfx_slot *ns = nullptr;
  uint64_t *nmeta = nullptr;
  MFX_HIP(hipMalloc((void **)&nmeta, MFX_META_WORDS * sizeof(uint64_t)));
  while (true) {
    const uint64_t new_bytes = new_lines * MFX_ALIGN;
    size_t free_b = 0, total_b = 0;
    const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    if (!known) (void)hipGetLastError();
    // the old and the new table are alive together until every entry has moved
    if ((ix->max_gb > 0 && (double)old_bytes + (double)new_bytes > ix->max_gb * 1e9) || (known && new_bytes > free_b) ||
        hipMalloc((void **)&ns, new_bytes) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(nmeta);
      return mfx_fail(MFX_E_NOMEM, "the k-mer table cannot grow from %.6f GB to %.6f GB (%lu k-mers stored): both tables are held while the entries move, "
                      "under a limit of %.6f GB (-memory; 0: none) with %.6f GB of device memory free", (double)old_bytes / 1e9, (double)new_bytes / 1e9,
                      (unsigned long)distinct, ix->max_gb, known ? (double)free_b / 1e9 : 0.0);
    }
    mfx_table_view nt = ix->view();
    nt.slots = ns;
    nt.nlines = new_lines;
    nt.qshift = 0;
    for (uint64_t x = new_lines; x > 1; x >>= 1) ++nt.qshift;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    uint64_t meta[MFX_META_WORDS] = {0};
    float ms = 0;
    const bool ok = mfx_memset_now(nmeta, 0, MFX_META_WORDS * sizeof(uint64_t)) == hipSuccess && hipEventCreate(&e0) == hipSuccess &&
                    hipEventCreate(&e1) == hipSuccess && mfx_k_table_init(ns, new_lines * MFX_SLOTS_LINE, nullptr) == hipSuccess &&
                    hipEventRecord(e0, nullptr) == hipSuccess &&
                    mfx_k_table_rehash(ix->d_slots, ix->nlines * MFX_SLOTS_LINE, nt, nmeta, nullptr) == hipSuccess &&
                    hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
                    hipEventElapsedTime(&ms, e0, e1) == hipSuccess &&
                    hipMemcpy(meta, nmeta, sizeof(meta), hipMemcpyDeviceToHost) == hipSuccess;
    const hipError_t err = ok ? hipSuccess : hipGetLastError();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (!ok) {
      (void)hipFree(ns);
      (void)hipFree(nmeta);
      return mfx_fail(MFX_E_HIP, "moving the k-mer table into a larger one failed: %s", hipGetErrorString(err));
    }
    ix->rehash_seconds += ms * 1e-3;
    ix->rehash_bytes += old_bytes + meta[0] * 2 * MFX_ALIGN;          // the old lines read, a line read and written per entry claimed
    if (meta[2] == 0 && meta[0] == distinct) break;
    (void)hipFree(ns);
    ns = nullptr;
    if (meta[2] == 0) {                                                // (never seen: the keys of a table are distinct)
      (void)hipFree(nmeta);
      return mfx_fail(MFX_E_HIP, "moving the k-mer table into a larger one lost entries: %lu of %lu arrived", (unsigned long)meta[0], (unsigned long)distinct);
    }
    // entries hit the probe limit in the larger table (one minimizer's k-mers beyond its lines): a table twice as large again
    if (new_lines > ((1ull << 32) - 16) / 2) { (void)hipFree(nmeta); return mfx_fail(MFX_E_NOMEM, "the k-mer table cannot grow beyond 2^32 lines (%.6f GB now, %.6f GB tried)", (double)old_bytes / 1e9, (double)new_bytes / 1e9); }
    new_lines *= 2;
  }
  (void)hipFree(nmeta);
  (void)hipFree(ix->d_slots);
  ix->d_slots = ns;
  ix->nlines = new_lines;
  ix->capacity_kmers = (uint64_t)((double)new_lines * MFX_SLOTS_LINE * 0.7);
  ix->version++;
  return MFX_OK;
}

// claiming counter: room for a batch of B positions, whatever they hold (mfx_grow.h)
static int claim_reserve(mfx_reads *r, uint64_t B) {
  mfx_index *ix = r->ix;
#ifdef MFX_V_GROW_NO_PENDING                                  // A/B build only: the bound without the positions in flight (tests/test_gpu_count.py must FAIL on it)
  const uint64_t pending = 0;
#else
  const uint64_t pending = r->pending;
#endif
  if (mfx_grow_fits(r->distinct_known, pending, B, ix->nlines * MFX_SLOTS_LINE)) return MFX_OK;
  for (auto &s : r->S) if (int rc = stage_settle(r, s)) return rc;
  uint64_t meta[3] = {0, 0, 0};
  MFX_HIP(hipMemcpy(meta, ix->d_meta, sizeof(meta), hipMemcpyDeviceToHost));
  r->distinct_known = meta[0];
  r->pending = 0;
  if (mfx_grow_fits(r->distinct_known, 0, B, ix->nlines * MFX_SLOTS_LINE)) return MFX_OK;
  const uint64_t nl = mfx_grow_lines(r->distinct_known, B, ix->nlines, MFX_SLOTS_LINE, (1ull << 32) - 16);
  if (nl == 0)
    return mfx_fail(MFX_E_NOMEM, "the k-mer table cannot grow from %.6f GB to one that holds %lu k-mers and a batch of %lu positions: beyond 2^32 lines "
                    "(%.6f GB)", (double)ix->nlines * MFX_ALIGN / 1e9, (unsigned long)r->distinct_known, (unsigned long)B, (double)(1ull << 32) * MFX_ALIGN / 1e9);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = table_grow(ix, nl, r->distinct_known);
  if (rc == MFX_OK) {
    ix->grow_count += 1;
    ix->grow_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  return rc;
}

// a batch of npos positions goes to the device on the next stage; fill(codes, valid, nw) writes its planes of nw words into the stage
template <class Fill>
static int reads_send(mfx_reads *r, uint64_t npos, Fill &&fill) {
  if (npos == 0) return MFX_OK;
  mfx_reads::Stage &s = r->S[r->cur];
  if (int rc = stage_settle(r, s)) return rc;
  if (r->claim) {
    if (int rc = claim_reserve(r, npos)) {
      r->fail_code = rc;
      r->fail_text = mfx_last_error();
      return rc;
    }
    r->pending += npos;
  }
  const uint64_t ntiles = (npos + MFX_TILE - 1) / MFX_TILE;
  const uint64_t nw = std::min(r->words, ntiles * (MFX_TILE / 32) + MFX_TILE_WORDS_HOST);
  fill(s.hc, s.hv, nw);
  mfx_reads_args a;
  a.t = r->ix->view();
  a.codes = s.dc;
  a.valid = s.dv;
  a.npos = npos;
  a.meta = r->ix->d_meta;
  a.stats = r->d_stats;
  a.key_lo = r->key_lo;
  a.key_hi = r->key_hi;
  MFX_HIP(hipEventRecord(s.e0, s.st));
  MFX_HIP(hipMemcpyAsync(s.dc, s.hc, nw * sizeof(uint64_t), hipMemcpyHostToDevice, s.st));
  MFX_HIP(hipMemcpyAsync(s.dv, s.hv, nw * sizeof(uint32_t), hipMemcpyHostToDevice, s.st));
  MFX_HIP(hipEventRecord(s.e1, s.st));
  MFX_HIP(r->ranged ? mfx_k_reads_claim_range(a, s.st) : r->claim ? mfx_k_reads_claim(a, s.st) : r->ix->wide() ? mfx_kw_reads(a, s.st) : mfx_k_reads(a, s.st));
  MFX_HIP(hipEventRecord(s.e2, s.st));
  s.busy = true;
  r->cur = (r->cur + 1) % MFX_READS_STAGES;
  return MFX_OK;
}

// the batch being filled goes to the device
static int reads_flush(mfx_reads *r) {
  const uint64_t npos = r->b.used;
  if (int rc = reads_send(r, npos, [&](uint64_t *hc, uint32_t *hv, uint64_t nw) { batch_pack(r->b.bytes.data(), npos, nw, hc, hv); })) return rc;
  r->b.used = 0;
  return MFX_OK;
}

// what both counters ask of the index's read side and of the batch, then the stages; `who`: the entry point, for the texts
static mfx_reads *reads_open(mfx_index *ix, uint64_t batch_bases, const char *who, bool claim) {
  if (ix->shard_n > 1) { mfx_fail(MFX_E_INVAL, "%s: a sharded index does not take read counts from reads", who); return nullptr; }
  if (ix->filter_set || ix->reads_counted) {
    mfx_fail(MFX_E_INVAL, "%s: the read side of this index already took counts (a database load or an earlier read counter); "
             "an index takes its read counts from one source", who);
    return nullptr;
  }
  batch_bases = batch_size_checked(batch_bases, ix->k, who);
  if (batch_bases == 0) return nullptr;
  DeviceScope g(ix->device);
  if (!g.ok) { mfx_fail(MFX_E_HIP, "hipSetDevice(%d) failed", ix->device); return nullptr; }
  mfx_reads *r = new mfx_reads;
  r->ix = ix;
  r->claim = claim;
  r->b.cap = batch_bases;
  r->words = (batch_bases + MFX_TILE - 1) / MFX_TILE * (MFX_TILE / 32) + MFX_TILE_WORDS_HOST;
  r->b.bytes.resize(batch_bases + 32);
  bool ok = hipMalloc((void **)&r->d_stats, 4 * sizeof(uint64_t)) == hipSuccess && mfx_memset_now(r->d_stats, 0, 4 * sizeof(uint64_t)) == hipSuccess;
  for (auto &s : r->S) {
    if (!ok) break;
    ok = hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) == hipSuccess &&
         hipHostMalloc((void **)&s.hc, r->words * sizeof(uint64_t), hipHostMallocPortable) == hipSuccess &&
         hipHostMalloc((void **)&s.hv, r->words * sizeof(uint32_t), hipHostMallocPortable) == hipSuccess &&
         hipMalloc((void **)&s.dc, r->words * sizeof(uint64_t)) == hipSuccess && hipMalloc((void **)&s.dv, r->words * sizeof(uint32_t)) == hipSuccess &&
         hipEventCreate(&s.e0) == hipSuccess && hipEventCreate(&s.e1) == hipSuccess && hipEventCreate(&s.e2) == hipSuccess;
  }
  if (!ok) {
    mfx_fail(MFX_E_NOMEM, "%s: staging of %llu bases per batch could not be allocated: %s", who, (unsigned long long)batch_bases,
             hipGetErrorString(hipGetLastError()));
    reads_free(r);
    return nullptr;
  }
  if (claim) {                                                 // what the assembly side claimed before
    uint64_t d = 0;
    if (hipMemcpy(&d, ix->d_meta, sizeof(d), hipMemcpyDeviceToHost) != hipSuccess) {
      mfx_fail(MFX_E_HIP, "%s: reading the table's state failed: %s", who, hipGetErrorString(hipGetLastError()));
      reads_free(r);
      return nullptr;
    }
    r->distinct_known = d;
  }
  // from here on the read side belongs to this counter: no second source of read counts, and -- the update-only counter -- no claim (the frozen rule)
  if (!claim) ix->frozen = true;
  ix->reads_counted = true;
  ix->filter_set = true;
  ix->minV = 0;
  ix->maxV = ~0ull;
  return r;
}

extern "C" mfx_reads *mfx_reads_begin(mfx_index *ix, uint64_t batch_bases) {
  if (!ix) { mfx_fail(MFX_E_INVAL, "mfx_reads_begin: null index"); return nullptr; }
  if (!ix->seq_only && !ix->wide()) {
    mfx_fail(MFX_E_INVAL, "mfx_reads_begin: the index is neither sequence-only nor path-only -- reads are counted only into k-mers claimed "
             "before (mfx_index_create_for_seq + mfx_index_count_asm / mfx_index_claim_seq, or mfx_index_claim_paths)");
    return nullptr;
  }
  return reads_open(ix, batch_bases, "mfx_reads_begin", false);
}

// what a claiming counter asks of the index; `who`: the entry point, for the texts
static bool claim_index_ok(const mfx_index *ix, const char *who) {
  if (!ix) { mfx_fail(MFX_E_INVAL, "%s: null index", who); return false; }
  if (ix->seq_only) {
    mfx_fail(MFX_E_INVAL, "%s: a sequence-only or path-only index holds the k-mers claimed for it and takes no others -- count every "
             "k-mer of the reads into a full index (mfx_index_create), or only the claimed ones with mfx_reads_begin", who);
    return false;
  }
  if (ix->wide()) {
    mfx_fail(MFX_E_INVAL, "%s: the table that grows holds k <= %d; this index holds %d-mers", who, MFX_MAX_K_NARROW, ix->k);
    return false;
  }
  return true;
}

extern "C" mfx_reads *mfx_reads_begin_all(mfx_index *ix, uint64_t batch_bases) {
  if (!claim_index_ok(ix, "mfx_reads_begin_all")) return nullptr;
  return reads_open(ix, batch_bases, "mfx_reads_begin_all", true);
}

extern "C" mfx_reads *mfx_reads_begin_range(mfx_index *ix, uint64_t batch_bases, uint64_t key_lo, uint64_t key_hi) {
  if (!claim_index_ok(ix, "mfx_reads_begin_range")) return nullptr;
  const uint64_t top = 1ull << (2 * ix->k);                    // 4^k (k <= 31)
  if (key_lo > key_hi) {
    mfx_fail(MFX_E_INVAL, "mfx_reads_begin_range: the range starts above its end (key_lo %llu > key_hi %llu)", (unsigned long long)key_lo,
             (unsigned long long)key_hi);
    return nullptr;
  }
  if (key_hi > top) {
    mfx_fail(MFX_E_INVAL, "mfx_reads_begin_range: the range ends beyond the %d-mers (key_hi %llu > 4^%d = %llu)", ix->k, (unsigned long long)key_hi, ix->k,
             (unsigned long long)top);
    return nullptr;
  }
  mfx_reads *r = reads_open(ix, batch_bases, "mfx_reads_begin_range", true);
  if (r && !(key_lo == 0 && key_hi == top)) {                  // every k-mer: the launches of mfx_reads_begin_all
    r->ranged = true;
    r->key_lo = key_lo;
    r->key_hi = key_hi;
  }
  return r;
}

extern "C" int mfx_index_growths(const mfx_index *ix, uint64_t *n, double *seconds, double *rehash_seconds, uint64_t *rehash_bytes) {
  if (!ix) return mfx_fail(MFX_E_INVAL, "mfx_index_growths: null index");
  if (n) *n = ix->grow_count;
  if (seconds) *seconds = ix->grow_seconds;
  if (rehash_seconds) *rehash_seconds = ix->rehash_seconds;
  if (rehash_bytes) *rehash_bytes = ix->rehash_bytes;
  return MFX_OK;
}

extern "C" int mfx_reads_set_filter(mfx_reads *r, uint64_t minV, uint64_t maxV) {
  if (!r) return mfx_fail(MFX_E_INVAL, "mfx_reads_set_filter: null argument");
  r->ix->minV = minV;
  r->ix->maxV = maxV;
  return MFX_OK;
}

extern "C" int mfx_reads_add(mfx_reads *r, const char *const *bases, const uint64_t *lens, uint64_t n) {
  if (!r || (n && (!bases || !lens))) return mfx_fail(MFX_E_INVAL, "mfx_reads_add: null argument");
  if (r->failed) return mfx_fail(MFX_E_INVAL, "mfx_reads_add: an earlier batch failed; end the counter");
  DeviceScope g(r->ix->device);
  return batch_records(r->b, (uint64_t)r->ix->k, bases, lens, n, r->stats.reads, r->stats.bases, "mfx_reads_add", [&]() {
    const int rc = reads_flush(r);
    if (rc) r->failed = true;
    return rc;
  });
}

// ---- the read store ---------------------------------------------------------------------------------------------------------------
static uint64_t store_batch_bytes(uint64_t npos) { return (npos + 31) / 32 * (sizeof(uint64_t) + sizeof(uint32_t)); }

// the batch being filled is complete: its planes are kept
static int store_keep(mfx_reads_store *s) {
  const uint64_t npos = s->b.used;
  if (npos == 0) return MFX_OK;
  if (s->max_bytes && s->bytes + store_batch_bytes(npos) > s->max_bytes) { s->complete = false; return 1; }
  mfx_reads_store::Packed p;
  const uint64_t nw = (npos + 31) / 32;
  p.codes.resize(nw);
  p.valid.resize(nw);
  batch_pack(s->b.bytes.data(), npos, nw, p.codes.data(), p.valid.data());
  p.npos = npos;
  p.reads = s->reads - s->reads_kept;
  p.bases = s->bases - s->bases_kept;
  s->reads_kept = s->reads;
  s->bases_kept = s->bases;
  s->bytes += store_batch_bytes(npos);
  s->batches.push_back(std::move(p));
  s->b.used = 0;
  return MFX_OK;
}

extern "C" mfx_reads_store *mfx_reads_store_create(int k, uint64_t batch_bases, uint64_t max_bytes) {
  if (k < 1 || k > MFX_MAX_K) { mfx_fail(MFX_E_INVAL, "mfx_reads_store_create: k = %d (1 <= k <= %d)", k, MFX_MAX_K); return nullptr; }
  batch_bases = batch_size_checked(batch_bases, k, "mfx_reads_store_create");
  if (batch_bases == 0) return nullptr;
  try {
    mfx_reads_store *s = new mfx_reads_store;
    s->k = k;
    s->max_bytes = max_bytes;
    s->b.cap = batch_bases;
    s->b.bytes.resize(batch_bases + 32);
    return s;
  } catch (const std::bad_alloc &) { mfx_fail(MFX_E_NOMEM, "mfx_reads_store_create: out of memory"); return nullptr; }
}

extern "C" int mfx_reads_store_add(mfx_reads_store *s, const char *const *bases, const uint64_t *lens, uint64_t n) {
  if (!s || (n && (!bases || !lens))) return mfx_fail(MFX_E_INVAL, "mfx_reads_store_add: null argument");
  if (!s->complete) return 1;
  try {
    const int rc = batch_records(s->b, (uint64_t)s->k, bases, lens, n, s->reads, s->bases, "mfx_reads_store_add", [&]() { return store_keep(s); });
    if (rc < 0) s->complete = false;                           // (a record without bases: what came before it is kept, the store is not the read set)
    if (rc) return rc;
    if (s->max_bytes && s->bytes + store_batch_bytes(s->b.used) > s->max_bytes) { s->complete = false; return 1; }
    return MFX_OK;
  } catch (const std::bad_alloc &) {
    s->complete = false;
    return mfx_fail(MFX_E_NOMEM, "mfx_reads_store_add: out of memory (%llu bytes of batches held)", (unsigned long long)s->bytes);
  }
}

extern "C" int mfx_reads_store_info(const mfx_reads_store *s, uint64_t *batches, uint64_t *bytes, uint64_t *reads, uint64_t *n_bases, int *complete) {
  if (!s) return mfx_fail(MFX_E_INVAL, "mfx_reads_store_info: null argument");
  if (batches) *batches = s->batches.size() + (s->b.used ? 1 : 0);
  if (bytes) *bytes = s->bytes + store_batch_bytes(s->b.used);
  if (reads) *reads = s->reads;
  if (n_bases) *n_bases = s->bases;
  if (complete) *complete = s->complete ? 1 : 0;
  return MFX_OK;
}

extern "C" void mfx_reads_store_free(mfx_reads_store *s) { delete s; }

extern "C" int mfx_reads_replay(mfx_reads *r, const mfx_reads_store *s, uint64_t first_batch, uint64_t n_batches) {
  if (!r || !s) return mfx_fail(MFX_E_INVAL, "mfx_reads_replay: null argument");
  if (r->failed) return mfx_fail(MFX_E_INVAL, "mfx_reads_replay: an earlier batch failed; end the counter");
  if (!s->complete) return mfx_fail(MFX_E_INVAL, "mfx_reads_replay: the store is incomplete (it was full before the reads ended): it is not the read set");
  if (s->k != r->ix->k) return mfx_fail(MFX_E_INVAL, "mfx_reads_replay: the store holds batches cut for %d-mers, the counter counts %d-mers", s->k, r->ix->k);
  if (r->b.cap < s->b.cap)
    return mfx_fail(MFX_E_INVAL, "mfx_reads_replay: the counter's batch of %llu bases is smaller than the store's of %llu", (unsigned long long)r->b.cap,
                    (unsigned long long)s->b.cap);
  const uint64_t held = s->batches.size() + (s->b.used ? 1 : 0);
  if (first_batch > held || n_batches > held - first_batch)
    return mfx_fail(MFX_E_INVAL, "mfx_reads_replay: batches [%llu, %llu + %llu) of a store of %llu", (unsigned long long)first_batch,
                    (unsigned long long)first_batch, (unsigned long long)n_batches, (unsigned long long)held);
  DeviceScope g(r->ix->device);
  if (int rc = reads_flush(r)) { r->failed = true; return rc; }               // records of mfx_reads_add before: their batch goes first
  for (uint64_t i = first_batch; i < first_batch + n_batches; ++i) {
    int rc;
    if (i < s->batches.size()) {
      const mfx_reads_store::Packed &p = s->batches[i];
      rc = reads_send(r, p.npos, [&](uint64_t *hc, uint32_t *hv, uint64_t nw) {
        const uint64_t packed = p.codes.size();
        memcpy(hc, p.codes.data(), packed * sizeof(uint64_t));
        memcpy(hv, p.valid.data(), packed * sizeof(uint32_t));
        memset(hc + packed, 0, (nw - packed) * sizeof(uint64_t));
        memset(hv + packed, 0, (nw - packed) * sizeof(uint32_t));
      });
      if (rc == MFX_OK) { r->stats.reads += p.reads; r->stats.bases += p.bases; }
    } else {                                                   // the store's last batch, still as bytes
      const uint64_t npos = s->b.used;
      rc = reads_send(r, npos, [&](uint64_t *hc, uint32_t *hv, uint64_t nw) { batch_pack(s->b.bytes.data(), npos, nw, hc, hv); });
      if (rc == MFX_OK) { r->stats.reads += s->reads - s->reads_kept; r->stats.bases += s->bases - s->bases_kept; }
    }
    if (rc) { r->failed = true; return rc; }
  }
  // records after the last complete batch that brought no bases (shorter than k): counted by the replay that reaches the store's end (also one of no
  // batches: a store whose every record is shorter than k)
  if (first_batch + n_batches == held && s->b.used == 0) { r->stats.reads += s->reads - s->reads_kept; r->stats.bases += s->bases - s->bases_kept; }
  return MFX_OK;
}

extern "C" int mfx_reads_end(mfx_reads *r, mfx_reads_stats *out) {
  if (!r) return mfx_fail(MFX_E_INVAL, "mfx_reads_end: null argument");
  int rc = MFX_OK;
  {
    DeviceScope g(r->ix->device);
    if (!r->failed) rc = reads_flush(r);
    for (auto &s : r->S) {
      const int src = stage_settle(r, s);
      if (rc == MFX_OK) rc = src;
    }
    uint64_t st[4] = {0, 0, 0, 0};
    if (rc == MFX_OK && hipMemcpy(st, r->d_stats, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess)
      rc = mfx_fail(MFX_E_HIP, "mfx_reads_end: reading the counters failed: %s", hipGetErrorString(hipGetLastError()));
    r->stats.kmers = st[0];
    r->stats.counted = st[1];
    r->stats.dropped = st[2];
    r->stats.saturated = st[3];
    if (rc == MFX_OK) rc = mfx_index_check(r->ix);               // a side table that filled up: MFX_E_FULL, as a database load
    if (rc == MFX_OK && r->failed && r->fail_code != MFX_OK) rc = mfx_fail(r->fail_code, "mfx_reads_end: %s", r->fail_text.c_str());
    if (rc == MFX_OK && r->failed) rc = mfx_fail(MFX_E_INVAL, "mfx_reads_end: a batch of this counter failed");
  }
  if (out) *out = r->stats;
  reads_free(r);
  return rc;
}
