// mfx_bin.cpp -- the driver of -bin (include/merfin_amd.h: mfx_bin_*; the arithmetic: csrc/mfx_bin.h; the kernel: mfx_kernels.hip,
// mfx_bin_kernel): records are cut into batches by the code of the read counters (mfx_batch_records), a full batch is packed into one
// of two pinned stages together with the first positions of its pieces and the first piece of every tile, counted on that stage's
// stream, and the pieces' counts come back on the same stream into pinned memory.  When a stage settles its pieces are folded into the
// records, in input order; a record is final once its last piece is.  No reference counterpart: merfin has no trio mode.
#include "mfx_host.h"
#include "mfx_kernels.h"
#include "mfx_bin.h"

#include <string.h>

#include <deque>
#include <vector>

extern "C" void mfx_pack_bases(const uint8_t *src, uint64_t n, uint64_t *codes, uint32_t *valid);      // mfx_pack.cpp

static_assert(sizeof(mfx_bin_record) == 16, "mfx_bin_record: the kernel adds to the record as two 64-bit words");
static_assert(MFX_BIN_TILE == MFX_TILE, "mfx_bin.h restates the tile");

namespace {
constexpr int MFX_BIN_STAGES = 2;
constexpr uint64_t MFX_TILE_WORDS_HOST = (MFX_TILE + 64) / 32;        // words a tile reads (mfx_device.h: MFX_TILE_WORDS)
}  // namespace

struct mfx_bin {
  const mfx_index *ix = nullptr;
  int device = 0, canon = 0;
  mfx_batch b;                       // the batch being filled
  std::vector<mfx_bin_piece> open;   // ... and its pieces (record: the number since begin)
  uint64_t words = 0;                // plane words per stage (whole tiles + the halo)
  struct Stage {
    uint64_t *hc = nullptr, *dc = nullptr;
    uint32_t *hv = nullptr, *dv = nullptr;
    uint64_t *h_start = nullptr, *d_start = nullptr;      // [room] first positions of the pieces
    uint64_t *h_tile = nullptr, *d_tile = nullptr;        // [tiles of a batch] the first piece of every tile
    uint64_t *h_out = nullptr, *d_out = nullptr;          // [room][2] the pieces' counts
    uint64_t room = 0;                                    // pieces the three arrays hold
    std::vector<mfx_bin_piece> pieces;                    // of the batch in flight
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;    // copies start, kernel starts, kernel done, counts back
    bool busy = false;
  } S[MFX_BIN_STAGES];
  int cur = 0;
  // the records in flight: [taken, taken + recs.size()) of the input order; the first `ready` of them are final
  struct Rec { mfx_bin_record r; bool final; };
  std::deque<Rec> recs;
  uint64_t taken = 0, ready = 0;
  mfx_bin_stats stats{};
  bool failed = false;
};

static void bin_free(mfx_bin *b) {
  if (!b) return;
  DevGuard g(b->device);
  for (auto &s : b->S) {
    if (s.st) (void)hipStreamSynchronize(s.st);
    if (s.hc) (void)hipHostFree(s.hc);
    if (s.hv) (void)hipHostFree(s.hv);
    if (s.h_start) (void)hipHostFree(s.h_start);
    if (s.h_tile) (void)hipHostFree(s.h_tile);
    if (s.h_out) (void)hipHostFree(s.h_out);
    if (s.dc) (void)hipFree(s.dc);
    if (s.dv) (void)hipFree(s.dv);
    if (s.d_start) (void)hipFree(s.d_start);
    if (s.d_tile) (void)hipFree(s.d_tile);
    if (s.d_out) (void)hipFree(s.d_out);
    if (s.e0) (void)hipEventDestroy(s.e0);
    if (s.e1) (void)hipEventDestroy(s.e1);
    if (s.e2) (void)hipEventDestroy(s.e2);
    if (s.e3) (void)hipEventDestroy(s.e3);
    if (s.st) (void)hipStreamDestroy(s.st);
  }
  delete b;
}

// the stage's batch is done: its times are added, its pieces folded into the records, its buffers free
static int stage_settle(mfx_bin *b, mfx_bin::Stage &s) {
  if (!s.busy) return MFX_OK;
  s.busy = false;
  MFX_HIP(hipEventSynchronize(s.e3));
  float m0 = 0, m1 = 0, m2 = 0;
  MFX_HIP(hipEventElapsedTime(&m0, s.e0, s.e1));
  MFX_HIP(hipEventElapsedTime(&m1, s.e1, s.e2));
  MFX_HIP(hipEventElapsedTime(&m2, s.e2, s.e3));
  b->stats.seconds_copy += (m0 + m2) * 1e-3;
  b->stats.seconds_kernel += m1 * 1e-3;
  mfx_bin_fold(s.pieces.data(), s.pieces.size(), reinterpret_cast<const uint32_t *>(s.h_out),
               [&](uint64_t record) { return &b->recs[(size_t)(record - b->taken)].r.kmers; });
  for (const mfx_bin_piece &p : s.pieces)
    if (p.last) b->recs[(size_t)(p.record - b->taken)].final = true;
  s.pieces.clear();
  while (b->ready < b->recs.size() && b->recs[(size_t)b->ready].final) ++b->ready;
  return MFX_OK;
}

// room for the arrays of n pieces in a settled stage
static int stage_room(mfx_bin::Stage &s, uint64_t n) {
  if (n <= s.room) return MFX_OK;
  const uint64_t room = std::max<uint64_t>(std::max<uint64_t>(n, 2 * s.room), 1024);
  if (s.h_start) (void)hipHostFree(s.h_start);
  if (s.h_out) (void)hipHostFree(s.h_out);
  if (s.d_start) (void)hipFree(s.d_start);
  if (s.d_out) (void)hipFree(s.d_out);
  s.h_start = s.h_out = s.d_start = s.d_out = nullptr;
  s.room = 0;
  if (hipHostMalloc((void **)&s.h_start, room * sizeof(uint64_t), hipHostMallocPortable) != hipSuccess ||
      hipHostMalloc((void **)&s.h_out, room * 2 * sizeof(uint64_t), hipHostMallocPortable) != hipSuccess ||
      hipMalloc((void **)&s.d_start, room * sizeof(uint64_t)) != hipSuccess || hipMalloc((void **)&s.d_out, room * 2 * sizeof(uint64_t)) != hipSuccess) {
    (void)hipGetLastError();
    return mfx_fail(MFX_E_NOMEM, "mfx_bin_add: no memory for the %llu pieces of a batch", (unsigned long long)room);
  }
  s.room = room;
  return MFX_OK;
}

// the batch being filled goes to the device on the next stage
static int bin_send(mfx_bin *b) {
  const uint64_t npos = b->b.used, np = b->open.size();
  if (npos == 0) return MFX_OK;
  mfx_bin::Stage &s = b->S[b->cur];
  if (int rc = stage_settle(b, s)) return rc;
  if (int rc = stage_room(s, np)) return rc;
  const uint64_t ntiles = (npos + MFX_TILE - 1) / MFX_TILE;
  const uint64_t nw = std::min(b->words, ntiles * (MFX_TILE / 32) + MFX_TILE_WORDS_HOST);
  const uint64_t packed = (npos + 31) / 32;
  mfx_pack_bases(b->b.bytes.data(), npos, s.hc, s.hv);
  if (nw > packed) {                                           // the words beyond the bases are invalid (the halo of the last tile)
    memset(s.hc + packed, 0, (nw - packed) * sizeof(uint64_t));
    memset(s.hv + packed, 0, (nw - packed) * sizeof(uint32_t));
  }
  for (uint64_t i = 0; i < np; ++i) s.h_start[i] = b->open[i].first;
  mfx_bin_tile_first(b->open.data(), np, npos, s.h_tile);
  mfx_bin_args a;
  a.t = b->ix->view();
  a.canonical = b->canon;
  a.codes = s.dc;
  a.valid = s.dv;
  a.npos = npos;
  a.piece_start = s.d_start;
  a.tile_first = s.d_tile;
  a.npieces = np;
  a.out = s.d_out;
  MFX_HIP(hipEventRecord(s.e0, s.st));
  MFX_HIP(hipMemcpyAsync(s.dc, s.hc, nw * sizeof(uint64_t), hipMemcpyHostToDevice, s.st));
  MFX_HIP(hipMemcpyAsync(s.dv, s.hv, nw * sizeof(uint32_t), hipMemcpyHostToDevice, s.st));
  MFX_HIP(hipMemcpyAsync(s.d_start, s.h_start, np * sizeof(uint64_t), hipMemcpyHostToDevice, s.st));
  MFX_HIP(hipMemcpyAsync(s.d_tile, s.h_tile, ntiles * sizeof(uint64_t), hipMemcpyHostToDevice, s.st));
  MFX_HIP(hipMemsetAsync(s.d_out, 0, np * 2 * sizeof(uint64_t), s.st));
  MFX_HIP(hipEventRecord(s.e1, s.st));
  MFX_HIP(mfx_k_bin(a, s.st));
  MFX_HIP(hipEventRecord(s.e2, s.st));
  MFX_HIP(hipMemcpyAsync(s.h_out, s.d_out, np * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s.st));
  MFX_HIP(hipEventRecord(s.e3, s.st));
  s.pieces.swap(b->open);
  b->open.clear();
  s.busy = true;
  b->cur = (b->cur + 1) % MFX_BIN_STAGES;
  b->b.used = 0;
  return MFX_OK;
}

// the batch size the plan and the device path take; 0: refused (the text is set)
static uint64_t bin_batch_checked(uint64_t batch_bases, int k, const char *who) {
  if (batch_bases == 0) batch_bases = MFX_BATCH_BASES_DEFAULT;
  if (batch_bases < mfx_batch_bases_min(k)) {
    mfx_fail(MFX_E_INVAL, "%s: a batch of %llu bases is too small for %d-mers (at least %llu)", who, (unsigned long long)batch_bases, k,
             (unsigned long long)mfx_batch_bases_min(k));
    return 0;
  }
  if (batch_bases > MFX_BATCH_BASES_MAX) { mfx_fail(MFX_E_INVAL, "%s: batch of %llu bases is beyond 2^34", who, (unsigned long long)batch_bases); return 0; }
  return batch_bases;
}

extern "C" mfx_bin *mfx_bin_begin(mfx_eval *ev, uint64_t batch_bases) {
  if (!ev || !ev->ix) { mfx_fail(MFX_E_INVAL, "mfx_bin_begin: null argument"); return nullptr; }
  const mfx_index *ix = ev->ix;
  if (ix->wide()) {
    mfx_fail(MFX_E_INVAL, "mfx_bin_begin: reads are binned for k <= %d; this index holds %d-mers", MFX_MAX_K_NARROW, ix->k);
    return nullptr;
  }
  if (ix->shard_n > 1) {
    mfx_fail(MFX_E_INVAL, "mfx_bin_begin: the index is shard %u of %u: a read's counts need both sets' whole membership; use a whole index", ix->shard_rank,
             ix->shard_n);
    return nullptr;
  }
  batch_bases = bin_batch_checked(batch_bases, ix->k, "mfx_bin_begin");
  if (batch_bases == 0) return nullptr;
  DevGuard g(ev->device);
  if (!g.ok) { mfx_fail(MFX_E_HIP, "hipSetDevice(%d) failed", ev->device); return nullptr; }
  int canon = 0;
  if (index_canonical(ix, &canon)) return nullptr;
  mfx_bin *b = new mfx_bin;
  b->ix = ix;
  b->device = ev->device;
  b->canon = canon;
  b->b.cap = batch_bases;
  b->b.bytes.resize(batch_bases + 32);
  const uint64_t tiles = (batch_bases + MFX_TILE - 1) / MFX_TILE;
  b->words = tiles * (MFX_TILE / 32) + MFX_TILE_WORDS_HOST;
  bool ok = true;
  for (auto &s : b->S) {
    if (!ok) break;
    ok = hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) == hipSuccess &&
         hipHostMalloc((void **)&s.hc, b->words * sizeof(uint64_t), hipHostMallocPortable) == hipSuccess &&
         hipHostMalloc((void **)&s.hv, b->words * sizeof(uint32_t), hipHostMallocPortable) == hipSuccess &&
         hipHostMalloc((void **)&s.h_tile, tiles * sizeof(uint64_t), hipHostMallocPortable) == hipSuccess &&
         hipMalloc((void **)&s.dc, b->words * sizeof(uint64_t)) == hipSuccess && hipMalloc((void **)&s.dv, b->words * sizeof(uint32_t)) == hipSuccess &&
         hipMalloc((void **)&s.d_tile, tiles * sizeof(uint64_t)) == hipSuccess && hipEventCreate(&s.e0) == hipSuccess &&
         hipEventCreate(&s.e1) == hipSuccess && hipEventCreate(&s.e2) == hipSuccess && hipEventCreate(&s.e3) == hipSuccess;
  }
  if (!ok) {
    mfx_fail(MFX_E_NOMEM, "mfx_bin_begin: staging of %llu bases per batch could not be allocated: %s", (unsigned long long)batch_bases,
             hipGetErrorString(hipGetLastError()));
    bin_free(b);
    return nullptr;
  }
  return b;
}

extern "C" int mfx_bin_add(mfx_bin *b, const char *const *bases, const uint64_t *lens, uint64_t n) {
  if (!b || (n && (!bases || !lens))) return mfx_fail(MFX_E_INVAL, "mfx_bin_add: null argument");
  if (b->failed) return mfx_fail(MFX_E_INVAL, "mfx_bin_add: an earlier batch failed; end the binner");
  const uint64_t k = (uint64_t)b->ix->k;
  for (uint64_t i = 0; i < n; ++i) {                           // before anything of the call is taken
    if (lens[i] >= (1ull << 32))
      return mfx_fail(MFX_E_INVAL, "mfx_bin_add: record %llu has %llu bases: a record's counts are 32-bit, it holds fewer than 2^32 bases", (unsigned long long)i,
                      (unsigned long long)lens[i]);
    if (lens[i] >= k && !bases[i]) return mfx_fail(MFX_E_INVAL, "mfx_bin_add: record %llu has no bases", (unsigned long long)i);
  }
  DevGuard g(b->device);
  const uint64_t rec0 = b->taken + b->recs.size();
  for (uint64_t i = 0; i < n; ++i) b->recs.push_back({{0u, 0u, 0u, 0u}, lens[i] < k});      // (no k-mer: final with zeros, in its place)
  const int rc = mfx_batch_records(b->b, k, bases, lens, n, b->stats.reads, b->stats.bases, [](uint64_t) { return MFX_E_INVAL; },
                                   [&]() { return bin_send(b); },
                                   [&](uint64_t i, uint64_t first, uint64_t len, bool last) { b->open.push_back({rec0 + i, first, len, last}); });
  if (rc) b->failed = true;
  while (b->ready < b->recs.size() && b->recs[(size_t)b->ready].final) ++b->ready;
  return rc;
}

extern "C" int mfx_bin_flush(mfx_bin *b) {
  if (!b) return mfx_fail(MFX_E_INVAL, "mfx_bin_flush: null argument");
  if (b->failed) return mfx_fail(MFX_E_INVAL, "mfx_bin_flush: an earlier batch failed; end the binner");
  DevGuard g(b->device);
  int rc = bin_send(b);
  for (int i = 0; i < MFX_BIN_STAGES; ++i) {                   // in the order they were sent
    const int src = stage_settle(b, b->S[(b->cur + i) % MFX_BIN_STAGES]);
    if (rc == MFX_OK) rc = src;
  }
  if (rc) b->failed = true;
  return rc;
}

extern "C" uint64_t mfx_bin_ready(const mfx_bin *b) { return b ? b->ready : 0; }

extern "C" int mfx_bin_take(mfx_bin *b, mfx_bin_record *dst, uint64_t cap, uint64_t *n_out) {
  if (!b || !n_out || (!dst && cap)) return mfx_fail(MFX_E_INVAL, "mfx_bin_take: null argument");
  const uint64_t n = std::min(cap, b->ready);
  for (uint64_t i = 0; i < n; ++i) {
    const mfx_bin_record &r = b->recs.front().r;
    dst[i] = r;
    b->stats.kmers += r.kmers; b->stats.a += r.a; b->stats.b += r.b; b->stats.shared += r.shared;
    b->recs.pop_front();
  }
  b->taken += n;
  b->ready -= n;
  *n_out = n;
  return MFX_OK;
}

extern "C" int mfx_bin_end(mfx_bin *b, mfx_bin_stats *out) {
  if (!b) return mfx_fail(MFX_E_INVAL, "mfx_bin_end: null argument");
  int rc = MFX_OK;
  if (!b->failed) rc = mfx_bin_flush(b);
  else rc = mfx_fail(MFX_E_INVAL, "mfx_bin_end: a batch of this binner failed");
  for (const mfx_bin::Rec &x : b->recs) {                      // (not taken: lost, but counted)
    b->stats.kmers += x.r.kmers; b->stats.a += x.r.a; b->stats.b += x.r.b; b->stats.shared += x.r.shared;
  }
  if (out) *out = b->stats;
  bin_free(b);
  return rc;
}

extern "C" int mfx_bin_classify(const mfx_bin_record *r, uint64_t n, const mfx_bin_opts *o, uint8_t *cls) {
  if (!o || (n && (!r || !cls))) return mfx_fail(MFX_E_INVAL, "mfx_bin_classify: null argument");
  if (o->ratio_milli < 1000u)
    return mfx_fail(MFX_E_INVAL, "mfx_bin_classify: a ratio of %u / 1000 is below 1: a read could be of both classes", o->ratio_milli);
  for (uint64_t i = 0; i < n; ++i) cls[i] = (uint8_t)mfx_bin_class(r[i].a, r[i].b, o->norm_a, o->norm_b, o->ratio_milli, o->min_hits);
  return MFX_OK;
}

extern "C" int mfx_bin_plan_host(const uint64_t *lens, uint64_t n, int k, uint64_t batch_bases, uint64_t *pieces, uint64_t cap, uint64_t *n_pieces) {
  if ((!lens && n) || !n_pieces || (!pieces && cap)) return mfx_fail(MFX_E_INVAL, "mfx_bin_plan_host: null argument");
  if (k < 1 || k > MFX_MAX_K) return mfx_fail(MFX_E_INVAL, "mfx_bin_plan_host: k = %d is outside [1, %d]", k, MFX_MAX_K);
  batch_bases = bin_batch_checked(batch_bases, k, "mfx_bin_plan_host");
  if (batch_bases == 0) return MFX_E_INVAL;
  mfx_batch b;
  b.cap = batch_bases;
  uint64_t batch = 0, np = 0, reads = 0, nbases = 0;
  mfx_batch_records(b, (uint64_t)k, nullptr, lens, n, reads, nbases, [](uint64_t) { return 0; },
                    [&]() { if (b.used) ++batch; b.used = 0; return 0; },
                    [&](uint64_t i, uint64_t first, uint64_t len, bool) {
                      if (np < cap) { uint64_t *p = pieces + 4 * np; p[0] = batch; p[1] = i; p[2] = first; p[3] = len; }
                      ++np;
                    });
  *n_pieces = np;
  return MFX_OK;
}
