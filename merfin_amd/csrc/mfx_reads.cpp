// mfx_reads.cpp -- the read k-mer counter (include/merfin_amd.h: mfx_reads_*): the read counts of a run straight from its
// reads, counted on the device into the k-mers the index already holds (mfx_kernels.hip: mfx_reads_kernel).
//
// Host side.  Records are copied back to back into a byte batch, one 'N' between two of them (no k-mer spans two reads);
// a record longer than the room left is cut, and its rest starts the next batch k-1 bases before the cut, so every k-mer
// is in exactly one batch.  A full batch is packed into 2-bit codes + validity bits (mfx_pack_bases) in one of two pinned
// stages, copied and counted on that stage's stream: the caller parses the next records while the device counts.
#include "mfx_internal.h"
#include "mfx_kernels.h"

#include <string.h>

#include <algorithm>
#include <vector>

extern "C" void mfx_pack_bases(const uint8_t *src, uint64_t n, uint64_t *codes, uint32_t *valid);      // mfx_pack.cpp

namespace {
constexpr uint64_t MFX_READS_BATCH_DEFAULT = 1ull << 26;     // bases per batch: 24 MB of planes per stage
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
}  // namespace

struct mfx_reads {
  mfx_index *ix = nullptr;
  uint64_t cap = 0;                  // bases per batch
  uint64_t words = 0;                // plane words per stage (whole tiles + the halo)
  std::vector<uint8_t> bytes;        // the batch being filled
  uint64_t used = 0;
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

// the batch in r->bytes goes to the device on the next stage
static int reads_flush(mfx_reads *r) {
  if (r->used == 0) return MFX_OK;
  mfx_reads::Stage &s = r->S[r->cur];
  if (int rc = stage_settle(r, s)) return rc;
  const uint64_t npos = r->used;
  const uint64_t ntiles = (npos + MFX_TILE - 1) / MFX_TILE;
  const uint64_t nw = std::min(r->words, ntiles * (MFX_TILE / 32) + MFX_TILE_WORDS_HOST);
  const uint64_t packed = (npos + 31) / 32;
  mfx_pack_bases(r->bytes.data(), npos, s.hc, s.hv);
  if (nw > packed) {                                           // the halo of the last tile: invalid bases
    memset(s.hc + packed, 0, (nw - packed) * sizeof(uint64_t));
    memset(s.hv + packed, 0, (nw - packed) * sizeof(uint32_t));
  }
  mfx_reads_args a;
  a.t = r->ix->view();
  a.codes = s.dc;
  a.valid = s.dv;
  a.npos = npos;
  a.meta = r->ix->d_meta;
  a.stats = r->d_stats;
  MFX_HIP(hipEventRecord(s.e0, s.st));
  MFX_HIP(hipMemcpyAsync(s.dc, s.hc, nw * sizeof(uint64_t), hipMemcpyHostToDevice, s.st));
  MFX_HIP(hipMemcpyAsync(s.dv, s.hv, nw * sizeof(uint32_t), hipMemcpyHostToDevice, s.st));
  MFX_HIP(hipEventRecord(s.e1, s.st));
  MFX_HIP(r->ix->wide() ? mfx_kw_reads(a, s.st) : mfx_k_reads(a, s.st));
  MFX_HIP(hipEventRecord(s.e2, s.st));
  s.busy = true;
  r->cur = (r->cur + 1) % MFX_READS_STAGES;
  r->used = 0;
  return MFX_OK;
}

extern "C" mfx_reads *mfx_reads_begin(mfx_index *ix, uint64_t batch_bases) {
  if (!ix) { mfx_fail(MFX_E_INVAL, "mfx_reads_begin: null index"); return nullptr; }
  if (!ix->seq_only && !ix->wide()) {
    mfx_fail(MFX_E_INVAL, "mfx_reads_begin: the index is neither sequence-only nor path-only -- reads are counted only into k-mers claimed "
             "before (mfx_index_create_for_seq + mfx_index_count_asm / mfx_index_claim_seq, or mfx_index_claim_paths)");
    return nullptr;
  }
  if (ix->shard_n > 1) { mfx_fail(MFX_E_INVAL, "mfx_reads_begin: a sharded index does not take read counts from reads"); return nullptr; }
  if (ix->filter_set || ix->reads_counted) {
    mfx_fail(MFX_E_INVAL, "mfx_reads_begin: the read side of this index already took counts (a database load or an earlier read counter); "
             "an index takes its read counts from one source");
    return nullptr;
  }
  const uint64_t min_batch = 2ull * (uint64_t)ix->k + 2;
  if (batch_bases == 0) batch_bases = MFX_READS_BATCH_DEFAULT;
  if (batch_bases < min_batch) {
    mfx_fail(MFX_E_INVAL, "mfx_reads_begin: a batch of %llu bases is too small for %d-mers (at least %llu)", (unsigned long long)batch_bases,
             ix->k, (unsigned long long)min_batch);
    return nullptr;
  }
  if (batch_bases > (1ull << 34)) { mfx_fail(MFX_E_INVAL, "mfx_reads_begin: batch of %llu bases is beyond 2^34", (unsigned long long)batch_bases); return nullptr; }
  DeviceScope g(ix->device);
  if (!g.ok) { mfx_fail(MFX_E_HIP, "hipSetDevice(%d) failed", ix->device); return nullptr; }
  mfx_reads *r = new mfx_reads;
  r->ix = ix;
  r->cap = batch_bases;
  r->words = (batch_bases + MFX_TILE - 1) / MFX_TILE * (MFX_TILE / 32) + MFX_TILE_WORDS_HOST;
  r->bytes.resize(batch_bases + 32);
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
    mfx_fail(MFX_E_NOMEM, "mfx_reads_begin: staging of %llu bases per batch could not be allocated: %s", (unsigned long long)batch_bases,
             hipGetErrorString(hipGetLastError()));
    reads_free(r);
    return nullptr;
  }
  // from here on the read side belongs to this counter: no claim (the frozen rule), no second source of read counts
  ix->frozen = true;
  ix->reads_counted = true;
  ix->filter_set = true;
  ix->minV = 0;
  ix->maxV = ~0ull;
  return r;
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
  const uint64_t k = (uint64_t)r->ix->k;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t len = lens[i];
    r->stats.reads += 1;
    r->stats.bases += len;
    if (len < k) continue;                                     // no k-mer
    if (!bases[i]) return mfx_fail(MFX_E_INVAL, "mfx_reads_add: record %llu has no bases", (unsigned long long)i);
    const uint8_t *src = reinterpret_cast<const uint8_t *>(bases[i]);
    uint64_t at = 0;
    while (true) {
      if (r->cap - r->used < k) {                              // no whole k-mer fits: the batch goes
        if (int rc = reads_flush(r)) { r->failed = true; return rc; }
      }
      const uint64_t take = std::min(len - at, r->cap - r->used);
      memcpy(r->bytes.data() + r->used, src + at, take);
      r->used += take;
      if (at + take == len) {
        if (r->used < r->cap) r->bytes[r->used++] = 'N';       // (a read that ends the batch needs no separator)
        break;
      }
      at += take - (k - 1);                                    // the rest, from the first k-mer this batch does not hold
      if (int rc = reads_flush(r)) { r->failed = true; return rc; }
    }
  }
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
    if (rc == MFX_OK && r->failed) rc = mfx_fail(MFX_E_INVAL, "mfx_reads_end: a batch of this counter failed");
  }
  if (out) *out = r->stats;
  reads_free(r);
  return rc;
}
