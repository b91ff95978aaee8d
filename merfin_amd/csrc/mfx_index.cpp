// mfx_index.cpp -- the k-mer table: its sizing, creation, the host -> table ingest pipeline, the add / count / build entry points,
// the staged database load, and what reads a table back (value, info, export).
#include "mfx_host.h"
#include "mfx_place.h"
#include "mfx_kernels.h"
#include "mfx_pool.h"

#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace {
// Table fill target.  MFX_LOAD_FACTOR fixes it; otherwise it is chosen per index between MFX_LF_MAX (the least
// memory a table may take: what mfx_index_estimate_gb reports and -memory is checked against) and MFX_LF_MIN,
// as low as a share of the free HBM (and of max_gb) allows: emptier lines mean fewer full home lines and fewer
// second probes (3 Gb -hist, w = 3: 0.7 -> 80, 0.6 -> 85, 0.52 -> 89.8, 0.45 -> 91.5, 0.40 -> 91.2 G k-mers/s: nothing is
// gained below 0.45), and 288 GB of HBM are there to be used.
constexpr double MFX_LF_MAX = 0.7, MFX_LF_MIN = 0.45, MFX_LF_HBM_SHARE = 0.75;
// The compact layout of a sequence-only index (16 slots per line in 8 mini-buckets, buckets of w = 4 windows): the emptier the
// table, the more k-mers sit in their first mini-bucket (one 16-byte load) -- 3 Gb -hist: 102.6 / 108.0 / 111.9 G k-mers/s at load
// factors 0.30 / 0.25 / 0.20 (profiles/r03_kernel_experiments.txt).  Round 4's kernel runs at the HBM's random-line rate, so every
// line not fetched is time: 148.1 / 151.8 / 152.7 / 153.6 / 154.3 G at 0.225 / 0.18 / 0.15 / 0.125 / 0.10
// (profiles/r04_ab_load_factor.txt).  0.18 is 135 GB for a human assembly -- under two thirds of what the full table of reads +
// assembly takes at its 0.45 -- and still chosen only when that much HBM is free (lines_auto).
constexpr double MFX_CLF_MAX = 0.5, MFX_CLF_MIN = 0.18;
// A sequence-only index in 16-byte slots (22 <= k <= 31) holds the assembly's k-mers only -- half of what the full tables hold --
// and gives the memory back as speed: 500 Mb -hist at k = 31: 71.3 / 80.6 / 86.7 G k-mers/s at load factors 0.45 / 0.35 / 0.25
// (profiles/r03_hist_rates_by_k.txt).  0.30 is 160 GB for a human assembly.
constexpr double MFX_SLF_MIN = 0.30;

thread_local double t_lf_request = 0;      // mfx_index_create_for_seq_lf: the caller's load factor for the table being created (0: none)
bool load_factor_fixed(double *lf) {
  const char *e = getenv("MFX_LOAD_FACTOR");
  if (!e && t_lf_request > 0) { *lf = std::min(0.9, std::max(0.05, t_lf_request)); return true; }
  if (!e) return false;
  double v = atof(e);
  if (!(v > 0.05 && v <= 0.9)) v = MFX_LF_MAX;
  *lf = v;
  return true;
}

uint64_t lines_at(uint64_t capacity_kmers, double lf, uint32_t slots_line) {
  double slots = (double)capacity_kmers / lf;
  uint64_t nlines = (uint64_t)ceil(slots / slots_line);
  if (nlines < 1024) nlines = 1024;      // probe sequences may span 512 lines
  return nlines;
}

// smallest table this build makes for `capacity_kmers`
uint64_t lines_for(uint64_t capacity_kmers, uint32_t slots_line = MFX_SLOTS_LINE) {
  double lf = slots_line == MFX_CSLOTS_LINE ? MFX_CLF_MAX : MFX_LF_MAX;
  (void)load_factor_fixed(&lf);
  return lines_at(capacity_kmers, lf, slots_line);
}

// the table actually allocated: budget_bytes = what the table may take (0: unknown, use the smallest)
uint64_t lines_auto(uint64_t capacity_kmers, double budget_bytes, uint32_t slots_line, bool seq_only = false) {
  const double lf_max = slots_line == MFX_CSLOTS_LINE ? MFX_CLF_MAX : MFX_LF_MAX,
               lf_min = slots_line == MFX_CSLOTS_LINE ? MFX_CLF_MIN : (seq_only && slots_line == MFX_SLOTS_LINE) ? MFX_SLF_MIN : MFX_LF_MIN;
  double lf;
  if (load_factor_fixed(&lf)) return lines_at(capacity_kmers, lf, slots_line);
  lf = lf_max;
  if (budget_bytes > 0) {
    lf = (double)capacity_kmers * (MFX_ALIGN / slots_line) / budget_bytes;
    lf = std::min(lf_max, std::max(lf_min, lf));
  }
  uint64_t nl = lines_at(capacity_kmers, lf, slots_line);
  if (nl >= (1ull << 32)) nl = std::max<uint64_t>(lines_at(capacity_kmers, lf_max, slots_line), (1ull << 32) - 16);
  return nl;
}

// does a sequence-only index of k-mers of this size take the compact layout?  (MFX_SEQ_COMPACT=0: never -- A/B, tests)
// k <= 21: the slot holds the k-mer; 22 <= k <= 31: its quotient (mfx_kernels.hip: mfx_q_place), which needs the default
// placement (4 windows, mod-minimizer) and the per-lane probe
bool seq_compact(int k) {
  const char *e = getenv("MFX_SEQ_COMPACT");
  const char *hm = getenv("MFX_HOME_MODE");
  if (k > MFX_MAX_K_COMPACT || (e && atoi(e) == 0) || (hm && strcmp(hm, "plain") == 0)) return false;
  if (k > MFX_MAX_K_DIRECT) {
    const char *ws = getenv("MFX_MZ_W"), *mm = getenv("MFX_MZ_MOD"), *q = getenv("MFX_SEQ_QUOT");
    if ((ws && atoi(ws) != MFX_MZ_W_COMPACT) || (mm && atoi(mm) == 0) || (q && atoi(q) == 0) || !mfx_k_quot_supported()) return false;
  }
  return true;
}
// the fewest lines a quotient table may have: the key field keeps 2m - floor(log2(nlines)) + 9 bits of a k-mer (m = k - 3) in 40
uint64_t quot_min_lines(int k) { return k > MFX_MAX_K_DIRECT ? 1ull << (2 * (k - 3) - 31) : 0; }

// Side table of a compact index (exact counts of the saturated fields, 16-byte slots at load factor <= 0.5): room for
// 1/64 of the capacity -- a count saturates at 2047, i.e. beyond ~70 copies at 30x coverage -- and never fewer than
// 1024 lines.  MFX_SIDE_DIV overrides the divisor; a side table that fills up fails the load with MFX_E_FULL.
uint64_t side_lines_for(uint64_t capacity_kmers) {
  const char *e = getenv("MFX_SIDE_DIV");
  uint64_t div = e && atoll(e) > 0 ? (uint64_t)atoll(e) : 64;
  return std::max<uint64_t>(1024, (capacity_kmers / div) * 2 / MFX_SLOTS_LINE + 1);
}
}  // namespace

// ---------------------------------------------------------------------------
// index
// ---------------------------------------------------------------------------
mfx_table_view mfx_index::view() const {
  mfx_table_view v;
  v.slots = d_slots;
  v.nlines = nlines;
  v.minV = minV > 0xffffffffull ? 0xffffffffu : (uint32_t)minV;
  v.maxV = maxV > 0xffffffffull ? 0xffffffffu : (uint32_t)maxV;
  v.k = k;
  v.mz_w = mz_w;
  v.mz_t = mz_t;
  v.shard_rank = shard_rank;
  v.shard_n = shard_n;
  v.wide = wide() ? 1 : 0;
  v.seq_only = seq_only ? 1 : 0;
  v.compact = compact ? 1 : 0;
  v.quot = quot ? 1 : 0;
  v.qshift = 0;
  for (uint64_t x = nlines; x > 1; x >>= 1) ++v.qshift;      // floor(log2(nlines))
  v.side = compact ? d_slots + nlines * MFX_SLOTS_LINE : nullptr;      // the side table follows the main lines
  v.side_nlines = side_nlines;
  return v;
}

extern "C" double mfx_index_estimate_gb(int k, uint64_t capacity_kmers) {
  return (double)lines_for(capacity_kmers, k > MFX_MAX_K_NARROW ? MFX_WSLOTS_LINE : MFX_SLOTS_LINE) * MFX_ALIGN / 1e9;
}

// bytes of the smallest 16-byte-slot / compact sequence-only table for this capacity
static double seq_plain_bytes(uint64_t capacity_kmers) { return (double)lines_for(capacity_kmers, MFX_SLOTS_LINE) * MFX_ALIGN; }
static double seq_compact_bytes(int k, uint64_t capacity_kmers) {
  return (double)(std::max(lines_for(capacity_kmers, MFX_CSLOTS_LINE), quot_min_lines(k)) + side_lines_for(capacity_kmers)) * MFX_ALIGN;
}
// The quotient form needs a table of at least 2^(2(k-3)-31) lines (4 GB at k = 31) whatever the genome's size: a small genome under a
// small -memory limit (or on a nearly full device) takes the 16-byte slots, sized by the genome, instead (budget_bytes 0: no limit known).
static bool seq_compact_fits(int k, uint64_t capacity_kmers, double budget_bytes) {
  if (!seq_compact(k)) return false;
  if (k <= MFX_MAX_K_DIRECT || budget_bytes <= 0) return true;
  const double cb = seq_compact_bytes(k, capacity_kmers);
  return cb <= budget_bytes || cb <= seq_plain_bytes(capacity_kmers);
}

extern "C" double mfx_index_estimate_gb_for_seq(int k, uint64_t capacity_kmers) {
  if (k > MFX_MAX_K_NARROW) return mfx_index_estimate_gb(k, capacity_kmers);
  if (!seq_compact(k)) return seq_plain_bytes(capacity_kmers) / 1e9;
  // (the smaller of the two layouts a run may take: index_create falls back to the 16-byte slots when the quotient form's floor does not fit)
  return std::min(seq_compact_bytes(k, capacity_kmers), k > MFX_MAX_K_DIRECT ? seq_plain_bytes(capacity_kmers) : 1e300) / 1e9;
}

static mfx_index *index_create(int k, uint64_t capacity_kmers, double max_gb, int device, bool seq_only);

extern "C" mfx_index *mfx_index_create(int k, uint64_t capacity_kmers, double max_gb, int device) {
  return index_create(k, capacity_kmers, max_gb, device, false);
}

extern "C" mfx_index *mfx_index_create_for_seq(int k, uint64_t capacity_kmers, double max_gb, int device) {
  if (k > MFX_MAX_K_NARROW) {
    mfx_fail(MFX_E_INVAL, "a sequence-only index handles k <= %d; this one would hold %d-mers (use mfx_index_create)", MFX_MAX_K_NARROW, k);
    return nullptr;
  }
  return index_create(k, capacity_kmers, max_gb, device, true);
}

// The table's load factor chosen by the caller instead of by the free memory (0: as mfx_index_create_for_seq; MFX_LOAD_FACTOR still
// overrides).  The emptiest table is the fastest to probe (3 Gb, k = 21: 151.8 G k-mers/s at 0.18 = 135 GB against 136 G at 0.4 = 61 GB)
// but not the fastest RUN: a process that starts behind another one waits in hipMalloc while the driver clears what that one freed,
// and how long depends on how much of the HBM both want (profiles/r05_e2e_lf_ab.txt: `merfin -hist` at 3 Gb back to back 4.5-4.9 s at
// 0.18, 1.2-1.3 s at 0.4) -- the CLI asks for 0.4, a resident service for 0.18.
extern "C" mfx_index *mfx_index_create_for_seq_lf(int k, uint64_t capacity_kmers, double max_gb, int device, double load_factor) {
  t_lf_request = load_factor > 0 ? load_factor : 0;
  mfx_index *ix = mfx_index_create_for_seq(k, capacity_kmers, max_gb, device);
  t_lf_request = 0;
  return ix;
}

// (the full table likewise: the variant modes and -completeness of the CLI ask for the smallest table, 0.7 -- their device stage is a
// hundredth of the run, the table's allocation behind another process is seconds)
extern "C" mfx_index *mfx_index_create_lf(int k, uint64_t capacity_kmers, double max_gb, int device, double load_factor) {
  t_lf_request = load_factor > 0 ? load_factor : 0;
  mfx_index *ix = mfx_index_create(k, capacity_kmers, max_gb, device);
  t_lf_request = 0;
  return ix;
}

static mfx_index *index_create(int k, uint64_t capacity_kmers, double max_gb, int device, bool seq_only) {
  if (k < 1 || k > MFX_MAX_K) {
    mfx_fail(MFX_E_INVAL, "k=%d unsupported: k-mers hold 2k <= 128 bits, 1 <= k <= 64", k);
    return nullptr;
  }
  if (mfx_device_count() <= device || device < 0) {
    mfx_fail(MFX_E_NODEVICE, "HIP device %d not available (%d visible); merfin_amd has no CPU path", device, mfx_device_count());
    return nullptr;
  }
  bool compact = seq_only && seq_compact(k);
  if (compact && k > MFX_MAX_K_DIRECT) {                      // the quotient form's floor against -memory and the free device memory
    double budget = max_gb > 0 ? max_gb * 1e9 : 0;
    DevGuard bg(device);
    size_t free_b = 0, total_b = 0;
    if (bg.ok && hipMemGetInfo(&free_b, &total_b) == hipSuccess) { const double fb = MFX_LF_HBM_SHARE * (double)free_b; budget = budget > 0 ? std::min(budget, fb) : fb; }
    else (void)hipGetLastError();
    compact = seq_compact_fits(k, capacity_kmers, budget);
  }
  const uint32_t slots_line = k > MFX_MAX_K_NARROW ? MFX_WSLOTS_LINE : compact ? MFX_CSLOTS_LINE : MFX_SLOTS_LINE;
  if (lines_for(capacity_kmers, slots_line) >= 0xfffffff0ull) {
    mfx_fail(MFX_E_INVAL, "capacity of %lu k-mers needs more than 2^32 table lines (512 GB); shard the index instead",
             (unsigned long)capacity_kmers);
    return nullptr;
  }
  double need = !seq_only ? mfx_index_estimate_gb(k, capacity_kmers) : k > MFX_MAX_K_NARROW ? mfx_index_estimate_gb(k, capacity_kmers)
                : compact ? seq_compact_bytes(k, capacity_kmers) / 1e9 : seq_plain_bytes(capacity_kmers) / 1e9;
  if (max_gb > 0 && need > max_gb) {
    // merfin-globals.C:148-153
    mfx_fail(MFX_E_NOMEM, "Not enough memory to load databases.  Increase -memory. (need %.3f GB, limit %.3f GB)", need, max_gb);
    return nullptr;
  }
  DevGuard g(device);
  if (!g.ok) { mfx_fail(MFX_E_HIP, "hipSetDevice(%d) failed", device); return nullptr; }
  mfx_index *ix = new mfx_index;
  ix->device = device;
  ix->k = k;
  ix->capacity_kmers = capacity_kmers;
  ix->max_gb = max_gb > 0 ? max_gb : 0;
  ix->seq_only = seq_only;
  ix->compact = compact;
  ix->quot = compact && k > MFX_MAX_K_DIRECT;
  ix->side_nlines = compact ? side_lines_for(capacity_kmers) : 0;
  {
    size_t free_b = 0, total_b = 0;
    double budget = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = MFX_LF_HBM_SHARE * (double)free_b;
    if (max_gb > 0) budget = budget > 0 ? std::min(budget, max_gb * 1e9) : max_gb * 1e9;
    if (budget > 0) budget = std::max(1.0, budget - (double)ix->side_nlines * MFX_ALIGN);
    ix->nlines = lines_auto(capacity_kmers, budget, slots_line, seq_only);
    if (ix->quot) ix->nlines = std::max(ix->nlines, quot_min_lines(k));     // (k = 31: 4 GB of table at least; a small genome's table is mostly air)
  }
  if (ix->nlines >= (1ull << 32)) {        // line numbers are 32-bit on the device (550 GB of table: beyond one GPU anyway)
    mfx_fail(MFX_E_NOMEM, "Not enough memory to load databases.  %lu k-mers need %.0f GB on one GPU; shard the index (mfx_index_set_shard).",
             (unsigned long)capacity_kmers, (double)ix->nlines * MFX_ALIGN / 1e9);
    delete ix;
    return nullptr;
  }
  {
    // placement: "mz" (default) = minimizer-keyed home line, consecutive k-mers share 128-byte lines;
    // "plain" = k-mer hash only.  w = 3 windows (m = k-2) by default; w = 2 bounds every minimizer's bucket by
    // one line (a (k-1)-mer is contained in at most 8 k-mers) at 0.69 instead of 0.53 line fetches per k-mer.
    const char *hm = getenv("MFX_HOME_MODE");
    bool mz = hm ? (strcmp(hm, "plain") != 0) : true;
    const char *ws = getenv("MFX_MZ_W");
    const int w_default = compact ? MFX_MZ_W_COMPACT : MFX_MZ_W_DEFAULT;
    int w = ws ? atoi(ws) : w_default;
    if (w < 1 || w > 5) w = w_default;
    ix->mz_w = (mz && !ix->wide()) ? std::min(w, k) : 0;    // 128-bit k-mers: plain hashing (mfx_wide.hip)
    // compact layout: the window is sampled by the k-mer's smallest t-mer (mod-minimizer: 0.30 instead of 0.40 lines per k-mer);
    // t makes (k - t) % 4 == 3, which makes the choice the same on both strands.  MFX_MZ_MOD=0: the smallest m-mer, as the other layouts.
    {
      const char *mm = getenv("MFX_MZ_MOD");
      // (w = 5, MFX_MZ_W=5, direct form only: t = 4 .. 8 with (k - t) % 5 == 4)
      const bool modw = ix->mz_w == 4 || (ix->mz_w == 5 && !ix->quot);
      ix->mz_t = (compact && modw && k >= 13 && !(mm && atoi(mm) == 0)) ? (ix->mz_w == 4 ? ((k + 1) & 3) + 4 : 4 + ((k - 8) % 5)) : 0;
    }
  }
  hipError_t e = hipMalloc((void **)&ix->d_slots, ix->total_lines() * MFX_ALIGN);
  if (e != hipSuccess && ix->nlines > std::max(lines_for(capacity_kmers, slots_line), quot_min_lines(ix->quot ? k : 0))) {
    // the roomier table did not fit after all (fragmentation, another process): fall back to the smallest one
    (void)hipGetLastError();
    ix->nlines = std::max(lines_for(capacity_kmers, slots_line), quot_min_lines(ix->quot ? k : 0));
    e = hipMalloc((void **)&ix->d_slots, ix->total_lines() * MFX_ALIGN);
  }
  if (e != hipSuccess) {
    mfx_fail(MFX_E_NOMEM, "hipMalloc of %.3f GB for the k-mer table failed: %s", need, hipGetErrorString(e));
    delete ix;
    return nullptr;
  }
  if (hipMalloc((void **)&ix->d_meta, MFX_META_WORDS * sizeof(uint64_t)) != hipSuccess ||
      mfx_memset_now(ix->d_meta, 0, MFX_META_WORDS * sizeof(uint64_t)) != hipSuccess ||
      (ix->wide() ? hipMemsetAsync(ix->d_slots, 0, ix->nlines * MFX_ALIGN, nullptr)           // state 0 = empty
       : ix->compact ? hipMemsetAsync(ix->d_slots, 0xff, ix->nlines * MFX_ALIGN, nullptr)      // 8-byte slots: the all-ones word is empty
                     : mfx_k_table_init(ix->d_slots, ix->nlines * MFX_SLOTS_LINE, nullptr)) != hipSuccess ||
      (ix->compact && mfx_k_table_init(ix->d_slots + ix->nlines * MFX_SLOTS_LINE, ix->side_nlines * MFX_SLOTS_LINE, nullptr) != hipSuccess) ||
      hipDeviceSynchronize() != hipSuccess) {
    mfx_fail(MFX_E_HIP, "k-mer table initialisation failed: %s", hipGetErrorString(hipGetLastError()));
    mfx_index_free(ix);
    return nullptr;
  }
  return ix;
}

extern "C" void mfx_index_free(mfx_index *ix) {
  if (!ix) return;
  DevGuard g(ix->device);
  mfx_index_ingest_release(ix);
  if (ix->d_slots) (void)hipFree(ix->d_slots);
  if (ix->d_meta) (void)hipFree(ix->d_meta);
  delete ix;
}

static mfx_ingest *ingest_get(mfx_index *ix, uint64_t n);

static int index_check(mfx_index *ix) {
  ix->version++;
  uint64_t meta[5];
  MFX_HIP(hipMemcpy(meta, ix->d_meta, sizeof(meta), hipMemcpyDeviceToHost));
  if (meta[4] != 0)
    return mfx_fail(MFX_E_FORMAT, "the database holds %lu records wider than 2k = %d bits: damaged or not a %d-mer database (none was inserted)",
                    (unsigned long)meta[4], 2 * ix->k, ix->k);
  if (meta[2] != 0)
    return mfx_fail(MFX_E_FULL, "k-mer table full: %lu inserts hit the probe limit (capacity %lu k-mers, %lu stored)",
                    (unsigned long)meta[2], (unsigned long)ix->capacity_kmers, (unsigned long)meta[0]);
  if ((double)meta[0] > 0.92 * (double)(ix->nlines * ix->slots_per_line()))
    return mfx_fail(MFX_E_FULL, "k-mer table over-full: %lu k-mers in %lu slots; create the index with a larger capacity",
                    (unsigned long)meta[0], (unsigned long)(ix->nlines * ix->slots_per_line()));
  if (ix->seq_only && meta[1] != 0)
    return mfx_fail(MFX_E_NONCANON, "the database holds %lu non-canonical k-mers: a sequence-only index keeps one slot per canonical k-mer of the "
                    "sequence and cannot answer value(fmer) + value(rmer) for it; build a full index (mfx_index_create)", (unsigned long)meta[1]);
  return MFX_OK;
}

int mfx_index_check(mfx_index *ix) { return index_check(ix); }

// a table of 32 <= k <= 64 claims whatever it is given (mfx_wide.hip): once reads were counted into it, a k-mer it took now would lack
// their counts -- its assembly side comes before mfx_reads_begin
int mfx_reads_claim_error(const mfx_index *ix, const char *who) {
  return mfx_fail(MFX_E_INVAL, "%s: reads were counted into this table of %d-mers (mfx_reads_begin); a table of k > %d claims every k-mer it is "
                  "given, and one claimed now would lack the reads' counts -- give the assembly side before the reads", who, ix->k, MFX_MAX_K_NARROW);
}

// Host -> table pipeline.  LANES of pinned staging are filled by the host and emptied over PCIe into a RING of device
// buffers; the insert kernel of a chunk runs on the device buffer.  The two are decoupled (round 4): a lane is free again
// as soon as its chunk has crossed the link, a device buffer once its chunk is inserted -- so the transfers run ahead of
// the inserts by the depth of the ring (up to MFX_INGEST_RING_BYTES, 3 GB), e.g. while the kernel that claims the
// sequence's k-mers is still running (mfx_index_build_for_hist: the inserts wait for it, the link does not).
// Lanes and ring belong to the index and are REUSED by every load call (pinning memory costs ~0.4 ms per MB: allocating
// them per call was 3.5 s of a 5.1 s ingest at 1 Gb); they are released with the index (or by mfx_index_ingest_release).
constexpr uint64_t MFX_INGEST_CHUNK = 1ull << 24;           // k-mers per lane: 128 MB of keys + 64 MB of counts
constexpr int MFX_INGEST_MAX_LANES = 4, MFX_INGEST_MAX_RING = 64, MFX_INGEST_STREAMS = 4;
struct mfx_ingest {
  struct Lane {
    uint64_t *hk = nullptr;
    uint32_t *hv = nullptr;
    hipEvent_t copied = nullptr;   // the lane's chunk has left the pinned buffer (recorded on the copy stream)
    bool busy = false;
  } L[MFX_INGEST_MAX_LANES];
  struct Dev {
    uint64_t *dk = nullptr;
    uint32_t *dv = nullptr;
    hipEvent_t done = nullptr;     // the buffer's chunk is inserted
    bool busy = false;
  } D[MFX_INGEST_MAX_RING];
  hipStream_t cs = nullptr;                                  // the copy stream
  hipStream_t is[MFX_INGEST_STREAMS] = {nullptr, nullptr, nullptr, nullptr};   // insert streams, ring buffer r uses is[r % 4]
  hipEvent_t after = nullptr;  // inserts wait for this event (the claim / count kernel of mfx_index_build_for_hist); owned here
  int nl = 2;                  // lanes in use (MFX_INGEST_LANES)
  int nd = 2;                  // ring buffers in use
  uint64_t cap = 0;            // k-mers per lane
  size_t kw = 1;
};

static void ingest_free(mfx_ingest *g) {
  if (!g) return;
  if (g->cs) { (void)hipStreamSynchronize(g->cs); }
  for (auto &st : g->is) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
  if (g->cs) (void)hipStreamDestroy(g->cs);
  if (g->after) { (void)hipEventSynchronize(g->after); (void)hipEventDestroy(g->after); }
  for (auto &l : g->L) {
    if (l.hk) (void)hipHostFree(l.hk);
    if (l.hv) (void)hipHostFree(l.hv);
    if (l.copied) (void)hipEventDestroy(l.copied);
  }
  for (auto &d : g->D) {
    if (d.dk) (void)hipFree(d.dk);
    if (d.dv) (void)hipFree(d.dv);
    if (d.done) (void)hipEventDestroy(d.done);
  }
  delete g;
}

void mfx_index_ingest_release(mfx_index *ix) {
  if (!ix || !ix->ingest) return;
  DevGuard g(ix->device);
  ingest_free(ix->ingest);
  ix->ingest = nullptr;
}

static mfx_ingest *ingest_get(mfx_index *ix, uint64_t n) {
  uint64_t chunk = MFX_INGEST_CHUNK;
  if (const char *e = getenv("MFX_INGEST_CHUNK_LOG2")) { const int lg = atoi(e); if (lg >= 16 && lg <= 28) chunk = 1ull << lg; }
  const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(n, 1), chunk);
  // lanes of 4 M k-mers or more serve any load (it goes through them in chunks): re-pinning larger ones costs more than they save
  if (ix->ingest && (ix->ingest->cap >= want || ix->ingest->cap >= (1ull << 22))) return ix->ingest;
  hipEvent_t keep_after = nullptr;                          // (an event the inserts must wait for survives a re-sizing of the lanes)
  if (ix->ingest) { keep_after = ix->ingest->after; ix->ingest->after = nullptr; }
  mfx_index_ingest_release(ix);
  // small loads (tests, single contigs) get small lanes; the first large one gets the full-size lanes
  uint64_t cap = 1ull << 16;
  while (cap < want) cap <<= 1;
  mfx_ingest *g = new mfx_ingest;
  g->after = keep_after;
  g->cap = cap;
  g->kw = ix->key_words();
  // three or more lanes let the fill of a chunk, the transfer of the one before and the insert of the one before that overlap;
  // small loads keep two (pinning costs 0.4 ms per MB)
  g->nl = cap >= (1ull << 20) ? 4 : 2;
  if (const char *e = getenv("MFX_INGEST_LANES")) { const int v = atoi(e); if (v >= 2 && v <= MFX_INGEST_MAX_LANES) g->nl = v; }
  // the ring: as many device buffers as MFX_INGEST_RING_BYTES hold (large loads), never fewer than the lanes
  const uint64_t buf_bytes = cap * 8 * g->kw + cap * 4;
  uint64_t ring_bytes = cap >= (1ull << 20) ? (3ull << 30) : 0;
  if (const char *e = getenv("MFX_INGEST_RING_MB")) ring_bytes = (uint64_t)std::max(0, atoi(e)) << 20;
  g->nd = (int)std::min<uint64_t>(MFX_INGEST_MAX_RING, std::max<uint64_t>((uint64_t)g->nl, ring_bytes / buf_bytes));
  bool ok = hipStreamCreateWithFlags(&g->cs, hipStreamNonBlocking) == hipSuccess;
  for (int si = 0; si < MFX_INGEST_STREAMS && ok; ++si) ok = hipStreamCreateWithFlags(&g->is[si], hipStreamNonBlocking) == hipSuccess;
  for (int li = 0; li < g->nl && ok; ++li) {
    auto &l = g->L[li];
    ok = hipHostMalloc((void **)&l.hk, cap * 8 * g->kw, hipHostMallocPortable) == hipSuccess &&      // DMA source for any device
         hipHostMalloc((void **)&l.hv, cap * 4, hipHostMallocPortable) == hipSuccess &&
         hipEventCreateWithFlags(&l.copied, hipEventDisableTiming) == hipSuccess;
  }
  for (int di = 0; di < g->nd && ok; ++di) {
    auto &d = g->D[di];
    const bool got = hipMalloc((void **)&d.dk, cap * 8 * g->kw) == hipSuccess && hipMalloc((void **)&d.dv, cap * 4) == hipSuccess &&
                     hipEventCreateWithFlags(&d.done, hipEventDisableTiming) == hipSuccess;
    if (!got) {
      (void)hipGetLastError();
      if (d.dk) { (void)hipFree(d.dk); d.dk = nullptr; }
      if (d.dv) { (void)hipFree(d.dv); d.dv = nullptr; }
      if (d.done) { (void)hipEventDestroy(d.done); d.done = nullptr; }
      if (di >= g->nl) { g->nd = di; break; }                // a shorter ring will do (the HBM is full of table)
      ok = false;
    }
  }
  if (!ok) { (void)hipGetLastError(); ingest_free(g); return nullptr; }
  ix->ingest = g;
  return g;
}

// The staging loop of every host-side load.  next(cap, hk, hv, d): put the next chunk of the source into the pinned lane
// buffers (room: cap * 8 * key_words bytes in hk, cap * 4 in hv) and describe it in d -- 1 = a chunk is ready, 0 = the
// source is done, -1 = it failed.  ONE source, nix tables: the chunk is staged once (in the first index's pinned lane)
// and sent to every index's device over that device's own PCIe link; each table inserts what it keeps (a sharded index
// skips the k-mers it does not own in the insert kernel).  nix = 1 is the ordinary load.
struct IngestChunk {
  size_t kbytes = 0, vbytes = 0;                             // what goes over the link from hk / hv
  // enqueue the insert of the chunk (device copies at dk / dv) on st
  std::function<hipError_t(mfx_index *ix, uint64_t *dk, uint32_t *dv, hipStream_t st)> launch;
};

template <class Next>
static int index_ingest_chunks(mfx_index *const *ixs, uint32_t nix, uint64_t n_hint, Next &&next) {
  const bool timing = getenv("MFX_INGEST_TIMING") != nullptr;
  auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_begin = now();
  double t_wait = 0, t_fill = 0;
  uint64_t nchunks = 0, nbytes = 0;
  std::vector<mfx_ingest *> gs(nix, nullptr);
  for (uint32_t i = 0; i < nix; ++i)
    if (ixs[i]->reads_counted && ixs[i]->wide()) return mfx_reads_claim_error(ixs[i], "mfx_index_add / load");
  for (uint32_t i = 0; i < nix; ++i) {
    DevGuard dg(ixs[i]->device);
    ixs[i]->frozen = true;                                  // a sequence-only index takes no more claims once counts arrive
    gs[i] = ingest_get(ixs[i], n_hint);
    if (!gs[i]) return mfx_fail(MFX_E_NOMEM, "mfx_index_add: staging allocation failed");
  }
  const double t_lanes = now() - t_begin;
  uint64_t cap = gs[0]->cap;
  for (uint32_t i = 1; i < nix; ++i) cap = std::min(cap, gs[i]->cap);
  bool ok = true, src_ok = true;
  int nl = gs[0]->nl;
  for (uint32_t i = 1; i < nix; ++i) nl = std::min(nl, gs[i]->nl);
  // the inserts of a table wait for whatever still claims its k-mers (mfx_index_build_for_hist); the transfers do not
  for (uint32_t i = 0; i < nix && ok; ++i)
    if (gs[i]->after) {
      DevGuard dg(ixs[i]->device);
      for (auto &st : gs[i]->is) if (hipStreamWaitEvent(st, gs[i]->after, 0) != hipSuccess) ok = false;
    }
  std::vector<uint64_t> ring_at(nix, 0);                     // chunks sent to table i so far: chunk c lands in ring buffer c % nd
  for (int cur = 0; ok; cur = (cur + 1) % nl) {
    const double t0 = now();
    for (uint32_t i = 0; i < nix && ok; ++i) {               // the lane's previous chunk has left the pinned buffer everywhere
      mfx_ingest::Lane &l = gs[i]->L[cur];
      if (l.busy) { DevGuard dg(ixs[i]->device); if (hipEventSynchronize(l.copied) != hipSuccess) ok = false; }
      l.busy = false;
    }
    if (!ok) break;
    mfx_ingest::Lane &src = gs[0]->L[cur];
    IngestChunk d;
    const double t1 = now();
    const int got = next(cap, src.hk, src.hv, d);
    t_wait += t1 - t0; t_fill += now() - t1;
    if (got < 0) src_ok = false;
    if (got <= 0) break;
    ++nchunks; nbytes += d.kbytes + d.vbytes;
    for (uint32_t i = 0; i < nix && ok; ++i) {
      mfx_index *ix = ixs[i];
      mfx_ingest *g = gs[i];
      const int r = (int)(ring_at[i]++ % (uint64_t)g->nd);
      mfx_ingest::Dev &dv = g->D[r];
      hipStream_t ist = g->is[r % MFX_INGEST_STREAMS];
      DevGuard dg(ix->device);
      // the ring buffer is free once its previous chunk is inserted: the COPY STREAM waits for that, not the host
      ok = (!dv.busy || hipStreamWaitEvent(g->cs, dv.done, 0) == hipSuccess) &&
           (d.kbytes == 0 || hipMemcpyAsync(dv.dk, src.hk, d.kbytes, hipMemcpyHostToDevice, g->cs) == hipSuccess) &&
           (d.vbytes == 0 || hipMemcpyAsync(dv.dv, src.hv, d.vbytes, hipMemcpyHostToDevice, g->cs) == hipSuccess) &&
           hipEventRecord(g->L[cur].copied, g->cs) == hipSuccess &&
           hipStreamWaitEvent(ist, g->L[cur].copied, 0) == hipSuccess &&
           d.launch(ix, dv.dk, dv.dv, ist) == hipSuccess && hipEventRecord(dv.done, ist) == hipSuccess;
      g->L[cur].busy = true;
      dv.busy = true;
    }
  }
  for (uint32_t i = 0; i < nix; ++i) {
    DevGuard dg(ixs[i]->device);
    if (hipStreamSynchronize(gs[i]->cs) != hipSuccess) ok = false;
    for (auto &st : gs[i]->is) if (hipStreamSynchronize(st) != hipSuccess) ok = false;
    for (int li = 0; li < gs[i]->nl; ++li) gs[i]->L[li].busy = false;
    for (int di = 0; di < gs[i]->nd; ++di) gs[i]->D[di].busy = false;
    if (gs[i]->after) {                                      // what the inserts waited for is over as well: its errors are in meta
      if (hipEventSynchronize(gs[i]->after) != hipSuccess) ok = false;
      (void)hipEventDestroy(gs[i]->after);
      gs[i]->after = nullptr;
    }
  }
  if (timing)
    fprintf(stderr, "-- ingest: %.3f s = lanes %.3f (cap %llu, ring %d) + fill %.3f + waits for the link %.3f + drain; %llu chunks, %.2f GB over the link\n",
            now() - t_begin, t_lanes, (unsigned long long)cap, gs[0]->nd, t_fill, t_wait, (unsigned long long)nchunks, nbytes / 1e9);
  if (!ok) return mfx_fail(MFX_E_HIP, "mfx_index_add: transfer / insert failed: %s", hipGetErrorString(hipGetLastError()));
  if (!src_ok) return mfx_last_error_code() ? mfx_last_error_code() : MFX_E_IO;
  for (uint32_t i = 0; i < nix; ++i) {
    DevGuard dg(ixs[i]->device);
    int rc = index_check(ixs[i]);
    if (rc) return rc;
  }
  return MFX_OK;
}

// fill(o, m, hk, hv): put k-mers [o, o+m) of the source into the pinned lane buffers; false = the source failed.
// packed: the records carry their counts (MFX_PACKED_VBITS), nothing comes through hv.
template <class Fill>
static int index_ingest_multi(mfx_index *const *ixs, uint32_t nix, uint64_t n, int side, Fill &&fill, bool packed = false) {
  uint64_t o = 0;
  return index_ingest_chunks(ixs, nix, n, [&](uint64_t cap, uint64_t *hk, uint32_t *hv, IngestChunk &d) {
    if (o >= n) return 0;
    const uint64_t m = std::min(cap, n - o);
    if (!fill(o, m, hk, hv)) return -1;
    o += m;
    d.kbytes = m * 8 * ixs[0]->key_words();
    d.vbytes = packed ? 0 : m * 4;
    d.launch = [m, side, packed](mfx_index *ix, uint64_t *dk, uint32_t *dv, hipStream_t st) {
      return ix->wide() ? mfx_kw_table_add(ix->view(), dk, dv, m, side, ix->d_meta, st)
                        : mfx_k_table_add(ix->view(), dk, packed ? nullptr : dv, m, side, ix->d_meta, st);
    };
    return 1;
  });
}

template <class Fill>
static int index_ingest(mfx_index *ix, uint64_t n, int side, Fill &&fill) {
  return index_ingest_multi(&ix, 1, n, side, fill);
}

static int set_read_filter(mfx_index *ix, uint64_t minV, uint64_t maxV) {
  if (ix->reads_counted)
    return mfx_fail(MFX_E_INVAL, "mfx_index_add_read / load: the read side of this index was counted from reads (mfx_reads_begin); an index takes its "
                    "read counts from one source");
  if (ix->filter_set && (ix->minV != minV || ix->maxV != maxV))
    return mfx_fail(MFX_E_INVAL, "mfx_index_add_read: -min/-max must be the same for every batch of one index");
  ix->minV = minV; ix->maxV = maxV; ix->filter_set = true;
  return MFX_OK;
}

static int check_same_kind(mfx_index *const *ixs, uint32_t nix, const char *who) {
  if (!ixs || nix == 0) return mfx_fail(MFX_E_INVAL, "%s: no index", who);
  for (uint32_t i = 0; i < nix; ++i)
    if (!ixs[i] || ixs[i]->k != ixs[0]->k) return mfx_fail(MFX_E_INVAL, "%s: the indexes of one load must hold the same k", who);
  return MFX_OK;
}

// host arrays into several tables at once (the shards of one process): side 0 read counts (filter applies), 1 assembly
int mfx_index_add_multi(mfx_index *const *ixs, uint32_t nix, const uint64_t *kmers, const uint32_t *values, uint64_t n, int side,
                        uint64_t minV, uint64_t maxV) {
  int rc = check_same_kind(ixs, nix, "mfx_index_add_multi");
  if (rc) return rc;
  if (n && (!kmers || !values)) return mfx_fail(MFX_E_INVAL, "mfx_index_add_multi: null argument");
  if (side == 0) for (uint32_t i = 0; i < nix; ++i) if ((rc = set_read_filter(ixs[i], minV, maxV)) != MFX_OK) return rc;
  const size_t kw = ixs[0]->key_words();
  return index_ingest_multi(ixs, nix, n, side, [&](uint64_t o, uint64_t m, uint64_t *hk, uint32_t *hv) {
    par_memcpy((uint8_t *)hk, (const char *)(kmers + o * kw), m * 8 * kw);
    par_memcpy((uint8_t *)hv, (const char *)(values + o), m * 4);
    return true;
  });
}

// n bytes at file offset `off` into dst, read by several threads (each pread copies straight out of the page cache:
// no mapping to fault in page by page, which is what made the mmap + memcpy route top out at ~7 GB/s)
static unsigned pread_threads() {
  // these threads wait on memory, not on the ALUs: more of them than the CPU quota grants still pays (1 Gb ingest on
  // a 16-core quota: 1.9 s with 16 readers, 1.3 s with 32), unless MFX_HOST_THREADS fixes the count
  if (const char *pe = getenv("MFX_PREAD_THREADS")) if (atoi(pe) > 0) return std::min((unsigned)atoi(pe), 64u);   // (A/B)
  unsigned nt = std::max(1u, mfx_host_threads());
  if (!getenv("MFX_HOST_THREADS")) nt = std::max(nt, std::min(32u, std::max(1u, std::thread::hardware_concurrency())));
  return std::min(nt, 64u);
}

// pool: reader threads that live for the whole file (a database is read in ~100 chunks: starting and joining 32 threads for
// each was a third of the time of a chunk once the records shrank to 8 bytes); nullptr: threads of this call
static bool par_pread(int fd, uint8_t *dst, size_t n, uint64_t off, WorkerPool *pool = nullptr) {
  const unsigned nt = pool ? pool->W : pread_threads();
  auto rd = [fd](uint8_t *d, size_t len, uint64_t o) {
    while (len) {
      ssize_t r = pread(fd, d, len, (off_t)o);
      if (r <= 0) return false;
      d += r; o += (uint64_t)r; len -= (size_t)r;
    }
    return true;
  };
  if (n < (8u << 20) || nt == 1) return rd(dst, n, off);
  std::vector<char> good(nt, 1);
  const size_t per = ((n + nt - 1) / nt + 4095) & ~(size_t)4095;
  if (pool) {
    pool->start([&](unsigned t) {
      const size_t b = std::min(n, t * per), e = std::min(n, b + per);
      if (e > b) good[t] = rd(dst + b, e - b, off + b) ? 1 : 0;
    });
    pool->wait();
    for (char c : good) if (!c) return false;
    return true;
  }
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) {
    const size_t b = std::min(n, t * per), e = std::min(n, b + per);
    if (e > b) th.emplace_back([&, t, b, e]() { good[t] = rd(dst + b, e - b, off + b) ? 1 : 0; });
  }
  for (auto &x : th) x.join();
  for (char c : good) if (!c) return false;
  return true;
}

// k-mers [0, n) of an open flat-binary database: keys at keys_off (8 * key_words bytes each), counts at vals_off
int mfx_index_add_from_file(mfx_index *const *ixs, uint32_t nix, int fd, const char *path, uint64_t keys_off, uint64_t vals_off, uint64_t n,
                            int side, uint64_t minV, uint64_t maxV) {
  int rc = check_same_kind(ixs, nix, "mfx_index_add_from_file");
  if (rc) return rc;
  if (fd < 0) return mfx_fail(MFX_E_INVAL, "mfx_index_add_from_file: bad argument");
  if (side == 0) for (uint32_t i = 0; i < nix; ++i) if ((rc = set_read_filter(ixs[i], minV, maxV)) != MFX_OK) return rc;
  const size_t kw = ixs[0]->key_words();
  const bool packed = vals_off == 0;
  if (packed && kw != 1) return mfx_fail(MFX_E_INVAL, "mfx_index_add_from_file: packed records hold k-mers of k <= %d", MFX_MAX_K_PACKED);
  std::unique_ptr<WorkerPool> pool(n * 8 * kw >= (64u << 20) ? new WorkerPool(pread_threads(), true) : nullptr);
  return index_ingest_multi(ixs, nix, n, side, [&](uint64_t o, uint64_t m, uint64_t *hk, uint32_t *hv) {
    if (par_pread(fd, (uint8_t *)hk, m * 8 * kw, keys_off + o * 8 * kw, pool.get()) &&
        (packed || par_pread(fd, (uint8_t *)hv, m * 4, vals_off + o * 4, pool.get()))) return true;
    mfx_fail(MFX_E_IO, "reading '%s' failed", path);
    return false;
  }, packed);
}

// the delta-coded blocks of an open flat database (mfx_db.cpp FLAT_DELTA): dir = (nblocks + 1) x {first k-mer, file offset |
// kbits << 48 | vbits << 56}, n k-mers in all.  Whole blocks go through the lanes as they lie in the file -- 2.5-3 bytes
// per k-mer of a 30x read set -- and are decoded by the kernel that inserts them (mfx_table_add_delta_kernel).
int mfx_index_add_delta_file(mfx_index *const *ixs, uint32_t nix, int fd, const char *path, const uint64_t *dir, uint64_t nblocks, uint64_t n,
                             int side, uint64_t minV, uint64_t maxV, int placed) {
  int rc = check_same_kind(ixs, nix, "mfx_index_add_delta_file");
  if (rc) return rc;
  if (fd < 0 || !dir || ixs[0]->key_words() != 1) return mfx_fail(MFX_E_INVAL, "mfx_index_add_delta_file: bad argument");
  if (side == 0) for (uint32_t i = 0; i < nix; ++i) if ((rc = set_read_filter(ixs[i], minV, maxV)) != MFX_OK) return rc;
  auto off = [dir](uint64_t b) { return dir[2 * b + 1] & 0xffffffffffffull; };
  const uint64_t total = off(nblocks) - off(0);
  std::unique_ptr<WorkerPool> pool(total >= (64u << 20) ? new WorkerPool(pread_threads(), true) : nullptr);
  uint64_t b0 = 0;
  // lanes sized as for total / 8 records (32 MB at most: ~13 M k-mers a chunk): a chunk is a byte range of the file, not a k-mer count
  return index_ingest_chunks(ixs, nix, std::min<uint64_t>(std::max<uint64_t>(total / 8 + 1, 2 * MFX_DELTA_BLOCK * 11), 1ull << 22), [&](uint64_t cap, uint64_t *hk, uint32_t *hv, IngestChunk &d) {
    if (b0 >= nblocks) return 0;
    uint64_t b1 = b0 + 1;                                    // at least one block (a lane holds the largest possible block)
    while (b1 < nblocks && off(b1 + 1) - off(b0) <= cap * 8 && (b1 + 2 - b0) * 16 <= cap * 4) ++b1;
    const uint64_t bytes = off(b1) - off(b0), nb = b1 - b0;
    if (bytes > cap * 8 || (nb + 1) * 16 > cap * 4) { mfx_fail(MFX_E_FORMAT, "'%s': a block larger than the format allows", path); return -1; }
    if (!par_pread(fd, (uint8_t *)hk, bytes, off(b0), pool.get())) { mfx_fail(MFX_E_IO, "reading '%s' failed", path); return -1; }
    memcpy(hv, dir + 2 * b0, (nb + 1) * 16);
    const uint64_t base = off(b0), m = std::min<uint64_t>(n - b0 * MFX_DELTA_BLOCK, nb * MFX_DELTA_BLOCK);
    d.kbytes = bytes;
    d.vbytes = (nb + 1) * 16;
    d.launch = [nb, m, base, side, placed](mfx_index *ix, uint64_t *dk, uint32_t *dv, hipStream_t st) {
      return placed ? mfx_k_table_add_placed(ix->view(), dk, reinterpret_cast<const uint64_t *>(dv), (uint32_t)nb, m, base, side, ix->d_meta, st)
                    : mfx_k_table_add_delta(ix->view(), dk, reinterpret_cast<const uint64_t *>(dv), (uint32_t)nb, m, base, side, ix->d_meta, st);
    };
    b0 = b1;
    return 1;
  });
}

static int index_add(mfx_index *ix, const uint64_t *kmers, const uint32_t *values, uint64_t n, int side, int on_device) {
  if (!ix || (n && (!kmers || !values))) return mfx_fail(MFX_E_INVAL, "mfx_index_add: null argument");
  if (ix->reads_counted && ix->wide()) return mfx_reads_claim_error(ix, "mfx_index_add");
  DevGuard g(ix->device);
  const size_t kw = ix->key_words();                      // uint64 words per k-mer (2 for k > 31)
  auto table_add = [&](const uint64_t *dk, const uint32_t *dv, uint64_t m, hipStream_t s) {
    return ix->wide() ? mfx_kw_table_add(ix->view(), dk, dv, m, side, ix->d_meta, s) : mfx_k_table_add(ix->view(), dk, dv, m, side, ix->d_meta, s);
  };
  if (on_device) {
    ix->frozen = true;
    MFX_HIP(table_add(kmers, values, n, nullptr));
    MFX_HIP(hipDeviceSynchronize());
    return index_check(ix);
  }
  return index_ingest(ix, n, side, [&](uint64_t o, uint64_t m, uint64_t *hk, uint32_t *hv) {
    par_memcpy((uint8_t *)hk, (const char *)(kmers + o * kw), m * 8 * kw);
    par_memcpy((uint8_t *)hv, (const char *)(values + o), m * 4);
    return true;
  });
}

extern "C" int mfx_index_add_read(mfx_index *ix, const uint64_t *kmers, const uint32_t *values, uint64_t n,
                                  uint64_t minV, uint64_t maxV, int on_device) {
  if (!ix) return mfx_fail(MFX_E_INVAL, "mfx_index_add_read: null index");
  if (ix->reads_counted)
    return mfx_fail(MFX_E_INVAL, "mfx_index_add_read: the read side of this index was counted from reads (mfx_reads_begin); an index takes its "
                    "read counts from one source");
  if (ix->filter_set && (ix->minV != minV || ix->maxV != maxV))
    return mfx_fail(MFX_E_INVAL, "mfx_index_add_read: -min/-max must be the same for every batch of one index");
  ix->minV = minV;
  ix->maxV = maxV;
  ix->filter_set = true;
  return index_add(ix, kmers, values, n, 0, on_device);
}

extern "C" int mfx_index_add_asm(mfx_index *ix, const uint64_t *kmers, const uint32_t *values, uint64_t n, int on_device) {
  return index_add(ix, kmers, values, n, 1, on_device);
}

// defer: the kernel is launched and NOT waited for -- an event recorded behind it is left in the index's staging state
// (mfx_ingest::after), the inserts of the load that follows wait for it on the device, and that load's final check reads what
// both left in meta (mfx_index_build_for_hist)
// no_wait: the kernel is launched on `stream` and neither waited for nor checked -- the caller orders what follows behind it and checks
static int index_count(mfx_index *ix, const mfx_seq *seq, int count, void *stream, const char *who, bool defer = false, bool no_wait = false) {
  if (!ix || !seq) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (ix->device != seq->device) return mfx_fail(MFX_E_INVAL, "index and sequence live on different devices");
  if (ix->reads_counted && ix->wide()) return mfx_reads_claim_error(ix, who);
  if (ix->seq_only && ix->frozen && count != 2)
    return mfx_fail(MFX_E_INVAL, "%s: this sequence-only index already took counts; its k-mers must all be claimed before the first add / load "
                    "(a k-mer claimed now would have missed them)", who);
  if (count == 2 && (!ix->seq_only || ix->wide())) return mfx_fail(MFX_E_INVAL, "%s: counting claimed k-mers needs a sequence-only index (mfx_index_create_for_seq)", who);
  // the k <= 31 kernel reads the packed planes when the sequence has them (a packed upload never makes the bytes)
  if (seq->partial) return mfx_seq_partial_error(seq, who);
  const bool from_planes = !ix->wide() && (seq->planes_ok || seq->bases_stale) && !(getenv("MFX_COUNT_ASCII") && atoi(getenv("MFX_COUNT_ASCII")));
  if (!from_planes) if (int erc = mfx_seq_ensure_ascii(seq)) return erc;
  DevGuard g(ix->device);
  mfx_count_args a;
  a.t = ix->view();
  a.bases = seq->d_bases;
  if (from_planes) { a.codes = seq->d_codes; a.valid = seq->d_valid; }
  a.contig_off = seq->d_contig_off;
  a.contig_len = seq->d_contig_len;
  a.tile_start = seq->d_tile_start;
  a.ncontigs = seq->ncontigs;
  a.ntiles = seq->ntiles;
  a.meta = ix->d_meta;
  a.count = count;
  if (ix->seq_only && count != 2) {                            // what this table can answer for: the k-mers of THIS sequence
    uint32_t d = 0;
    if (int drc = mfx_seq_digest32(seq, &d)) return drc;
    // one sequence per sequence-only index: a second claim from ANOTHER sequence would leave the index bound to the last one and the
    // evaluation of the first refused ("holds the k-mers of another sequence") -- say so here, where the mistake is made
    if (ix->seq_digest != 0 && ix->seq_digest != d)
      return mfx_fail(MFX_E_INVAL, "%s: this sequence-only index already claimed the k-mers of another sequence (content digest %08x, this one %08x); "
                      "one such index answers for ONE sequence object -- put the contigs into one mfx_seq", who, ix->seq_digest, d);
    ix->seq_digest = d;
  }
  if (count == 2) ix->frozen = true;                           // counts arrived: no more claims
  MFX_HIP(ix->wide() ? mfx_kw_count(a, (hipStream_t)stream) : mfx_k_count(a, (hipStream_t)stream));
  if (no_wait) return MFX_OK;
  // While the kernel claims / counts a large sequence's k-mers (0.11 s for 3 Gb), the host pins the staging lanes the database
  // load that follows will want (0.06 s): the lanes belong to the index and are reused by every load.
  if (defer) {
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev, (hipStream_t)stream);
    mfx_ingest *g = e == hipSuccess ? ingest_get(ix, 1ull << 22) : nullptr;      // (pins the lanes while the kernel runs)
    if (g) {
      if (g->after) { (void)hipEventSynchronize(g->after); (void)hipEventDestroy(g->after); }
      g->after = ev;
      return MFX_OK;
    }
    if (ev) (void)hipEventDestroy(ev);
    (void)hipGetLastError();                                  // no staging state: fall through to the waited form
  } else if (ix->seq_only && seq->total_bases >= (256ull << 20)) (void)ingest_get(ix, 1ull << 22);
  MFX_HIP(hipStreamSynchronize((hipStream_t)stream));
  return index_check(ix);
}

// an event the inserts were to wait for is waited for here and dropped (error paths of mfx_index_build_for_hist)
static void ingest_settle_after(mfx_index *ix) {
  if (!ix || !ix->ingest || !ix->ingest->after) return;
  DevGuard g(ix->device);
  (void)hipEventSynchronize(ix->ingest->after);
  (void)hipEventDestroy(ix->ingest->after);
  ix->ingest->after = nullptr;
}

extern "C" int mfx_index_count_asm(mfx_index *ix, const mfx_seq *seq, void *stream) {
  return index_count(ix, seq, 1, stream, "mfx_index_count_asm");
}

// The assembly counts of the k-mers claimed BEFORE (mfx_index_claim_seq), taken from another -- usually larger -- sequence:
// asmV += 1 per occurrence of a claimed k-mer, nothing is claimed.  This is how a device that evaluates PART of an assembly
// (some contigs) gets value() right for its k-mers: they are claimed from its contigs and counted over the whole assembly
// (`meryl count` of -sequence counts every contig, merfin-globals.C:182-186), and the read database then updates them.
extern "C" int mfx_index_count_claimed(mfx_index *ix, const mfx_seq *seq, void *stream) {
  return index_count(ix, seq, 2, stream, "mfx_index_count_claimed");
}

// mfx_index_count_asm + mfx_index_load_db(side 0) as ONE call -- what `merfin -hist -sequence s -readmers db` needs
// (load_Kmers, merfin-globals.C:114-163 + the `meryl count` of -sequence, :182-186) -- with the database's bytes crossing
// PCIe while the sequence's k-mers are still being claimed and counted: the inserts wait for that kernel on the device,
// the transfers fill the staging ring meanwhile.  Same table as the two calls one after the other.
extern "C" int mfx_index_build_for_hist(mfx_index *ix, const mfx_seq *seq, const char *read_db_path, uint64_t minV, uint64_t maxV) {
  if (!ix || !seq || !read_db_path) return mfx_fail(MFX_E_INVAL, "mfx_index_build_for_hist: null argument");
  const char *ov = getenv("MFX_BUILD_OVERLAP");              // 0: the two calls one after the other (A/B, tests)
  const bool defer = !(ov && atoi(ov) == 0);
  int rc = index_count(ix, seq, 1, nullptr, "mfx_index_build_for_hist", defer);
  if (rc == MFX_OK) rc = mfx_index_load_db(ix, read_db_path, 0, minV, maxV);
  ingest_settle_after(ix);                                   // (a load that failed before its staging loop leaves the event behind)
  return rc;
}

// ---------------------------------------------------------------------------
// STAGED load of the read database (load_Kmers, merfin-globals.C:114-163, as `merfin -hist` pays it per run).  The database's bytes do
// not depend on anything else of the run, so they start moving when the process starts: mfx_db_stage_begin opens a delta-coded flat
// database, takes device memory for ALL of its blocks + directory, and a thread of its own reads the file through three pinned
// lanes into that memory (one copy stream) -- under the FASTA read, the sequence upload, the table's allocation and the kernel that
// claims and counts the sequence's k-mers.  mfx_index_build_for_hist_staged then launches that kernel and, behind it, the decode +
// update kernel over the staged blocks, chunk by chunk as their copies complete (the kernels wait for the copy events on the device).
// The link is busy from the first 0.1 s of the process instead of from the moment the table exists; same table as
// mfx_index_build_for_hist.  nullptr from _begin (another database form, too little free HBM): the caller takes the unstaged call.
// ---------------------------------------------------------------------------
struct mfx_db_stage {
  int device = 0, fd = -1;
  std::string path;
  mfx_flat_delta_info info;
  std::vector<uint64_t> dir;                                  // (nblocks + 1) x {first k-mer, file offset | kbits << 48 | vbits << 56}
  uint64_t off0 = 0, payload_bytes = 0;
  uint8_t *d_payload = nullptr;
  uint64_t *d_dir = nullptr;
  uint64_t *d_esc_k = nullptr;                                // the escape list (k-mers whose count did not fit their block's field), staged like the blocks
  uint32_t *d_esc_v = nullptr;
  hipEvent_t esc_copied = nullptr;
  std::atomic<int> esc_ready{0};                              // the escape copies are enqueued and esc_copied is recorded
  std::atomic<int> boost{0};                                  // 0: a few reader threads (the FASTA reader has the host); 1: all of them (mfx_db_stage_boost)
  struct Chunk { uint64_t b0, b1; hipEvent_t copied = nullptr; };
  std::vector<Chunk> chunks;
  std::atomic<int64_t> enqueued{0};                           // chunks whose copy is enqueued and whose event is recorded
  std::atomic<int> failed{0};
  std::string error;
  std::thread worker;
  double t_begin = 0, t_first_copy = 0, t_last_enqueued = 0, t_all_copied = 0;
  double t_setup[8] = {0, 0, 0, 0, 0, 0, 0, 0};              // begin: file + directory, memory info, device memory, events; worker: device + stream, first lane, first read, first enqueue
  double t_part[2][3] = {{0, 0, 0}, {0, 0, 0}};              // [before / after the boost][lane wait, file read, enqueue] seconds of the worker (diagnostics)
  uint64_t n_part[2] = {0, 0}, b_part[2] = {0, 0};
  uint64_t file_off(uint64_t b) const { return dir[2 * b + 1] & 0xffffffffffffull; }
};

static double stage_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static void stage_worker(mfx_db_stage *S) {
  constexpr int NLMAX = 8;
  int NL = 3;
  if (const char *le = getenv("MFX_DB_STAGE_LANES")) NL = std::min(NLMAX, std::max(2, atoi(le)));
  const size_t LANE = 32u << 20;
  uint8_t *lane[NLMAX] = {nullptr};
  hipEvent_t left[NLMAX] = {nullptr};
  hipStream_t cs = nullptr;
  bool busy[NLMAX] = {false};
  auto fail = [&](const char *what, hipError_t e) {
    S->error = std::string(what) + (e != hipSuccess ? std::string(": ") + hipGetErrorString(e) : std::string());
    S->failed.store(1);
  };
  double tw0 = stage_now();
  hipError_t e = hipSetDevice(S->device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
  S->t_setup[4] = stage_now() - tw0;
  // (a lane is pinned when its first chunk comes up -- 13 ms each -- and the directory goes over behind the first chunk: the first
  // bytes of the database are on the link as early as the runtime allows)
  auto lane_up = [&](int i) -> hipError_t {
    if (lane[i]) return hipSuccess;
    hipError_t le = hipHostMalloc((void **)&lane[i], LANE, hipHostMallocDefault);
    if (le == hipSuccess) le = hipEventCreateWithFlags(&left[i], hipEventDisableTiming);
    return le;
  };
  if (e != hipSuccess) fail("staging set-up failed", e);
  {
    // While the FASTA file is being read and encoded the host's threads are busy with that (a full pool here slowed the sequence
    // down by more than the database gained: profiles/r05_e2e_staged.txt); until the caller says the sequence is in
    // (mfx_db_stage_boost) a few readers keep the link fed, then all of them.
    unsigned few = 8;                                          // (2 / 4 / 8: 3 Gb wall 1.23-1.25 / 1.20-1.23 / 1.18-1.19 s spaced, profiles/r05_e2e_staged.txt)
    if (const char *fe = getenv("MFX_DB_STAGE_THREADS")) few = (unsigned)std::max(1, atoi(fe));
    std::unique_ptr<WorkerPool> pool_few(new WorkerPool(std::min(few, pread_threads()), true)), pool_all;
    auto pool_now = [&]() -> WorkerPool * {
      if (!S->boost.load(std::memory_order_relaxed)) return pool_few.get();
      if (!pool_all) pool_all.reset(new WorkerPool(pread_threads(), true));
      return pool_all.get();
    };
    for (size_t c = 0; c < S->chunks.size() && !S->failed.load(); ++c) {
      const int li = (int)(c % NL);
      const int ph = S->boost.load(std::memory_order_relaxed) ? 1 : 0;              // (diagnostics: before / after mfx_db_stage_boost)
      double tq = stage_now();
      if ((e = lane_up(li)) != hipSuccess) { fail("staging set-up failed", e); break; }
      if (c == 0) S->t_setup[5] = stage_now() - tq;
      if (busy[li] && (e = hipEventSynchronize(left[li])) != hipSuccess) { fail("staging copy failed", e); break; }
      const uint64_t o = S->file_off(S->chunks[c].b0), bytes = S->file_off(S->chunks[c].b1) - o;
      double tr = stage_now();
      S->t_part[ph][0] += tr - tq;
      if (!par_pread(S->fd, lane[li], bytes, o, pool_now())) { fail("reading the database failed", hipSuccess); break; }
      tq = stage_now();
      S->t_part[ph][1] += tq - tr;
      if (c == 0) S->t_setup[6] = tq - tr;
      S->n_part[ph] += 1;
      S->b_part[ph] += bytes;
      if (c == 0) S->t_first_copy = stage_now();
      e = hipMemcpyAsync(S->d_payload + (o - S->off0), lane[li], bytes, hipMemcpyHostToDevice, cs);
      if (e == hipSuccess && c == 0) e = hipMemcpyAsync(S->d_dir, S->dir.data(), S->dir.size() * 8, hipMemcpyHostToDevice, cs);     // (ahead of every chunk's `copied` event but the first's, which the next line records behind it)
      if (e == hipSuccess) e = hipEventRecord(left[li], cs);
      if (e == hipSuccess) e = hipEventRecord(S->chunks[c].copied, cs);
      if (e != hipSuccess) { fail("staging copy failed", e); break; }
      busy[li] = true;
      S->enqueued.store((int64_t)c + 1, std::memory_order_release);
      S->t_part[ph][2] += stage_now() - tq;
      if (c == 0) S->t_setup[7] = stage_now() - tq;
    }
    // the escape list behind the blocks: k-mers (8 bytes each), then their counts (4 bytes each)
    const uint64_t ne = S->info.n_escape;
    for (int part = 0; part < 2 && ne && !S->failed.load(); ++part) {
      const uint64_t width = part == 0 ? 8 : 4, total = ne * width, at = S->info.escapes_off + (part == 0 ? 0 : ne * 8);
      uint8_t *dst = part == 0 ? reinterpret_cast<uint8_t *>(S->d_esc_k) : reinterpret_cast<uint8_t *>(S->d_esc_v);
      for (uint64_t o = 0, c = S->chunks.size(); o < total && !S->failed.load(); o += LANE, ++c) {
        const int li = (int)(c % NL);
        const uint64_t bytes = std::min<uint64_t>(LANE, total - o);
        if ((e = lane_up(li)) != hipSuccess) { fail("staging set-up failed", e); break; }
        if (busy[li] && (e = hipEventSynchronize(left[li])) != hipSuccess) { fail("staging copy failed", e); break; }
        if (!par_pread(S->fd, lane[li], bytes, at + o, pool_now())) { fail("reading the database failed", hipSuccess); break; }
        if (part == 0) {                                      // a k-mer of k bases has no bit at or above 2k (a damaged file)
          const uint64_t *kk = reinterpret_cast<const uint64_t *>(lane[li]);
          bool wide = false;
          if (S->info.k < 32) for (uint64_t i = 0; i < bytes / 8; ++i) wide |= (kk[i] >> (2 * S->info.k)) != 0;
          if (wide) { fail("an escaped k-mer is wider than 2k bits", hipSuccess); break; }
        }
        e = hipMemcpyAsync(dst + o, lane[li], bytes, hipMemcpyHostToDevice, cs);
        if (e == hipSuccess) e = hipEventRecord(left[li], cs);
        if (e != hipSuccess) { fail("staging copy failed", e); break; }
        busy[li] = true;
      }
    }
    if (!S->failed.load()) {
      e = hipEventRecord(S->esc_copied, cs);
      if (e != hipSuccess) fail("staging copy failed", e);
      else S->esc_ready.store(1, std::memory_order_release);
    }
  }
  S->t_last_enqueued = stage_now();
  if (cs) (void)hipStreamSynchronize(cs);
  S->t_all_copied = stage_now();
  for (int i = 0; i < NL; ++i) { if (lane[i]) (void)hipHostFree(lane[i]); if (left[i]) (void)hipEventDestroy(left[i]); }
  if (cs) (void)hipStreamDestroy(cs);
}

extern "C" void mfx_db_stage_free(mfx_db_stage *S) {
  if (!S) return;
  S->failed.store(1);                                          // (a worker still on the file stops at its next chunk)
  if (S->worker.joinable()) S->worker.join();
  DevGuard g(S->device);
  for (auto &c : S->chunks) if (c.copied) (void)hipEventDestroy(c.copied);
  if (S->d_payload) (void)hipFree(S->d_payload);
  if (S->d_dir) (void)hipFree(S->d_dir);
  if (S->d_esc_k) (void)hipFree(S->d_esc_k);
  if (S->d_esc_v) (void)hipFree(S->d_esc_v);
  if (S->esc_copied) (void)hipEventDestroy(S->esc_copied);
  if (S->fd >= 0) close(S->fd);
  delete S;
}

// the sequence is read and uploaded: the stager may use every reader thread from here on
extern "C" void mfx_db_stage_boost(mfx_db_stage *S) {
  if (S) S->boost.store(1, std::memory_order_relaxed);
}

extern "C" mfx_db_stage *mfx_db_stage_begin(const char *path, int device) {
  if (!path) { mfx_fail(MFX_E_INVAL, "mfx_db_stage_begin: null argument"); return nullptr; }
  if (device < 0 || device >= mfx_device_count()) { mfx_fail(MFX_E_NODEVICE, "mfx_db_stage_begin: HIP device %d not available (%d visible)", device, mfx_device_count()); return nullptr; }
  if (const char *e = getenv("MFX_DB_STAGE")) if (atoi(e) == 0) { mfx_fail(MFX_E_INVAL, "staged load disabled (MFX_DB_STAGE=0)"); return nullptr; }
  std::unique_ptr<mfx_db_stage> S(new mfx_db_stage);
  S->t_begin = stage_now();
  S->device = device;
  S->path = path;
  if (mfx_flat_delta_open(path, &S->fd, &S->info, S->dir)) return nullptr;
  S->t_setup[0] = stage_now() - S->t_begin;
  auto drop = [&](mfx_db_stage *x) { mfx_db_stage_free(x); return (mfx_db_stage *)nullptr; };
  if (S->info.n == 0 || S->info.k > MFX_MAX_K_NARROW) { mfx_fail(MFX_E_INVAL, "'%s': nothing to stage", path); return drop(S.release()); }
  S->off0 = S->file_off(0);
  S->payload_bytes = S->file_off(S->info.nblocks) - S->off0;
  DevGuard g(device);
  if (!g.ok) { mfx_fail(MFX_E_HIP, "hipSetDevice(%d) failed", device); return drop(S.release()); }
  size_t free_b = 0, total_b = 0;
  double tq = stage_now();
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); mfx_fail(MFX_E_HIP, "hipMemGetInfo failed"); return drop(S.release()); }
  S->t_setup[1] = stage_now() - tq; tq = stage_now();
  // a fifth of the free HBM at most: the table is sized by what is left (a read database beyond that goes through the ring)
  if ((double)(S->payload_bytes + S->dir.size() * 8 + S->info.n_escape * 12) > 0.2 * (double)free_b) {
    mfx_fail(MFX_E_NOMEM, "'%s': %.1f GB of blocks against %.1f GB of free device memory: not staged", path, S->payload_bytes / 1e9, free_b / 1e9);
    return drop(S.release());
  }
  if (hipMalloc((void **)&S->d_payload, S->payload_bytes + 64) != hipSuccess || hipMalloc((void **)&S->d_dir, S->dir.size() * 8) != hipSuccess ||
      hipEventCreateWithFlags(&S->esc_copied, hipEventDisableTiming) != hipSuccess ||
      (S->info.n_escape && (hipMalloc((void **)&S->d_esc_k, S->info.n_escape * 8) != hipSuccess || hipMalloc((void **)&S->d_esc_v, S->info.n_escape * 4) != hipSuccess))) {
    (void)hipGetLastError();
    mfx_fail(MFX_E_NOMEM, "'%s': no device memory for the staged database", path);
    return drop(S.release());
  }
  S->t_setup[2] = stage_now() - tq; tq = stage_now();
  // chunks: whole blocks, at most 32 MB of file each
  const uint64_t LANE = 32u << 20;
  for (uint64_t b0 = 0; b0 < S->info.nblocks;) {
    uint64_t b1 = b0 + 1;
    while (b1 < S->info.nblocks && S->file_off(b1 + 1) - S->file_off(b0) <= LANE) ++b1;
    if (S->file_off(b1) - S->file_off(b0) > LANE) { mfx_fail(MFX_E_FORMAT, "'%s': a block larger than the format allows", path); return drop(S.release()); }
    mfx_db_stage::Chunk c;
    c.b0 = b0; c.b1 = b1;
    if (hipEventCreateWithFlags(&c.copied, hipEventDisableTiming) != hipSuccess) { mfx_fail(MFX_E_HIP, "event creation failed"); return drop(S.release()); }
    S->chunks.push_back(c);
    b0 = b1;
  }
  S->t_setup[3] = stage_now() - tq;
  mfx_db_stage *raw = S.release();
  raw->worker = std::thread(stage_worker, raw);
  return raw;
}

// seq != nullptr: the claim / count kernel of the sequence first (mfx_index_build_for_hist_staged); nullptr: the staged database alone, into side
// `side` of a table whose k-mers are there or claimed already (mfx_index_load_db_staged)
static int staged_load(mfx_index *ix, const mfx_seq *seq, mfx_db_stage *S, int side, uint64_t minV, uint64_t maxV, const char *who) {
  if (ix->device != S->device) return mfx_fail(MFX_E_INVAL, "%s: index and staged database live on different devices", who);
  if (S->info.k != ix->k) return mfx_fail(MFX_E_INVAL, "'%s' holds %d-mers but the index is built for k=%d", S->path.c_str(), S->info.k, ix->k);
  if (ix->wide()) return mfx_fail(MFX_E_INVAL, "%s: k <= 31 only", who);
  const bool timing = getenv("MFX_INGEST_TIMING") != nullptr;
  const double t0 = stage_now();
  int rc = side == 0 ? set_read_filter(ix, minV, maxV) : MFX_OK;
  if (rc) return rc;
  DevGuard g(ix->device);
  hipStream_t is[MFX_INGEST_STREAMS] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t counted = nullptr;
  auto release = [&]() {
    for (auto &st : is) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (counted) (void)hipEventDestroy(counted);
  };
#define STAGED_HIP(call)                                                                                          \
  do {                                                                                                            \
    hipError_t e_ = (call);                                                                                       \
    if (e_ != hipSuccess) { rc = mfx_fail(MFX_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); release(); return rc; } \
  } while (0)
  for (auto &st : is) STAGED_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  STAGED_HIP(hipEventCreateWithFlags(&counted, hipEventDisableTiming));
  // the claim / count kernel on the first insert stream; every insert stream waits for it
  if (seq) {
    rc = index_count(ix, seq, 1, is[0], who, false, /*no_wait=*/true);
    if (rc) { release(); return rc; }
    STAGED_HIP(hipEventRecord(counted, is[0]));
    for (int i = 1; i < MFX_INGEST_STREAMS; ++i) STAGED_HIP(hipStreamWaitEvent(is[i], counted, 0));
  }
  ix->frozen = true;
  const double t1 = stage_now();
  double t_wait = 0;
  for (size_t c = 0; c < S->chunks.size(); ++c) {
    const double tw = stage_now();
    while (S->enqueued.load(std::memory_order_acquire) <= (int64_t)c) {
      if (S->failed.load()) { release(); return mfx_fail(MFX_E_IO, "'%s': %s", S->path.c_str(), S->error.c_str()); }
      std::this_thread::sleep_for(std::chrono::microseconds(50));     // (not a yield spin: under a CPU quota it would hold a core against the stager's readers)
    }
    t_wait += stage_now() - tw;
    const mfx_db_stage::Chunk &ch = S->chunks[c];
    hipStream_t st = is[c % MFX_INGEST_STREAMS];
    STAGED_HIP(hipStreamWaitEvent(st, ch.copied, 0));
    const uint64_t nb = ch.b1 - ch.b0, m = std::min<uint64_t>(S->info.n - ch.b0 * MFX_DELTA_BLOCK, nb * MFX_DELTA_BLOCK);
    STAGED_HIP(S->info.placed ? mfx_k_table_add_placed(ix->view(), reinterpret_cast<const uint64_t *>(S->d_payload), S->d_dir + 2 * ch.b0, (uint32_t)nb, m, S->off0, side, ix->d_meta, st)
                              : mfx_k_table_add_delta(ix->view(), reinterpret_cast<const uint64_t *>(S->d_payload), S->d_dir + 2 * ch.b0, (uint32_t)nb, m, S->off0, side, ix->d_meta, st));
  }
  // the escapes, from the staged copy: an ordinary update of (k-mer, count) arrays that are already on the device
  while (!S->esc_ready.load(std::memory_order_acquire)) {
    if (S->failed.load()) { release(); return mfx_fail(MFX_E_IO, "'%s': %s", S->path.c_str(), S->error.c_str()); }
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
  if (S->info.n_escape) {
    STAGED_HIP(hipStreamWaitEvent(is[0], S->esc_copied, 0));
    STAGED_HIP(mfx_k_table_add(ix->view(), S->d_esc_k, S->d_esc_v, S->info.n_escape, side, ix->d_meta, is[0]));
  }
  const double t2 = stage_now();
  for (auto &st : is) STAGED_HIP(hipStreamSynchronize(st));
#undef STAGED_HIP
  const double t3 = stage_now();
  release();
  if (S->failed.load()) return mfx_fail(MFX_E_IO, "'%s': %s", S->path.c_str(), S->error.c_str());
  rc = index_check(ix);
  if (timing)
    fprintf(stderr, "-- staged build: %.3f s = count launched %.3f + %zu update launches + escapes %.3f (of which waiting for the stager %.3f) + drain %.3f + check %.3f; "
            "stager: first copy %.3f s after its start, last copy enqueued after %.3f s (%.2f GB); the build began %.3f s after the stager\n",
            stage_now() - t0, t1 - t0, S->chunks.size(), t2 - t1, t_wait, t3 - t2, stage_now() - t3, S->t_first_copy - S->t_begin, S->t_last_enqueued - S->t_begin,
            S->payload_bytes / 1e9, t0 - S->t_begin);
  if (timing)
    fprintf(stderr, "-- stager set-up: begin = file + directory %.3f, memory info %.3f, device memory %.3f, events %.3f; worker = device + stream %.3f, first lane %.3f, first read %.3f, "
            "first enqueue %.3f s\n", S->t_setup[0], S->t_setup[1], S->t_setup[2], S->t_setup[3], S->t_setup[4], S->t_setup[5], S->t_setup[6], S->t_setup[7]);
  if (timing)
    for (int ph = 0; ph < 2; ++ph)
      fprintf(stderr, "-- stager %s the sequence was in: %lu chunks, %.2f GB; the worker waited for a lane %.3f s, read the file %.3f s (%.1f GB/s), enqueued copies %.3f s\n",
              ph ? "after" : "before", (unsigned long)S->n_part[ph], S->b_part[ph] / 1e9, S->t_part[ph][0], S->t_part[ph][1],
              S->t_part[ph][1] > 0 ? S->b_part[ph] / 1e9 / S->t_part[ph][1] : 0.0, S->t_part[ph][2]);
  return rc;
}

extern "C" int mfx_index_build_for_hist_staged(mfx_index *ix, const mfx_seq *seq, mfx_db_stage *S, uint64_t minV, uint64_t maxV) {
  if (!ix || !seq || !S) return mfx_fail(MFX_E_INVAL, "mfx_index_build_for_hist_staged: null argument");
  return staged_load(ix, seq, S, 0, minV, maxV, "mfx_index_build_for_hist_staged");
}
// mfx_index_load_db of a STAGED database: its bytes have been on their way into device memory since mfx_db_stage_begin; only the decode +
// insert kernels are left (side 0: -readmers with the -min/-max filter, 1: -seqmers).  Same table as mfx_index_load_db.
extern "C" int mfx_index_load_db_staged(mfx_index *ix, mfx_db_stage *S, int side, uint64_t minV, uint64_t maxV) {
  if (!ix || !S || (side != 0 && side != 1)) return mfx_fail(MFX_E_INVAL, "mfx_index_load_db_staged: null argument or side not 0 / 1");
  return staged_load(ix, nullptr, S, side, minV, maxV, "mfx_index_load_db_staged");
}

// P (mfx_place.h) of n k-mers -- canonicalised first --: on_device != 0: both arrays are device pointers on `device` (tools that sort a
// database on the GPU); else host arrays, host threads
extern "C" int mfx_db_place_keys(int k, const uint64_t *kmers, uint64_t n, uint64_t *out, int on_device, int device) {
  if (n && (!kmers || !out)) return mfx_fail(MFX_E_INVAL, "mfx_db_place_keys: null argument");
  if (k < MFX_PLACE_MIN_K || k > MFX_PLACE_MAX_K || mfx_p_split(k))      // (k = 31: P takes 65 bits; its placed database is made by mfx_db_convert_placed)
    return mfx_fail(MFX_E_INVAL, "mfx_db_place_keys: %d <= k <= 30 (k = %d)", MFX_PLACE_MIN_K, k);
  if (!on_device) { mfx_place_keys_host(k, kmers, n, out); return MFX_OK; }
  DevGuard g(device);
  MFX_HIP(mfx_k_place_keys(k, kmers, n, out, nullptr));
  MFX_HIP(hipStreamSynchronize(nullptr));
  return MFX_OK;
}

extern "C" int mfx_index_claim_seq(mfx_index *ix, const mfx_seq *seq, void *stream) {
  if (ix && !ix->seq_only) return mfx_fail(MFX_E_INVAL, "mfx_index_claim_seq: not a sequence-only index (mfx_index_create_for_seq)");
  return index_count(ix, seq, 0, stream, "mfx_index_claim_seq");
}

extern "C" int mfx_index_value(const mfx_index *ix, const uint64_t *kmers, uint64_t n, uint32_t *readV, uint32_t *asmV) {
  if (!ix || (n && (!kmers || !readV || !asmV))) return mfx_fail(MFX_E_INVAL, "mfx_index_value: null argument");
  DevGuard g(ix->device);
  DevBuf<uint64_t> dk;
  DevBuf<uint32_t> dr, da;
  MFX_HIP(dk.alloc(n * ix->key_words()));
  MFX_HIP(dr.alloc(n));
  MFX_HIP(da.alloc(n));
  MFX_HIP(hipMemcpy(dk.p, kmers, n * ix->key_words() * sizeof(uint64_t), hipMemcpyHostToDevice));
  MFX_HIP(ix->wide() ? mfx_kw_table_value(ix->view(), dk.p, n, dr.p, da.p, nullptr) : mfx_k_table_value(ix->view(), dk.p, n, dr.p, da.p, nullptr));
  MFX_HIP(hipMemcpy(readV, dr.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  MFX_HIP(hipMemcpy(asmV, da.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return MFX_OK;
}

extern "C" int mfx_index_get_info(const mfx_index *ix, mfx_index_info *out) {
  if (!ix || !out) return mfx_fail(MFX_E_INVAL, "mfx_index_get_info: null argument");
  DevGuard g(ix->device);
  uint64_t meta[4];
  MFX_HIP(hipMemcpy(meta, ix->d_meta, sizeof(meta), hipMemcpyDeviceToHost));
  out->k = ix->k;
  out->canonical = (meta[1] == 0) ? 1 : 0;
  out->capacity = ix->nlines * ix->slots_per_line();
  out->distinct = meta[0];
  out->bytes = ix->total_lines() * MFX_ALIGN;
  out->seq_only = ix->seq_only ? 1 : 0;
  out->compact = ix->compact ? 1 : 0;
  out->dropped = meta[3];
  return MFX_OK;
}

extern "C" int mfx_index_export(const mfx_index *ix, uint64_t *kmers, uint32_t *readV, uint32_t *asmV, uint64_t *n_out) {
  if (!ix || !kmers || !readV || !asmV || !n_out) return mfx_fail(MFX_E_INVAL, "mfx_index_export: null argument");
  DevGuard g(ix->device);
  mfx_index_info info;
  int rc = mfx_index_get_info(ix, &info);
  if (rc) return rc;
  DevBuf<uint64_t> dk;
  DevBuf<uint32_t> dr, da;
  DevBuf<unsigned long long> dc;
  MFX_HIP(dk.alloc(info.distinct * ix->key_words()));
  MFX_HIP(dr.alloc(info.distinct));
  MFX_HIP(da.alloc(info.distinct));
  MFX_HIP(dc.alloc(1));
  MFX_HIP(mfx_memset_now(dc.p, 0, sizeof(unsigned long long)));
  MFX_HIP(ix->wide() ? mfx_kw_table_export(ix->view(), dk.p, dr.p, da.p, dc.p, nullptr) : mfx_k_table_export(ix->view(), dk.p, dr.p, da.p, dc.p, nullptr));
  unsigned long long cnt = 0;
  MFX_HIP(hipMemcpy(&cnt, dc.p, sizeof(cnt), hipMemcpyDeviceToHost));
  MFX_HIP(hipMemcpy(kmers, dk.p, cnt * ix->key_words() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  MFX_HIP(hipMemcpy(readV, dr.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
  MFX_HIP(hipMemcpy(asmV, da.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
  *n_out = cnt;
  return MFX_OK;
}
