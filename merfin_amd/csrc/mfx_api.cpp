// mfx_api.cpp -- C-ABI entry points of libmerfin_amd (include/merfin_amd.h).
// Host-side orchestration only; all evaluation work is done by the HIP
// kernels in mfx_kernels.hip.  There is deliberately NO CPU fallback: without
// a usable HIP device every entry point fails with MFX_E_NODEVICE / MFX_E_HIP.
#include "mfx_host.h"
#include "mfx_histsum.h"
#include "mfx_kernels.h"
#include "mfx_pipe.h"
#include "mfx_pool.h"

#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
static thread_local int  g_err_code = 0;

void mfx_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int mfx_fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  g_err_code = code;
  return code;
}

extern "C" const char *mfx_last_error(void) { return g_err; }
extern "C" int mfx_last_error_code(void) { return g_err_code; }
extern "C" const char *mfx_version(void) { return "merfin_amd 0.2 (gfx950)"; }

// Diagnostic (no reference counterpart): random 128-byte lines per second this device's HBM delivers to independent
// 16-byte loads over a table of `table_bytes` (allocated and released here) -- the roof of the index probe on THIS box.
extern "C" int mfx_diag_gather_rate(int device, uint64_t table_bytes, double *lines_per_s) {
  if (!lines_per_s || table_bytes < (1ull << 20)) return mfx_fail(MFX_E_INVAL, "mfx_diag_gather_rate: bad argument");
  if (device < 0 || device >= mfx_device_count()) return mfx_fail(MFX_E_NODEVICE, "HIP device %d not available", device);
  int prev = -1;
  (void)hipGetDevice(&prev);
  MFX_HIP(hipSetDevice(device));
  void *t = nullptr;
  uint64_t *scratch = nullptr;
  hipError_t e = hipMalloc(&t, table_bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&scratch, 8);
  if (e == hipSuccess) e = mfx_memset_now(t, 0x5a, table_bytes);
  if (e == hipSuccess) e = mfx_k_gather_rate(t, table_bytes / MFX_ALIGN, scratch, lines_per_s, nullptr);
  if (t) (void)hipFree(t);
  if (scratch) (void)hipFree(scratch);
  if (prev >= 0) (void)hipSetDevice(prev);
  if (e != hipSuccess) { (void)hipGetLastError(); return mfx_fail(e == hipErrorOutOfMemory ? MFX_E_NOMEM : MFX_E_HIP, "mfx_diag_gather_rate: %s", hipGetErrorString(e)); }
  return MFX_OK;
}

extern "C" int mfx_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes) {
  if (device < 0 || device >= mfx_device_count()) return mfx_fail(MFX_E_NODEVICE, "HIP device %d not available", device);
  int prev = -1;
  (void)hipGetDevice(&prev);
  MFX_HIP(hipSetDevice(device));
  size_t f = 0, t = 0;
  const hipError_t e = hipMemGetInfo(&f, &t);
  if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
  if (e != hipSuccess) return mfx_fail(MFX_E_HIP, "hipMemGetInfo failed: %s", hipGetErrorString(e));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return MFX_OK;
}

extern "C" int mfx_device_warm(int device) {
  if (device < 0 || device >= mfx_device_count()) return mfx_fail(MFX_E_NODEVICE, "HIP device %d not available", device);
  int prev = -1;
  (void)hipGetDevice(&prev);
  MFX_HIP(hipSetDevice(device));
  // a device allocation + memset (the runtime's own kernels), one kernel of this library (its code object), a pinned
  // allocation and a stream: everything the first upload would otherwise bring up on the caller's time
  void *d = nullptr, *h = nullptr;
  hipStream_t st = nullptr;
  const bool timing = getenv("MFX_UPLOAD_TIMING") != nullptr;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double tw[8] = {now(), 0, 0, 0, 0, 0, 0, 0};
  hipError_t e = hipMalloc(&d, 1 << 20);
  tw[1] = now();
  if (e == hipSuccess) e = mfx_memset_now(d, 0, 1 << 20);
  tw[2] = now();
  if (e == hipSuccess) e = mfx_k_table_init(reinterpret_cast<mfx_slot *>(d), (1 << 20) / sizeof(mfx_slot), nullptr);
  tw[3] = now();
  if (e == hipSuccess) e = hipHostMalloc(&h, 1 << 20, hipHostMallocDefault);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  tw[4] = now();
  if (e == hipSuccess) e = hipMemcpyAsync(d, h, 1 << 20, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  tw[5] = now();
  // (no device-wide wait here: another thread's stream -- the database's stager -- may be busy for the whole run)
  if (st) (void)hipStreamDestroy(st);
  if (h) (void)hipHostFree(h);
  if (d) (void)hipFree(d);
  tw[6] = now();
  if (timing)
    fprintf(stderr, "-- device warm: %.3f s = first allocation %.3f + fill %.3f + first kernel of the library %.3f + pinned memory and a stream %.3f + a copy %.3f + release %.3f\n",
            tw[6] - tw[0], tw[1] - tw[0], tw[2] - tw[1], tw[3] - tw[2], tw[4] - tw[3], tw[5] - tw[4], tw[6] - tw[5]);
  if (prev >= 0) (void)hipSetDevice(prev);
  if (e != hipSuccess) { (void)hipGetLastError(); return mfx_fail(MFX_E_HIP, "mfx_device_warm: %s", hipGetErrorString(e)); }
  return MFX_OK;
}

extern "C" int mfx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ---------------------------------------------------------------------------
// evaluator
// ---------------------------------------------------------------------------
extern "C" mfx_eval *mfx_eval_create(const mfx_index *ix, const mfx_kparams *kp, uint32_t nbins) {
  if (!ix || !kp || (kp->n_prob && (!kp->probK || !kp->probP))) {
    mfx_fail(MFX_E_INVAL, "mfx_eval_create: null argument");
    return nullptr;
  }
  DevGuard g(ix->device);
  mfx_eval *ev = new mfx_eval;
  ev->ix = ix;
  ev->device = ix->device;
  ev->peak = kp->peak;
  ev->n_prob = kp->n_prob;
  ev->probK.assign(kp->probK, kp->probK + kp->n_prob);
  ev->probP.assign(kp->probP, kp->probP + kp->n_prob);
  ev->nbins = nbins ? std::max<uint32_t>(nbins, MFX_NB_LDS) : 65536;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, ix->device) != hipSuccess) {
    mfx_fail(MFX_E_HIP, "hipGetDeviceProperties failed");
    delete ev;
    return nullptr;
  }
  const char *e = getenv("MFX_BLOCKS_PER_CU");
  int bpc = e ? atoi(e) : mfx_k_hist_resident_blocks(ix->compact ? 1 : 0, ix->k);   // persistent blocks: as many as are resident at once
  if (bpc < 1) bpc = 1;
  ev->grid = prop.multiProcessorCount * bpc;
  size_t np = ev->n_prob ? ev->n_prob : 1;
  if (hipMalloc((void **)&ev->d_probK, np * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc((void **)&ev->d_probP, np * sizeof(double)) != hipSuccess ||
      hipMalloc((void **)&ev->d_partials, 2 * (size_t)ev->grid * sizeof(double)) != hipSuccess ||
      hipMalloc((void **)&ev->d_tile_ctr, 2 * sizeof(uint64_t)) != hipSuccess ||
      mfx_memset_now(ev->d_tile_ctr, 0, 2 * sizeof(uint64_t)) != hipSuccess ||
      hipMalloc((void **)&ev->d_ovf, MFX_OVF_WORDS * sizeof(uint64_t)) != hipSuccess ||
      hipMemsetAsync(ev->d_ovf + 2 + MFX_OVF_SLOTS, 0xff, (size_t)MFX_OVF_SLOTS * sizeof(uint64_t), nullptr) != hipSuccess ||      // keys: all ones = empty
      mfx_memset_now(ev->d_ovf, 0, (2 + (size_t)MFX_OVF_SLOTS) * sizeof(uint64_t)) != hipSuccess ||
      (ev->n_prob && hipMemcpy(ev->d_probK, ev->probK.data(), ev->n_prob * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) ||
      (ev->n_prob && hipMemcpy(ev->d_probP, ev->probP.data(), ev->n_prob * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)) {
    mfx_fail(MFX_E_HIP, "mfx_eval_create: device setup failed: %s", hipGetErrorString(hipGetLastError()));
    mfx_eval_free(ev);
    return nullptr;
  }
  // (1 - readK/asmK) * prob of every (read count < MFX_MAXP_LDS, asmV < MFX_KLUT) pair the kernel's exact tables cover, as the integer
  // the tile-driven kernel adds up (mfx_kfix): the same fp64 routines the kernel's generic path runs (mfx_kstar.h, no contraction)
  {
    std::vector<uint64_t> uq((size_t)MFX_MAXP_LDS * MFX_KLUT, 0);
    for (uint32_t rv = 0; rv < MFX_MAXP_LDS; ++rv) {
      double rk, pr;
      mfx_getK_core(ev->peak, ev->n_prob, ev->probK.data(), ev->probP.data(), rv, rk, pr);
      if (!(rk >= 1.0 && rk < (double)MFX_KLUT && rk == (double)(uint32_t)rk)) continue;
      for (uint32_t av = 1; av < MFX_KLUT; ++av)
        if ((double)av > rk) uq[(size_t)rv * MFX_KLUT + av] = mfx_kfix(mfx_overcopy_term(rk, (double)av, pr));
    }
    if (hipMalloc((void **)&ev->d_underq, uq.size() * sizeof(uint64_t)) != hipSuccess ||
        hipMemcpy(ev->d_underq, uq.data(), uq.size() * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) {
      mfx_fail(MFX_E_HIP, "mfx_eval_create: device setup failed: %s", hipGetErrorString(hipGetLastError()));
      mfx_eval_free(ev);
      return nullptr;
    }
  }
  return ev;
}

extern "C" void mfx_eval_free(mfx_eval *ev) {
  if (!ev) return;
  DevGuard g(ev->device);
  if (ev->d_probK) (void)hipFree(ev->d_probK);
  if (ev->d_probP) (void)hipFree(ev->d_probP);
  if (ev->d_underq) (void)hipFree(ev->d_underq);
  if (ev->d_partials) (void)hipFree(ev->d_partials);
  if (ev->d_tile_ctr) (void)hipFree(ev->d_tile_ctr);
  if (ev->d_tile_partials) (void)hipFree(ev->d_tile_partials);
  for (auto &w : ev->d_wl) if (w) (void)hipFree(w);
  if (ev->d_ovf) (void)hipFree(ev->d_ovf);
  if (ev->d_dbg) (void)hipFree(ev->d_dbg);
  for (auto &p : ev->h_stage) if (p) (void)hipHostFree(p);
  for (auto &p : ev->h_pack) if (p) (void)hipHostFree(p);
  delete ev->pool;
  if (ev->d_var_scratch) (void)hipFree(ev->d_var_scratch);
  if (ev->sr.d_counts) (void)hipFree(ev->sr.d_counts);
  if (ev->sr.d_kover) (void)hipFree(ev->sr.d_kover);
  if (ev->sr.h_img) (void)hipHostFree(ev->sr.h_img);
  for (auto &e : ev->sr.up) if (e) (void)hipEventDestroy(e);
  if (ev->sr.kdone) (void)hipEventDestroy(ev->sr.kdone);
  for (auto &x : ev->sr.d_exc) if (x) (void)hipFree(x);
  if (ev->sr.copy) (void)hipStreamDestroy(ev->sr.copy);
  for (auto &k : ev->sr.kern) if (k) (void)hipStreamDestroy(k);
  delete ev;
}

extern "C" uint32_t mfx_eval_nbins(const mfx_eval *ev) { return ev ? ev->nbins : 0; }

// Test hook: from now on -hist launches of this evaluator run the DEBUG instance of the kernel where one exists (the compact
// layout's specialised k = 21 kernel: same code with four counters in its probe) -- never what bench.py measures.
extern "C" int mfx_eval_debug_enable(mfx_eval *ev, int on) {
  if (!ev) return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_enable: null argument");
  DevGuard g(ev->device);
  if (on && !ev->d_dbg) {
    MFX_HIP(hipMalloc((void **)&ev->d_dbg, 8 * sizeof(uint64_t)));
    MFX_HIP(mfx_memset_now(ev->d_dbg, 0, 8 * sizeof(uint64_t)));
  } else if (!on && ev->d_dbg) {
    MFX_HIP(hipDeviceSynchronize());
    (void)hipFree(ev->d_dbg);
    ev->d_dbg = nullptr;
  }
  return MFX_OK;
}

// out[0] queries that were not in their first mini-bucket (first cooperative pass), [1] home line full of other k-mers (second
// cooperative pass), [2] a saturated count (side table), [3] per-lane whole-line scans; the counters are read and cleared
extern "C" int mfx_eval_debug_counters(mfx_eval *ev, uint64_t *out8) {
  if (!ev || !out8) return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_counters: null argument");
  if (!ev->d_dbg) return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_counters: not enabled (mfx_eval_debug_enable)");
  DevGuard g(ev->device);
  MFX_HIP(hipDeviceSynchronize());
  MFX_HIP(hipMemcpy(out8, ev->d_dbg, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  MFX_HIP(mfx_memset_now(ev->d_dbg, 0, 8 * sizeof(uint64_t)));
  return MFX_OK;
}

extern "C" void mfx_getK(const mfx_kparams *kp, uint32_t readV, uint32_t asmV, double *readK, double *asmK, double *prob) {
  double rk, pr;
  mfx_getK_core(kp->peak, kp->n_prob, kp->probK, kp->probP, readV, rk, pr);
  *readK = rk;
  *asmK = (double)asmV;   // merfin-globals.C:81
  *prob = pr;
}

extern "C" double mfx_getKmetric(double readK, double asmK) { return mfx_kmetric(readK, asmK); }

// merfin-histogram.C:22-31
extern "C" double mfx_histoQV(double kval, double ktot, int k) {
  double base = kval / ktot;
  double kinv = 1.0 / k;
  double qv = -10.0 * log10(1.0 - pow(1.0 - base, kinv));
  return qv;
}

// ---------------------------------------------------------------------------
// -hist
// ---------------------------------------------------------------------------
int index_canonical(const mfx_index *ix, int *canon) {
  uint64_t meta[4];
  MFX_HIP(hipMemcpy(meta, ix->d_meta, sizeof(meta), hipMemcpyDeviceToHost));
  // single probe of min(f,r) equals value(f)+value(r) for a canonical DB: the other strand is not in it (SURVEY A-7);
  // for even k the kernels count a palindromic k-mer's slot twice.  A database with non-canonical k-mers: both strands.
  *canon = meta[1] == 0 ? 1 : 0;
  return MFX_OK;
}

// the canonical/odd-k decision costs a blocking D2H read; evaluators cache it per index version so
// that mfx_hist_launch stays asynchronous (it is called once per step in the multi-GPU loop)
static int eval_canonical(mfx_eval *ev, int *canon) {
  if (ev->canon_version != ev->ix->version) {
    int rc = index_canonical(ev->ix, &ev->canon);
    if (rc) return rc;
    ev->canon_version = ev->ix->version;
  }
  *canon = ev->canon;
  return MFX_OK;
}

int ensure_tile_partials(mfx_eval *ev, uint64_t ntiles) {
  const uint64_t need = mfx_k_tile_partials_words(ntiles);
  if (need > ev->tile_partials_cap) {
    if (ev->d_tile_partials) (void)hipFree(ev->d_tile_partials);
    ev->d_tile_partials = nullptr;
    ev->tile_partials_cap = 0;
    MFX_HIP(hipMalloc((void **)&ev->d_tile_partials, need * sizeof(double)));
    ev->tile_partials_cap = need;
  }
  return MFX_OK;
}

// The worklist of a launch over ntl tiles (mfx_hist_rest_kernel): room for one position in 32 -- a genome with human-like repeat
// families lists 1-2 % of its positions (profiles/r06_repeats_ab.txt); a launch that lists more ends the rest per lane, as every
// launch did before round 6.  0.5 bytes per position of the largest launch so far.
static int ensure_worklist(mfx_eval *ev, int slot, uint64_t ntl) {
  const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(1u << 16, ntl * MFX_TILE / 32), 0xffffffffull);
  if (ev->d_wl[slot] && ev->wl_cap[slot] >= want) return MFX_OK;
  if (ev->d_wl[slot]) { MFX_HIP(hipDeviceSynchronize()); (void)hipFree(ev->d_wl[slot]); ev->d_wl[slot] = nullptr; ev->wl_cap[slot] = 0; }
  if (hipMalloc((void **)&ev->d_wl[slot], (MFX_WL_HEADER + 2 * want) * sizeof(uint64_t)) != hipSuccess) {
    (void)hipGetLastError();                                  // no memory for a list: the launches scan per lane
    ev->d_wl[slot] = nullptr;
    return MFX_OK;
  }
  MFX_HIP(mfx_memset_now(ev->d_wl[slot], 0, MFX_WL_HEADER * sizeof(uint64_t)));
  ev->wl_cap[slot] = want;
  return MFX_OK;
}

// part_n == 1: tiles [tile_begin, tile_end); part_n > 1: the block-cyclic share of part_rank over ALL tiles.
// chunk_of_total == 0: a complete evaluation -- the koverCpy values of its (tile, wave)s are summed into *d_kover.
// chunk_of_total  > 0: one chunk of a streamed evaluation over `chunk_of_total` tiles in all: the values land at
// their tile's place in ev->d_tile_partials (sized by the caller) and are summed ONCE after the last chunk, so
// koverCpy is bit-identical to a single launch over the whole range, however the upload was cut.
int hist_launch(mfx_eval *ev, const mfx_seq *seq, uint64_t tile_begin, uint64_t tile_end, uint32_t part_rank, uint32_t part_n,
                uint32_t part_shift, uint64_t *d_counts, double *d_kover, void *stream, uint64_t chunk_of_total, int ctr_slot, uint64_t partials_tile0) {
  uint64_t ntl = tile_end - tile_begin;
  if (part_n > 1) {
    const uint64_t blk = 1ull << part_shift, nblk = (seq->ntiles + blk - 1) / blk;
    ntl = 0;
    for (uint64_t b = part_rank; b < nblk; b += part_n) ntl += std::min<uint64_t>(blk, seq->ntiles - b * blk);
  }
  if (ntl == 0) return MFX_OK;
  DevGuard g(ev->device);
  int canon = 0;
  int rc = eval_canonical(ev, &canon);
  if (rc) return rc;
  if (!chunk_of_total) {                                     // (a streamed run checks once its upload is complete)
    if (seq->partial) return mfx_seq_partial_error(seq, "-hist");
    rc = mfx_check_seq_of_index(ev->ix, seq, "-hist");
    if (rc) return rc;
  }
  const char *force = getenv("MFX_FORCE_TWO_STRAND");
  if (force && atoi(force)) canon = 0;
  if (!chunk_of_total) {
    rc = ensure_tile_partials(ev, ntl);
    if (rc) return rc;
  }
  if (seq->bases_stale && ev->ix->wide()) {                 // the 128-bit kernels read one byte per base
    rc = mfx_seq_ensure_ascii(seq);
    if (rc) return rc;
  }
  if (!(seq->planes_ok || seq->bases_stale) && !seq->d_bases) {   // (a sequence nothing was put into: every byte 0)
    rc = mfx_seq_ensure_ascii(seq);
    if (rc) return rc;
  }
  mfx_hist_args a;
  a.t = ev->ix->view();
  a.canonical = canon;
  a.bases = seq->d_bases;
  if (seq->planes_ok || seq->bases_stale) { a.codes = seq->d_codes; a.valid = seq->d_valid; }      // packed planes present: the tiles are copied, not encoded
  a.contig_off = seq->d_contig_off;
  a.contig_len = seq->d_contig_len;
  a.tile_start = seq->d_tile_start;
  a.ncontigs = seq->ncontigs;
  a.tile_begin = tile_begin;
  a.tile_end = tile_end;
  a.tile_contig = seq->d_tile_contig;
  a.tile_ctr = ev->d_tile_ctr + ctr_slot;
  a.tile_partials = ev->d_tile_partials + (chunk_of_total ? (tile_begin - partials_tile0) * (MFX_BLOCK / 64) : 0);   // partials_tile0: first tile of a streamed PART
  a.n_logical = ntl;
  a.part_rank = part_rank;
  a.part_n = part_n;
  a.part_shift = part_shift;
  a.ks.peak = ev->peak;
  a.ks.n_prob = ev->n_prob;
  a.ks.probK = ev->d_probK;
  a.ks.probP = ev->d_probP;
  a.ks.underq = ev->d_underq;
  a.ks.nbins = ev->nbins;
  a.ks.ncontigs = seq->ncontigs;
  a.ks.counts = d_counts;
  a.ks.partials = ev->d_partials;
  a.ks.ovf = ev->d_ovf;
  a.dbg = ev->d_dbg;
  // MFX_HIST_WORKLIST=0 (read per launch, as MFX_FORCE_TWO_STRAND above) or the test hook's mode 0: no list, every wave ends its own rare endings
  const char *wl_env = getenv("MFX_HIST_WORKLIST");
  const bool wl_off = (wl_env && atoi(wl_env) == 0) || ev->dbg_wl_mode == 0;
  ev->wl_used_segs[ctr_slot] = ev->wl_used_segcap[ctr_slot] = 0;
  if (a.t.compact && canon && ntl < (1ull << 27) && !wl_off) {   // the probe's rare endings are listed and ended by mfx_hist_rest_kernel (mfx_kernels.hip)
    // (a streamed run's chunks grow to 128 MB of bases: its lists are made for that size at its first chunk, not re-made as they grow)
    rc = ensure_worklist(ev, ctr_slot, chunk_of_total ? std::max<uint64_t>(ntl, std::min<uint64_t>(chunk_of_total, (128ull << 20) / MFX_TILE)) : ntl);
    if (rc) return rc;
    const uint64_t segs = std::min<uint64_t>((uint64_t)ev->grid, ntl);     // the main kernel's grid: one segment per block
    if (ev->d_wl[ctr_slot] && segs <= MFX_WL_HEADER - 2) {
      a.wl = ev->d_wl[ctr_slot];
      a.wl_segs = (uint32_t)segs;
      a.wl_segcap = (uint32_t)(ev->wl_cap[ctr_slot] / segs);
      if (ev->dbg_wl_mode == 2) a.wl_segcap = std::min(a.wl_segcap, ev->dbg_wl_segcap);       // (test hook: fuller segments of the same allocation)
      ev->wl_used_segs[ctr_slot] = a.wl_segs;
      ev->wl_used_segcap[ctr_slot] = a.wl_segcap;
    }
  }
  MFX_HIP(ev->ix->wide() ? mfx_kw_hist(a, (int)std::min<uint64_t>((uint64_t)ev->grid, ntl), (hipStream_t)stream)
                          : mfx_k_hist(a, (int)std::min<uint64_t>((uint64_t)ev->grid, ntl), (hipStream_t)stream));
  if (a.wl) MFX_HIP(mfx_k_hist_rest(a, (int)(a.wl_segs * 4u), (hipStream_t)stream));                 // (MFX_REST_SPLIT blocks per segment)
  if (chunk_of_total) MFX_HIP(hipMemsetAsync(ev->d_tile_ctr + ctr_slot, 0, sizeof(uint64_t), (hipStream_t)stream));   // re-arm the tile scheduler
  else MFX_HIP(mfx_k_sum_tile_partials(ev->d_tile_partials, ntl, d_kover, ev->d_tile_ctr, (hipStream_t)stream, ev->ix->wide() ? 0 : 1));
  return MFX_OK;
}

extern "C" int mfx_hist_launch(mfx_eval *ev, const mfx_seq *seq, uint64_t tile_begin, uint64_t tile_end,
                               uint64_t *d_counts, double *d_kover, void *stream) {
  if (!ev || !seq || !d_counts || !d_kover) return mfx_fail(MFX_E_INVAL, "mfx_hist_launch: null argument");
  if (ev->device != seq->device) return mfx_fail(MFX_E_INVAL, "evaluator and sequence live on different devices");
  if (tile_begin > tile_end || tile_end > seq->ntiles) return mfx_fail(MFX_E_INVAL, "tile range [%lu,%lu) outside [0,%lu)",
                                                                      (unsigned long)tile_begin, (unsigned long)tile_end, (unsigned long)seq->ntiles);
  return hist_launch(ev, seq, tile_begin, tile_end, 0, 1, 0, d_counts, d_kover, stream);
}

extern "C" int mfx_hist_launch_cyclic(mfx_eval *ev, const mfx_seq *seq, uint32_t rank, uint32_t nranks, uint32_t block_tiles,
                                      uint64_t *d_counts, double *d_kover, void *stream) {
  if (!ev || !seq || !d_counts || !d_kover) return mfx_fail(MFX_E_INVAL, "mfx_hist_launch_cyclic: null argument");
  if (ev->device != seq->device) return mfx_fail(MFX_E_INVAL, "evaluator and sequence live on different devices");
  if (nranks == 0 || rank >= nranks || block_tiles == 0 || (block_tiles & (block_tiles - 1)))
    return mfx_fail(MFX_E_INVAL, "mfx_hist_launch_cyclic: rank %u of %u, block of %u tiles (a power of two)", rank, nranks, block_tiles);
  uint32_t shift = 0;
  while ((1u << shift) < block_tiles) ++shift;
  if (nranks == 1) return hist_launch(ev, seq, 0, seq->ntiles, 0, 1, 0, d_counts, d_kover, stream);
  return hist_launch(ev, seq, 0, seq->ntiles, rank, nranks, shift, d_counts, d_kover, stream);
}

// The evaluator's table of far K* bins emptied for the next launches, asynchronously on `st`: what an earlier launch left there
// and nobody collected is not the next run's.  16 MB of fills: ~10 us of device time.
hipError_t ovf_reset_hip(mfx_eval *ev, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(ev->d_ovf, 0, (2 + (size_t)MFX_OVF_SLOTS) * sizeof(uint64_t), st);
  return e != hipSuccess ? e : hipMemsetAsync(ev->d_ovf + 2 + MFX_OVF_SLOTS, 0xff, (size_t)MFX_OVF_SLOTS * sizeof(uint64_t), st);
}
int mfx_ovf_reset_async(mfx_eval *ev, hipStream_t st) {
  MFX_HIP(ovf_reset_hip(ev, st));
  return MFX_OK;
}

// the table's occupied slots as {key, occurrences} pairs in `pairs` (room for 2 * n words); the table is emptied.  Synchronises `st`.
int mfx_ovf_collect(mfx_eval *ev, uint64_t *header2, std::vector<uint64_t> *pairs, hipStream_t st) {
  uint64_t hd[2] = {0, 0};
  MFX_HIP(hipMemcpyAsync(hd, ev->d_ovf, sizeof(hd), hipMemcpyDeviceToHost, st));
  MFX_HIP(hipStreamSynchronize(st));
  if (header2) { header2[0] = hd[0]; header2[1] = hd[1]; }
  if (pairs) pairs->clear();
  if (hd[0] == 0 && hd[1] == 0) return MFX_OK;
  if (pairs && hd[0]) {
    // rare: the whole table comes over (16 MB) and is scanned here
    std::vector<uint64_t> tab(2 * (size_t)MFX_OVF_SLOTS);
    MFX_HIP(hipMemcpyAsync(tab.data(), ev->d_ovf + 2, tab.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    pairs->reserve(2 * hd[0]);
    for (size_t i = 0; i < MFX_OVF_SLOTS; ++i)
      if (tab[MFX_OVF_SLOTS + i] != ~0ull) { pairs->push_back(tab[MFX_OVF_SLOTS + i]); pairs->push_back(tab[i]); }
    std::vector<std::pair<uint64_t, uint64_t>> srt(pairs->size() / 2);          // by key: the same list whatever the races of the inserts were
    for (size_t i = 0; i < srt.size(); ++i) srt[i] = {(*pairs)[2 * i], (*pairs)[2 * i + 1]};
    std::sort(srt.begin(), srt.end());
    for (size_t i = 0; i < srt.size(); ++i) { (*pairs)[2 * i] = srt[i].first; (*pairs)[2 * i + 1] = srt[i].second; }
  }
  if (int rc = mfx_ovf_reset_async(ev, st)) return rc;
  MFX_HIP(hipStreamSynchronize(st));
  if (hd[1])
    return mfx_fail(MFX_E_OVERFLOW, "%lu k-mers fell into more distinct K* bins beyond the %u dense ones than the evaluator's table of far bins "
                    "holds (%u); create the evaluator with a larger nbins", (unsigned long)hd[1], ev->nbins, MFX_OVF_SLOTS);
  return MFX_OK;
}

extern "C" int mfx_hist_take_overflow(mfx_eval *ev, uint64_t *records, uint64_t cap, uint64_t *n_out) {
  if (!ev || !n_out) return mfx_fail(MFX_E_INVAL, "mfx_hist_take_overflow: null argument");
  DevGuard g(ev->device);
  std::vector<uint64_t> pairs;
  uint64_t hd[2];
  int rc = mfx_ovf_collect(ev, hd, &pairs, nullptr);
  *n_out = pairs.size() / 2;
  if (rc) return rc;
  const uint64_t m = std::min<uint64_t>(pairs.size() / 2, cap);
  if (m && records) memcpy(records, pairs.data(), 2 * m * sizeof(uint64_t));
  return (pairs.size() / 2 > cap) ? mfx_fail(MFX_E_OVERFLOW, "%lu distinct far K* bins, caller buffer holds %lu", (unsigned long)(pairs.size() / 2), (unsigned long)cap) : MFX_OK;
}

// The reference's arrays grow in steps of 1024 under a uint32 bound (increaseArray(..., histOverMax, 1024),
// merfin-histogram.C:74,87,116,121): a bin index above 2^32 - 1025 overflows that bound there (undefined behaviour);
// here it is an error, as is running out of host memory (an index of 4e9 is 34 GB of bins, there as here).
static int result_grow(uint64_t *&a, uint32_t &max, uint64_t need) {
  if (need <= max) return MFX_OK;
  const uint64_t nm = (need + 1023) / 1024 * 1024;
  if (nm > 0xffffffffull)
    return mfx_fail(MFX_E_INVAL, "K* histogram bin %lu is beyond the 32-bit array bound of merfin's histogram (merfin-histogram.C:74,87)",
                    (unsigned long)(need - 1));
  uint64_t *b = (uint64_t *)realloc(a, nm * sizeof(uint64_t));
  if (!b) return mfx_fail(MFX_E_NOMEM, "no host memory for %lu K* histogram bins", (unsigned long)nm);
  a = b;
  memset(a + max, 0, (nm - max) * sizeof(uint64_t));
  max = (uint32_t)nm;
  return MFX_OK;
}

extern "C" int mfx_hist_result_from_counts(uint32_t nbins, const uint64_t *h, double kover, uint32_t ncontigs,
                                           mfx_hist_result *out) {
  if (!nbins || !h || !out) return mfx_fail(MFX_E_INVAL, "mfx_hist_result_from_counts: null argument");
  memset(out, 0, sizeof(*out));
  const uint32_t nb = nbins;
  uint32_t um = 0, om = 0;
  for (uint32_t i = 0; i < nb; ++i) {
    if (h[i]) um = i + 1;
    if (h[nb + i]) om = i + 1;
  }
  // merfin-histogram.C:105-108: the global arrays start at 2048 entries
  if (result_grow(out->undr, out->undrMax, std::max<uint32_t>(um, 2048)) || result_grow(out->over, out->overMax, std::max<uint32_t>(om, 2048))) {
    free(out->undr);
    free(out->over);
    memset(out, 0, sizeof(*out));
    return mfx_last_error_code();
  }
  memcpy(out->undr, h, um * sizeof(uint64_t));
  memcpy(out->over, h + nb, om * sizeof(uint64_t));
  out->kasm = h[mfx_histsum::kasm(nb)];
  out->kmissing = h[mfx_histsum::kmissing(nb)];
  out->koverCpy = kover;
  out->ncontigs = ncontigs;
  out->contig_kasm = (uint64_t *)calloc(ncontigs ? ncontigs : 1, sizeof(uint64_t));
  out->contig_kmissing = (uint64_t *)calloc(ncontigs ? ncontigs : 1, sizeof(uint64_t));
  memcpy(out->contig_kasm, h + mfx_histsum::contig_kasm(nb), ncontigs * sizeof(uint64_t));
  memcpy(out->contig_kmissing, h + mfx_histsum::contig_kmissing(nb, ncontigs), ncontigs * sizeof(uint64_t));
  return MFX_OK;
}

// rec: {key, occurrences} pairs (mfx_hist_take_overflow's format)
static int result_add_overflow(mfx_hist_result *r, const std::vector<uint64_t> &rec) {
  uint64_t mu = 0, mo = 0;                                   // grow once, to the largest index of the batch
  for (size_t i = 0; i + 1 < rec.size(); i += 2) {
    const uint64_t x = rec[i], idx = x & ~(1ull << 63);
    if (x >> 63) mo = std::max(mo, idx + 1); else mu = std::max(mu, idx + 1);
  }
  if (int rc = result_grow(r->over, r->overMax, mo)) return rc;
  if (int rc = result_grow(r->undr, r->undrMax, mu)) return rc;
  for (size_t i = 0; i + 1 < rec.size(); i += 2) {
    const uint64_t x = rec[i], idx = x & ~(1ull << 63);
    if (x >> 63) r->over[idx] += rec[i + 1]; else r->undr[idx] += rec[i + 1];
  }
  return MFX_OK;
}

extern "C" int mfx_hist_result_add_overflow(mfx_hist_result *r, const uint64_t *records, uint64_t n) {
  if (!r || !r->undr || !r->over || (n && !records)) return mfx_fail(MFX_E_INVAL, "mfx_hist_result_add_overflow: null argument");
  return result_add_overflow(r, std::vector<uint64_t>(records, records + 2 * n));
}

// What a whole-assembly run needs besides the evaluator's tables -- a stream, the counts image, its pinned mirror -- belongs
// to the evaluator and is made once (mfx_eval::sr): creating and releasing it per call costs ~2.5 ms, which is most of an
// 8-device evaluation (4 ms of kernel per device at 3 Gb).  The device of `ev` must be current.
int eval_run_resources(mfx_eval *ev, size_t words) {
  auto &R = ev->sr;
  if (R.words < words) {
    if (R.d_counts) (void)hipFree(R.d_counts);
    if (R.h_img) (void)hipHostFree(R.h_img);
    R.d_counts = nullptr; R.h_img = nullptr; R.words = 0;
    MFX_HIP(hipMalloc((void **)&R.d_counts, words * sizeof(uint64_t)));
    MFX_HIP(hipHostMalloc((void **)&R.h_img, (words + 2) * sizeof(uint64_t), hipHostMallocDefault));
    R.words = words;
  }
  if (!R.d_kover) MFX_HIP(hipMalloc((void **)&R.d_kover, 2 * sizeof(double)));          // ([1]: hist_run_streamed_packed's digest word)
  for (auto &k : R.kern) if (!k) MFX_HIP(hipStreamCreateWithFlags(&k, hipStreamNonBlocking));
  return MFX_OK;
}

// clears + launch (contiguous tiles, or the block-cyclic share part_rank of part_n) + D2H of image and koverCpy, all
// asynchronous on the evaluator's own stream; the caller synchronises ev->sr.kern[0] and reads ev->sr.h_img
int eval_run_enqueue(mfx_eval *ev, const mfx_seq *seq, uint32_t part_rank, uint32_t part_n) {
  const size_t words = MFX_HIST_WORDS(ev->nbins, seq->ncontigs);
  int rc = eval_run_resources(ev, words);
  if (rc) return rc;
  auto &R = ev->sr;
  hipStream_t st = R.kern[0];
  MFX_HIP(hipMemsetAsync(R.d_counts, 0, words * sizeof(uint64_t), st));
  MFX_HIP(hipMemsetAsync(R.d_kover, 0, sizeof(double), st));
  if (int rc0 = mfx_ovf_reset_async(ev, st)) return rc0;             // far bins nobody collected from an earlier launch are not this run's
  rc = part_n > 1 ? mfx_hist_launch_cyclic(ev, seq, part_rank, part_n, 256, R.d_counts, R.d_kover, st)
                  : mfx_hist_launch(ev, seq, 0, seq->ntiles, R.d_counts, R.d_kover, st);
  if (rc) return rc;
  MFX_HIP(hipMemcpyAsync(R.h_img, R.d_counts, words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MFX_HIP(hipMemcpyAsync(R.h_img + words, R.d_kover, sizeof(double), hipMemcpyDeviceToHost, st));
  return MFX_OK;
}

extern "C" int mfx_hist_run(mfx_eval *ev, const mfx_seq *seq, mfx_hist_result *out) {
  if (!ev || !seq || !out) return mfx_fail(MFX_E_INVAL, "mfx_hist_run: null argument");
  if (ev->device != seq->device) return mfx_fail(MFX_E_INVAL, "evaluator and sequence live on different devices");
  DevGuard g(ev->device);
  const size_t words = MFX_HIST_WORDS(ev->nbins, seq->ncontigs);
  int rc = eval_run_enqueue(ev, seq, 0, 1);
  if (rc) return rc;
  MFX_HIP(hipStreamSynchronize(ev->sr.kern[0]));
  double kover = 0;
  memcpy(&kover, ev->sr.h_img + words, sizeof(double));
  const uint64_t novf = ev->sr.h_img[mfx_histsum::novf(ev->nbins)];
  rc = mfx_hist_result_from_counts(ev->nbins, ev->sr.h_img, kover, seq->ncontigs, out);
  if (rc) return rc;
  rc = result_take_overflow(ev, novf, out);
  if (rc) mfx_hist_result_free(out);
  return rc;
}

// fold the overflow list of `ev` (K* bins >= nbins) into a result
int result_take_overflow(mfx_eval *ev, uint64_t novf, mfx_hist_result *out) {
  if (!novf) return MFX_OK;
  std::vector<uint64_t> pairs;
  if (int rc = mfx_ovf_collect(ev, nullptr, &pairs, nullptr)) return rc;
  return result_add_overflow(out, pairs);
}

extern "C" void mfx_hist_result_free(mfx_hist_result *r) {
  if (!r) return;
  free(r->undr); free(r->over); free(r->contig_kasm); free(r->contig_kmissing);
  memset(r, 0, sizeof(*r));
}

// reportHistogram, merfin-histogram.C:140-176
extern "C" int mfx_hist_report(const mfx_hist_result *r, int k, const char *hist_path, const char *summary_path) {
  if (!r || !r->undr || !r->over) return mfx_fail(MFX_E_INVAL, "mfx_hist_report: empty result");
  if (hist_path) {
    mfx_file fh = mfx_open_writer(hist_path, false);     // compressedFileWriter: compressor chosen by suffix (mfx_pipe.h)
    FILE *f = fh.f;
    if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", hist_path);
    for (uint64_t ii = r->undrMax - 1; ii > 0; ii--)
      if (r->undr[ii] > 0)
        fprintf(f, "%.1f\t%lu\n", ((double)ii * -0.2), (unsigned long)r->undr[ii]);
    fprintf(f, "%.1f\t%lu\n", 0.0, (unsigned long)(r->undr[0] + r->over[0]));
    for (uint64_t ii = 1; ii < r->overMax; ii++)
      if (r->over[ii] > 0)
        fprintf(f, "%.1f\t%lu\n", ((double)ii * 0.2), (unsigned long)r->over[ii]);
    if (mfx_close(fh)) return mfx_fail(MFX_E_IO, "writing '%s' failed (stream error or the compressor exited with an error)", hist_path);
  }
  if (summary_path) {
    FILE *f = strcmp(summary_path, "-") == 0 ? stderr : fopen(summary_path, "w");
    if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", summary_path);
    fprintf(f, "\n");
    fprintf(f, "K-mers not found in reads (missing) : %lu\n", (unsigned long)r->kmissing);
    fprintf(f, "K-mers overly represented in assembly: %.2f\n", r->koverCpy);
    fprintf(f, "K-mers found in the assembly: %lu\n", (unsigned long)r->kasm);
    fprintf(f, "Missing QV: %.2f\n", mfx_histoQV((double)r->kmissing, (double)r->kasm, k));
    fprintf(f, "Merfin QV*: %.2f\n", mfx_histoQV(r->kmissing + r->koverCpy, (double)r->kasm, k));
    fprintf(f, "*** Note this QV is valid only if -seqmer was generated with -sequence ***\n\n");
    fprintf(f, "*** Missing QV only considers missing kmers as errors. Merfin QV* includes overrepresented kmers. ***\n\n");
    fprintf(f, "*** When the lookup table is provided, missing QV includes weighted low frequency kmers, otherwise it is identical to Merqury QV. ***\n\n");
    if (f != stderr) fclose(f);
  }
  return MFX_OK;
}

// ---------------------------------------------------------------------------
// -track: K* per fixed window of every contig, reduced on the device (mfx_track_kernel; csrc/mfx_track.h).  The evaluation is
// -dump's (merfin-dump.C:44-67); the records replace the -dump text + awk + wigToBigWig route of the reference README,
// "Assess collapses and duplications".
// ---------------------------------------------------------------------------
static_assert(sizeof(mfx_track_window) == 72 && offsetof(mfx_track_window, sum_readK) == 24 && offsetof(mfx_track_window, min_kstar) == 56,
              "mfx_track_window: the kernels address the record as 9 words");

extern "C" uint64_t mfx_track_num_windows(const mfx_seq *seq, uint64_t window) {
  if (!seq || window == 0) return 0;
  uint64_t n = 0;
  for (uint32_t c = 0; c < seq->ncontigs; ++c) n += seq->len[c] / window + (seq->len[c] % window ? 1 : 0);
  return n;
}

extern "C" int mfx_track_run(mfx_eval *ev, const mfx_seq *seq, uint64_t window, mfx_track_window *out, uint64_t cap, uint64_t *n_out,
                             uint64_t *kasm, uint64_t *kmissing) {
  if (!ev || !seq || !n_out) return mfx_fail(MFX_E_INVAL, "mfx_track_run: null argument");
  if (window == 0) return mfx_fail(MFX_E_INVAL, "mfx_track_run: the window must hold at least one position");
  if (ev->device != seq->device) return mfx_fail(MFX_E_INVAL, "evaluator and sequence live on different devices");
  if (ev->ix->shard_n > 1)
    return mfx_fail(MFX_E_INVAL, "mfx_track_run: the index is shard %u of %u: a window's records need every k-mer's counts; use a whole index",
                    ev->ix->shard_rank, ev->ix->shard_n);
  if (seq->partial) return mfx_seq_partial_error(seq, "-track");
  const uint64_t nrec = mfx_track_num_windows(seq, window);
  if (nrec > cap || (nrec && !out)) return mfx_fail(MFX_E_INVAL, "mfx_track_run: %lu windows, room for %lu", (unsigned long)nrec, (unsigned long)cap);
  uint64_t longest = 0;
  for (uint32_t c = 0; c < seq->ncontigs; ++c) longest = std::max(longest, seq->len[c]);
  if (std::min(longest, window) > 0xffffffffull)
    return mfx_fail(MFX_E_INVAL, "mfx_track_run: a window of more than 2^32 - 1 positions of one contig: its counters are 32 bits wide");
  DevGuard g(ev->device);
  int canon = 0;
  int rc = index_canonical(ev->ix, &canon);
  if (rc) return rc;
  if ((rc = mfx_check_seq_of_index(ev->ix, seq, "-track")) != MFX_OK) return rc;
  *n_out = nrec;
  if (kasm) *kasm = 0;
  if (kmissing) *kmissing = 0;
  if (nrec == 0) return MFX_OK;
  const bool planes = !ev->ix->wide() && (seq->planes_ok || seq->bases_stale);       // (the 128-bit kernel reads one byte per base)
  if (!planes && (rc = mfx_seq_ensure_ascii(seq)) != MFX_OK) return rc;
  const size_t bytes = (size_t)nrec * sizeof(mfx_track_window);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes > free_b)
    return mfx_fail(MFX_E_NOMEM, "mfx_track_run: %lu windows of %lu positions take %.2f GB on the device, %.2f GB are free; use a longer window",
                    (unsigned long)nrec, (unsigned long)window, (double)bytes / 1e9, (double)free_b / 1e9);
  DevBuf<uint64_t> drec, dfirst, dst;
  if (drec.alloc(nrec * 9) != hipSuccess) {
    (void)hipGetLastError();
    return mfx_fail(MFX_E_NOMEM, "mfx_track_run: no device memory for %lu windows (%.2f GB); use a longer window", (unsigned long)nrec, (double)bytes / 1e9);
  }
  std::vector<uint64_t> first(seq->ncontigs ? seq->ncontigs : 1, 0);
  {
    uint64_t r = 0;
    for (uint32_t c = 0; c < seq->ncontigs; ++c) { first[c] = r; r += seq->len[c] / window + (seq->len[c] % window ? 1 : 0); }
  }
  MFX_HIP(dfirst.alloc(first.size()));
  MFX_HIP(dst.alloc(2));
  MFX_HIP(hipMemcpy(dfirst.p, first.data(), first.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  MFX_HIP(mfx_memset_now(dst.p, 0, 2 * sizeof(uint64_t)));
  MFX_HIP(mfx_memset_now(drec.p, 0, bytes));
  mfx_track_args a;
  a.t = ev->ix->view();
  a.canonical = canon;
  a.bases = seq->d_bases;
  if (planes) { a.codes = seq->d_codes; a.valid = seq->d_valid; }
  a.contig_off = seq->d_contig_off;
  a.contig_len = seq->d_contig_len;
  a.tile_start = seq->d_tile_start;
  a.tile_contig = seq->d_tile_contig;
  a.contig_rec = dfirst.p;
  a.ntiles = seq->ntiles;
  a.window = window;
  a.peak = ev->peak;
  a.n_prob = ev->n_prob;
  a.probK = ev->d_probK;
  a.probP = ev->d_probP;
  a.recs = drec.p;
  a.stats = dst.p;
  MFX_HIP(ev->ix->wide() ? mfx_kw_track(a, nullptr) : mfx_k_track(a, nullptr));
  MFX_HIP(mfx_k_track_finish(drec.p, nrec, nullptr));
  MFX_HIP(hipMemcpy(out, drec.p, bytes, hipMemcpyDeviceToHost));
  uint64_t st[2];
  MFX_HIP(hipMemcpy(st, dst.p, sizeof(st), hipMemcpyDeviceToHost));
  if (kasm) *kasm = st[0];
  if (kmissing) *kmissing = st[1];
  return MFX_OK;
}

// mean K* of a window: the nearest double to the exact sum (an integer of 2^-52 units), over the number of scored k-mers
static double track_mean(const mfx_track_window &w) {
  const __int128 s = (__int128)(((unsigned __int128)(uint64_t)w.sum_kstar_hi << 64) | (unsigned __int128)w.sum_kstar_lo);
  return ldexp((double)s, -52) / (double)w.n_scored;
}

extern "C" int mfx_track_write(const mfx_track_window *w, uint64_t n, const mfx_seq *seq, const char *const *names, uint64_t window,
                               const char *tsv_path, const char *bedgraph_path) {
  if (!seq || (!w && n) || !names || window == 0) return mfx_fail(MFX_E_INVAL, "mfx_track_write: null argument or no window length");
  if (n != mfx_track_num_windows(seq, window))
    return mfx_fail(MFX_E_INVAL, "mfx_track_write: %lu records, the sequences have %lu windows of %lu positions", (unsigned long)n,
                    (unsigned long)mfx_track_num_windows(seq, window), (unsigned long)window);
  for (int what = 0; what < 2; ++what) {
    const char *path = what == 0 ? tsv_path : bedgraph_path;
    if (!path) continue;
    mfx_file fh = mfx_open_writer(path, false);             // compressedFileWriter: compressor chosen by suffix (mfx_pipe.h)
    FILE *f = fh.f;
    if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", path);
    if (what == 0) fprintf(f, "#name\tstart\tend\tn_kmers\tn_missing\tn_scored\tn_pos\tn_neg\tsum_readK\tsum_asmK\tmean_kstar\tmin_kstar\tmax_kstar\n");
    else fprintf(f, "track type=bedGraph name=\"K*\"\n");
    uint64_t i = 0;
    for (uint32_t c = 0; c < seq->ncontigs; ++c) {
      const uint64_t len = seq->len[c];
      for (uint64_t start = 0; start < len; start += window, ++i) {
        const mfx_track_window &r = w[i];
        const uint64_t end = std::min(start + window, len);
        if (what == 0) {
          if (r.n_kmers == 0) continue;
          fprintf(f, "%s\t%lu\t%lu\t%u\t%u\t%u\t%u\t%u\t%lu\t%lu\t%.6f\t%.6f\t%.6f\n", names[c], (unsigned long)start, (unsigned long)end, r.n_kmers,
                  r.n_missing, r.n_scored, r.n_pos, r.n_neg, (unsigned long)r.sum_readK, (unsigned long)r.sum_asmK,
                  r.n_scored ? track_mean(r) : 0.0, r.min_kstar, r.max_kstar);
        } else if (r.n_scored) {
          fprintf(f, "%s\t%lu\t%lu\t%.6f\n", names[c], (unsigned long)start, (unsigned long)end, track_mean(r));
        }
      }
    }
    if (mfx_close(fh)) return mfx_fail(MFX_E_IO, "writing '%s' failed (stream error or the compressor exited with an error)", path);
  }
  return MFX_OK;
}

// ---------------------------------------------------------------------------
// -completeness
// ---------------------------------------------------------------------------
extern "C" int mfx_completeness_pieces(mfx_eval *ev, double *total64, double *undrcpy64) {
  if (!ev || !total64 || !undrcpy64) return mfx_fail(MFX_E_INVAL, "mfx_completeness_pieces: null argument");
  if (ev->ix->seq_only) return mfx_fail(MFX_E_INVAL, "mfx_completeness: a sequence-only index holds the k-mers of one sequence, -completeness needs every read k-mer; build a full index (mfx_index_create)");
  DevGuard g(ev->device);
  DevBuf<double> dp;
  MFX_HIP(dp.alloc(128));
  MFX_HIP(mfx_memset_now(dp.p, 0, 128 * sizeof(double)));
  MFX_HIP(ev->ix->wide() ? mfx_kw_completeness(ev->ix->view(), ev->peak, ev->n_prob, ev->d_probK, ev->d_probP, dp.p, ev->grid, nullptr)
                          : mfx_k_completeness(ev->ix->view(), ev->peak, ev->n_prob, ev->d_probK, ev->d_probP, dp.p, ev->grid, nullptr));
  double h[128];
  MFX_HIP(hipMemcpy(h, dp.p, sizeof(h), hipMemcpyDeviceToHost));
  memcpy(total64, h, 64 * sizeof(double));
  memcpy(undrcpy64, h + 64, 64 * sizeof(double));
  return MFX_OK;
}

extern "C" int mfx_completeness(mfx_eval *ev, double *total, double *undrcpy) {
  if (!ev || !total || !undrcpy) return mfx_fail(MFX_E_INVAL, "mfx_completeness: null argument");
  double t64[64], u64[64];
  int rc = mfx_completeness_pieces(ev, t64, u64);
  if (rc) return rc;
  double t = 0, u = 0;
  for (int i = 0; i < 64; ++i) { t += t64[i]; u += u64[i]; }     // merfin-completeness.C:135-138
  *total = t;
  *undrcpy = u;
  return MFX_OK;
}
