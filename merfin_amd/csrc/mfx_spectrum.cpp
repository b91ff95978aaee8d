// mfx_spectrum.cpp -- host side of the copy-number spectrum (mfx_spectrum.h): the pass over an index, the rule that reads the
// haploid peak off its single-copy row, and the text report.  No reference counterpart (merfin is handed -peak).
// The report's layout is believed to be what Merqury's spectra-cn plot reads; it is written from memory and UNVALIDATED
// against Merqury.
#include "mfx_spectrum.h"
#include "mfx_pipe.h"

#include <inttypes.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace {
struct SpecDevGuard {
  int prev = -1;
  explicit SpecDevGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~SpecDevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
struct SpecScratch {       // the image on the device and the stream of one call
  uint64_t *d = nullptr;
  hipStream_t st = nullptr;
  ~SpecScratch() {
    if (st) (void)hipStreamDestroy(st);
    if (d) (void)hipFree(d);
  }
};
struct SpecEvents {
  hipEvent_t a = nullptr, b = nullptr;
  ~SpecEvents() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};
bool range_error(uint32_t copies, uint32_t max_mult, const char *who) {
  if (copies < MFX_SPEC_MIN_COPIES || copies > MFX_SPEC_MAX_COPIES) {
    mfx_fail(MFX_E_INVAL, "%s: copies = %u is outside [%u, %u]", who, copies, MFX_SPEC_MIN_COPIES, MFX_SPEC_MAX_COPIES);
    return true;
  }
  if (max_mult < MFX_SPEC_MIN_MULT || max_mult > MFX_SPEC_MAX_MULT) {
    mfx_fail(MFX_E_INVAL, "%s: max_mult = %u is outside [%u, %u]", who, max_mult, MFX_SPEC_MIN_MULT, MFX_SPEC_MAX_MULT);
    return true;
  }
  return false;
}
}  // namespace

// The pass itself.  aggregate < 0: the library's choice (MFX_SPECTRUM_AGG, else MFX_SPEC_AGG_DEFAULT); ms: null, or the kernels' time of each of
// `reps` passes between two HIP events (the image is cleared before every pass, outside the events)
static int spectrum_pass(const mfx_index *ix, uint32_t copies, uint32_t max_mult, int aggregate, uint32_t reps, uint64_t *out, uint64_t *n_entries,
                         float *ms, const char *who) {
  if (range_error(copies, max_mult, who)) return MFX_E_INVAL;
  SpecDevGuard g(ix->device);
  uint64_t meta[2] = {0, 0};
  MFX_HIP(hipMemcpy(meta, ix->d_meta, sizeof(meta), hipMemcpyDeviceToHost));
  if (meta[1] > 0)
    return mfx_fail(MFX_E_INVAL, "%s: the index took %" PRIu64 " non-canonical k-mers: such a database splits one k-mer over two "
                    "entries, so the spectrum of its entries is not the spectrum of its k-mers", who, meta[1]);
  const size_t cells = (size_t)(copies + 2u) * (max_mult + 1u), words = cells + 1;      // + the kernels' entry counter
  SpecScratch s;
  MFX_HIP(hipMalloc((void **)&s.d, words * sizeof(uint64_t)));
  MFX_HIP(mfx_memset_now(s.d, 0, words * sizeof(uint64_t)));
  MFX_HIP(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
  int cus = 0;
  MFX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix->device));
  mfx_spectrum_args a;
  a.t = ix->view();
  a.copies = copies;
  a.max_mult = max_mult;
  a.lds_cols = mfx_spec_lds_cols(copies, max_mult);
  const char *ag = getenv("MFX_SPECTRUM_AGG");                   // A/B (docs/KNOBS.md); read per call: tests switch it
  a.aggregate = aggregate >= 0 ? aggregate : ag ? (atoi(ag) != 0) : MFX_SPEC_AGG_DEFAULT;
  a.img = s.d;
  const int grid = (cus > 0 ? cus : 256) * 4;                    // 32 KB of LDS bins per block: four blocks of four waves per CU
  SpecEvents ev;
  if (ms) { MFX_HIP(hipEventCreate(&ev.a)); MFX_HIP(hipEventCreate(&ev.b)); }
  for (uint32_t rep = 0; rep < reps; ++rep) {
    if (rep) MFX_HIP(hipMemsetAsync(s.d, 0, words * sizeof(uint64_t), s.st));
    if (ms) MFX_HIP(hipEventRecord(ev.a, s.st));
    MFX_HIP(ix->wide() ? mfx_kw_spectrum(a, grid, s.st) : mfx_k_spectrum(a, grid, s.st));
    if (ms) {
      MFX_HIP(hipEventRecord(ev.b, s.st));
      MFX_HIP(hipEventSynchronize(ev.b));
      MFX_HIP(hipEventElapsedTime(&ms[rep], ev.a, ev.b));
    }
  }
  std::vector<uint64_t> h(words);
  MFX_HIP(hipMemcpyAsync(h.data(), s.d, words * sizeof(uint64_t), hipMemcpyDeviceToHost, s.st));
  MFX_HIP(hipStreamSynchronize(s.st));
  uint64_t sum = 0;
  for (size_t i = 0; i < cells; ++i) { if (out) out[i] = h[i]; sum += h[i]; }
  if (sum != h[cells])
    return mfx_fail(MFX_E_HIP, "%s: the image sums to %" PRIu64 ", the pass counted %" PRIu64 " entries", who, sum, h[cells]);
  if (n_entries) *n_entries = sum;
  return MFX_OK;
}

extern "C" int mfx_spectrum_run(const mfx_index *ix, uint32_t copies, uint32_t max_mult, uint64_t *out, uint64_t *n_entries) {
  if (!ix || !out || !n_entries) return mfx_fail(MFX_E_INVAL, "mfx_spectrum_run: null argument");
  return spectrum_pass(ix, copies, max_mult, -1, 1, out, n_entries, nullptr, "mfx_spectrum_run");
}

extern "C" int mfx_diag_spectrum_time(const mfx_index *ix, uint32_t copies, uint32_t max_mult, int aggregate, uint32_t reps, float *kernel_ms) {
  if (!ix || !kernel_ms || reps == 0) return mfx_fail(MFX_E_INVAL, "mfx_diag_spectrum_time: null argument");
  return spectrum_pass(ix, copies, max_mult, aggregate ? 1 : 0, reps, nullptr, nullptr, kernel_ms, "mfx_diag_spectrum_time");
}

// ---- the peak rule (include/merfin_amd.h) ------------------------------------------------------------------
namespace {
typedef unsigned __int128 u128;
struct Mean { u128 s; uint32_t n; };                             // s / n, n in [1, 5]: products of a sum with 10 * n stay below 2^74
inline bool le(const Mean &x, const Mean &y) { return x.s * y.n <= y.s * x.n; }      // x <= y
inline bool lt(const Mean &x, const Mean &y) { return x.s * y.n < y.s * x.n; }
}  // namespace

extern "C" int mfx_spectrum_peak(const uint64_t *row, uint32_t max_mult, mfx_spectrum_peak_t *out) {
  if (!row || !out) return mfx_fail(MFX_E_INVAL, "mfx_spectrum_peak: null argument");
  if (max_mult < MFX_SPEC_MIN_MULT || max_mult > MFX_SPEC_MAX_MULT)
    return mfx_fail(MFX_E_INVAL, "mfx_spectrum_peak: max_mult = %u is outside [%u, %u]", max_mult, MFX_SPEC_MIN_MULT, MFX_SPEC_MAX_MULT);
  const uint32_t last = max_mult - 1;                            // the largest m that takes part
  auto a = [&](uint32_t m) {
    const uint32_t lo = m > 3 ? m - 2 : 1, hi = m + 2 < last ? m + 2 : last;
    Mean r{0, hi - lo + 1};
    for (uint32_t j = lo; j <= hi; ++j) r.s += row[j];
    return r;
  };
  uint32_t v = 0;
  for (uint32_t m = 1; m + 1 <= last; ++m)
    if (le(a(m), a(m + 1))) { v = m; break; }
  if (v == 0) return mfx_fail(MFX_E_NODATA, "mfx_spectrum_peak: the row falls all the way: no valley, no peak");
  uint32_t p = v + 1;
  Mean ap = a(p);
  for (uint32_t m = v + 2; m <= last; ++m) { const Mean x = a(m); if (lt(ap, x)) { ap = x; p = m; } }
  if (ap.s == 0) return mfx_fail(MFX_E_NODATA, "mfx_spectrum_peak: nothing beyond the valley at %u", v);
  uint32_t hap = p;
  const uint32_t lo = std::max(v + 1, (2 * p + 4) / 5), hi = 3 * p / 5;
  if (lo <= hi) {
    uint32_t h = lo;
    Mean ah = a(h);
    for (uint32_t m = lo + 1; m <= hi; ++m) { const Mean x = a(m); if (lt(ah, x)) { ah = x; h = m; } }
    bool ok = 10 * ah.s * ap.n >= ap.s * ah.n;                   // 10 a[h] >= a[p]
    for (uint32_t j = h > 3 ? h - 2 : 1; ok && j <= (h + 2 < last ? h + 2 : last); ++j) ok = le(a(j), ah);
    if (ok) hap = h;                                             // a haploid assembly of a diploid genome: the 2-copy peak dominates
  }
  out->valley = v;
  out->main_peak = p;
  out->haploid_peak = hap;
  out->count_at_peak = row[hap];
  return MFX_OK;
}

extern "C" int mfx_spectrum_write(const uint64_t *img, uint32_t copies, uint32_t max_mult, int with_read_only, const char *path) {
  if (!img || !path) return mfx_fail(MFX_E_INVAL, "mfx_spectrum_write: null argument");
  if (range_error(copies, max_mult, "mfx_spectrum_write")) return MFX_E_INVAL;
  mfx_file fh = mfx_open_writer(path, false);                    // compressor chosen by suffix (mfx_pipe.h)
  if (!fh.f) return mfx_fail(MFX_E_IO, "mfx_spectrum_write: cannot open '%s' for writing", path);
  fprintf(fh.f, "Copies\tkmer_multiplicity\tCount\n");
  for (uint32_t r = with_read_only ? 0u : 1u; r < copies + 2u; ++r) {
    char label[16];
    if (r == 0) snprintf(label, sizeof label, "read-only");
    else if (r <= copies) snprintf(label, sizeof label, "%u", r);
    else snprintf(label, sizeof label, ">%u", copies);
    const uint64_t *row = img + (size_t)r * (max_mult + 1u);
    for (uint32_t m = 0; m <= max_mult; ++m)
      if (row[m]) fprintf(fh.f, "%s\t%u\t%" PRIu64 "\n", label, m, row[m]);
  }
  if (mfx_close(fh)) return mfx_fail(MFX_E_IO, "mfx_spectrum_write: writing '%s' failed", path);
  return MFX_OK;
}
