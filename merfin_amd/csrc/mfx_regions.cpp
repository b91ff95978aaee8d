// mfx_regions.cpp -- the driver of -regions (include/merfin_amd.h: mfx_regions_run; the scheme: csrc/mfx_regions.h): pass 1 over every
// tile (class planes), the plane kernels of mfx_regions.hip with their scans (runs, joining, filter), pass 2 over the flagged tiles (sums),
// the check of pass 2's count of every region against the scanned one, and the host side: the records' order, the BED text, and the same
// steps over caller-made planes (mfx_regions_from_planes_host).  No reference counterpart: the reference README makes these intervals
// with awk from the -dump text ("Assess collapses and duplications").
#include "mfx_host.h"
#include "mfx_kernels.h"
#include "mfx_pipe.h"
#include "mfx_regions.h"

#include <math.h>
#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <vector>

static_assert(sizeof(mfx_region) == 56 && offsetof(mfx_region, start) == 8 && offsetof(mfx_region, n_kmers) == 24 && offsetof(mfx_region, ext_kstar) == 48,
              "mfx_region: the kernels address the record as 7 words");
static_assert(MFX_RG_TILE == MFX_TILE, "mfx_regions.h restates the tile");

struct mfx_regions {
  std::vector<mfx_region> recs;        // contig, start, class order
  uint64_t tiles_revisited = 0;
  double ms[3] = {0, 0, 0};
};

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int no_room(const char *what, uint64_t n, double bytes) {
  (void)hipGetLastError();
  return mfx_fail(MFX_E_NOMEM, "mfx_regions_run: no device memory for %lu %s (%.2f GB): a larger -kstar flags fewer positions; -minrun does not help here, "
                  "it drops regions after their runs are listed", (unsigned long)n, what, bytes / 1e9);
}
}  // namespace

extern "C" int mfx_regions_run(mfx_eval *ev, const mfx_seq *seq, const mfx_regions_opts *o, mfx_regions **out, uint64_t *kasm, uint64_t *kmissing) {
  if (!ev || !seq || !o || !out) return mfx_fail(MFX_E_INVAL, "mfx_regions_run: null argument");
  *out = nullptr;
  if (!std::isfinite(o->kstar) || !(o->kstar > 0))
    return mfx_fail(MFX_E_INVAL, "mfx_regions_run: the threshold -kstar must be a finite number above 0 (here %g): at 0 every scored k-mer would be in two classes", o->kstar);
  if (ev->device != seq->device) return mfx_fail(MFX_E_INVAL, "mfx_regions_run: evaluator and sequence live on different devices");
  if (ev->ix->shard_n > 1)
    return mfx_fail(MFX_E_INVAL, "mfx_regions_run: the index is shard %u of %u: a k-mer's class needs its whole counts; use a whole index", ev->ix->shard_rank,
                    ev->ix->shard_n);
  if (seq->partial) return mfx_seq_partial_error(seq, "-regions");
  DevGuard g(ev->device);
  int canon = 0;
  int rc = index_canonical(ev->ix, &canon);
  if (rc) return rc;
  if ((rc = mfx_check_seq_of_index(ev->ix, seq, "-regions")) != MFX_OK) return rc;
  if (kasm) *kasm = 0;
  if (kmissing) *kmissing = 0;
  mfx_regions *R = new mfx_regions;
  struct Drop { mfx_regions *r; ~Drop() { delete r; } } drop{R};
  const uint64_t ntiles = seq->ntiles;
  if (ntiles == 0) { *out = R; drop.r = nullptr; return MFX_OK; }
  const bool planes = !ev->ix->wide() && (seq->planes_ok || seq->bases_stale);       // (the 128-bit kernels read one byte per base)
  if (!planes && (rc = mfx_seq_ensure_ascii(seq)) != MFX_OK) return rc;

  // ---- pass 1: the class planes ----
  const uint64_t nwords = ntiles * MFX_RG_WORDS, nct = ntiles * MFX_RG_CLASSES;
  DevBuf<uint64_t> dplanes, dst, dflag, dcs, dce;
  if (dplanes.alloc(3 * nwords) != hipSuccess) {
    (void)hipGetLastError();
    return mfx_fail(MFX_E_NOMEM, "mfx_regions_run: no device memory for the class planes of %lu tiles (%.2f GB)", (unsigned long)ntiles, 24.0 * (double)nwords / 1e9);
  }
  MFX_HIP(dst.alloc(2));
  MFX_HIP(dflag.alloc(ntiles));
  MFX_HIP(dcs.alloc(nct + 1));
  MFX_HIP(dce.alloc(nct + 1));
  MFX_HIP(mfx_memset_now(dst.p, 0, 2 * sizeof(uint64_t)));
  MFX_HIP(mfx_memset_now(dflag.p, 0, ntiles * sizeof(uint64_t)));
  MFX_HIP(mfx_memset_now(dcs.p, 0, (nct + 1) * sizeof(uint64_t)));
  MFX_HIP(mfx_memset_now(dce.p, 0, (nct + 1) * sizeof(uint64_t)));
  mfx_regions_args a;
  a.t = ev->ix->view();
  a.canonical = canon;
  a.bases = seq->d_bases;
  if (planes) { a.codes = seq->d_codes; a.valid = seq->d_valid; }
  a.contig_off = seq->d_contig_off;
  a.contig_len = seq->d_contig_len;
  a.tile_start = seq->d_tile_start;
  a.tile_contig = seq->d_tile_contig;
  a.ntiles = ntiles;
  a.peak = ev->peak;
  a.n_prob = ev->n_prob;
  a.probK = ev->d_probK;
  a.probP = ev->d_probP;
  a.kstar = o->kstar;
  a.planes = dplanes.p;
  a.stats = dst.p;
  double t0 = now_ms();
  MFX_HIP(ev->ix->wide() ? mfx_kw_regions_class(a, nullptr) : mfx_k_regions_class(a, nullptr));
  uint64_t st[2];
  MFX_HIP(hipMemcpy(st, dst.p, sizeof(st), hipMemcpyDeviceToHost));
  R->ms[0] = now_ms() - t0;
  if (kasm) *kasm = st[0];
  if (kmissing) *kmissing = st[1];

  // ---- planes -> runs: count, scan, scatter ----
  // (the scans share one temporary buffer, grown when a later array is longer; what the host needs of a stage -- a few totals -- is picked
  // into dtot and copied once: that copy is the stage's only wait)
  t0 = now_ms();
  DevBuf<uint64_t> dtot;
  MFX_HIP(dtot.alloc(8));
  struct Tmp {
    void *p = nullptr;
    size_t bytes = 0;
    ~Tmp() { if (p) (void)hipFree(p); }
    hipError_t room(uint64_t n) {
      const size_t need = mfx_k_rg_temp_bytes(n);
      if (need <= bytes) return hipSuccess;
      if (p) (void)hipFree(p);
      p = nullptr;
      bytes = 0;
      const hipError_t e = hipMalloc(&p, need);
      if (e == hipSuccess) bytes = need;
      return e;
    }
  } tmp;
  MFX_HIP(tmp.room(nct + 1));
  MFX_HIP(mfx_k_rg_count(dplanes.p, ntiles, seq->d_tile_contig, dcs.p, dce.p, dflag.p, nullptr));
  MFX_HIP(mfx_k_rg_scan(dcs.p, nct + 1, tmp.p, tmp.bytes, nullptr));
  MFX_HIP(mfx_k_rg_scan(dce.p, nct + 1, tmp.p, tmp.bytes, nullptr));
  uint64_t tot[8];
  {
    const uint64_t at_s[4] = {0, ntiles, 2 * ntiles, 3 * ntiles}, at_e[1] = {nct};
    MFX_HIP(mfx_k_rg_pick(dcs.p, at_s, 4, dtot.p, nullptr));
    MFX_HIP(mfx_k_rg_pick(dce.p, at_e, 1, dtot.p + 4, nullptr));
    MFX_HIP(mfx_k_rg_sum(dflag.p, ntiles, dtot.p + 5, tmp.p, tmp.bytes, nullptr));          // (a flag is 0 or 1)
    MFX_HIP(hipMemcpy(tot, dtot.p, 6 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  const uint64_t cls_run[MFX_RG_CLASSES + 1] = {tot[0], tot[1], tot[2], tot[3]}, ends_total = tot[4];
  const uint64_t nruns = cls_run[MFX_RG_CLASSES];
  if (ends_total != nruns)
    return mfx_fail(MFX_E_HIP, "mfx_regions_run: internal error: the planes hold %lu run starts and %lu run ends", (unsigned long)nruns, (unsigned long)ends_total);
  R->tiles_revisited = tot[5];
  uint64_t reg_begin[MFX_RG_CLASSES + 1] = {0, 0, 0, 0};
  DevBuf<uint64_t> dregs, drecount;
  uint64_t nreg = 0;
  if (nruns) {
    DevBuf<uint32_t> drc;
    DevBuf<uint64_t> drs, dre, dhead, dlen, dfirst, dlast, dkeep;
    const double run_bytes = 36.0 * (double)nruns;
    if (drc.alloc(nruns) != hipSuccess || drs.alloc(nruns) != hipSuccess || dre.alloc(nruns) != hipSuccess || dhead.alloc(nruns + 1) != hipSuccess ||
        dlen.alloc(nruns + 1) != hipSuccess || tmp.room(nruns + 1) != hipSuccess)
      return no_room("runs", nruns, run_bytes);
    MFX_HIP(mfx_k_rg_scatter(dplanes.p, ntiles, seq->d_tile_start, seq->d_tile_contig, dcs.p, dce.p, drc.p, drs.p, dre.p, nullptr));
    // ---- joining by -gap, filter by -minrun ----
    MFX_HIP(mfx_k_rg_heads(drc.p, drs.p, dre.p, nruns, cls_run, o->gap, dhead.p, dlen.p, nullptr));
    MFX_HIP(mfx_k_rg_scan(dhead.p, nruns + 1, tmp.p, tmp.bytes, nullptr));
    MFX_HIP(mfx_k_rg_scan(dlen.p, nruns + 1, tmp.p, tmp.bytes, nullptr));
    uint64_t cls_raw[MFX_RG_CLASSES + 1];                       // a class's first run opens a region: the heads in front of it number that region
    MFX_HIP(mfx_k_rg_pick(dhead.p, cls_run, 4, dtot.p, nullptr));
    MFX_HIP(hipMemcpy(cls_raw, dtot.p, sizeof(cls_raw), hipMemcpyDeviceToHost));
    const uint64_t nraw = cls_raw[MFX_RG_CLASSES];
    if (dfirst.alloc(nraw) != hipSuccess || dlast.alloc(nraw) != hipSuccess || dkeep.alloc(nraw + 1) != hipSuccess) return no_room("regions", nraw, 24.0 * (double)nraw);
    MFX_HIP(mfx_k_rg_bounds(dhead.p, nruns, dfirst.p, dlast.p, nullptr));
    MFX_HIP(mfx_k_rg_keep(dfirst.p, dlast.p, dlen.p, nraw, o->min_kmers, dkeep.p, nullptr));
    MFX_HIP(mfx_k_rg_scan(dkeep.p, nraw + 1, tmp.p, tmp.bytes, nullptr));
    MFX_HIP(mfx_k_rg_pick(dkeep.p, cls_raw, 4, dtot.p, nullptr));
    MFX_HIP(hipMemcpy(reg_begin, dtot.p, sizeof(reg_begin), hipMemcpyDeviceToHost));
    nreg = reg_begin[MFX_RG_CLASSES];
    if (nreg) {
      if (dregs.alloc(nreg * MFX_RG_REC_WORDS) != hipSuccess || drecount.alloc(nreg) != hipSuccess) return no_room("records", nreg, 64.0 * (double)nreg);
      MFX_HIP(mfx_memset_now(drecount.p, 0, nreg * sizeof(uint64_t)));
      MFX_HIP(mfx_k_rg_emit(dfirst.p, dlast.p, dlen.p, dkeep.p, nraw, cls_run, drc.p, drs.p, dre.p, dregs.p, nullptr));
    }
    MFX_HIP(hipStreamSynchronize(nullptr));
  }
  R->ms[1] = now_ms() - t0;

  // ---- pass 2: the sums, over the tiles that hold a flagged position ----
  if (nreg) {
    t0 = now_ms();
    a.stats = nullptr;
    a.tile_flag = dflag.p;
    a.regs = dregs.p;
    a.recount = drecount.p;
    a.reg_begin0 = reg_begin[0]; a.reg_begin1 = reg_begin[1]; a.reg_begin2 = reg_begin[2]; a.reg_begin3 = reg_begin[3];
    MFX_HIP(ev->ix->wide() ? mfx_kw_regions_sums(a, nullptr) : mfx_k_regions_sums(a, nullptr));
    MFX_HIP(mfx_k_rg_finish(dregs.p, nreg, nullptr));
    std::vector<mfx_region> byclass((size_t)nreg);
    std::vector<uint64_t> recount((size_t)nreg);
    MFX_HIP(hipMemcpy(byclass.data(), dregs.p, nreg * sizeof(mfx_region), hipMemcpyDeviceToHost));
    MFX_HIP(hipMemcpy(recount.data(), drecount.p, nreg * sizeof(uint64_t), hipMemcpyDeviceToHost));
    R->ms[2] = now_ms() - t0;
    for (uint64_t i = 0; i < nreg; ++i)
      if (recount[i] != byclass[i].n_kmers)
        return mfx_fail(MFX_E_HIP, "mfx_regions_run: internal error: region %lu (contig %u, class %u, [%lu, %lu)) holds %lu flagged k-mers by its runs, "
                        "the second pass found %lu", (unsigned long)i, byclass[i].contig, byclass[i].cls, (unsigned long)byclass[i].start,
                        (unsigned long)byclass[i].end, (unsigned long)byclass[i].n_kmers, (unsigned long)recount[i]);
    mfx_rg_order(byclass.data(), reg_begin, R->recs);
  } else {
    R->tiles_revisited = 0;                                   // no record survived: pass 2 did not run
  }
  *out = R;
  drop.r = nullptr;
  return MFX_OK;
}

extern "C" uint64_t mfx_regions_count(const mfx_regions *r) { return r ? r->recs.size() : 0; }
extern "C" uint64_t mfx_regions_tiles_revisited(const mfx_regions *r) { return r ? r->tiles_revisited : 0; }
extern "C" void mfx_diag_regions_times(const mfx_regions *r, double *ms) {
  if (r && ms) memcpy(ms, r->ms, sizeof(r->ms));
}
extern "C" int mfx_regions_copy(const mfx_regions *r, mfx_region *dst, uint64_t cap) {
  if (!r || (!dst && !r->recs.empty())) return mfx_fail(MFX_E_INVAL, "mfx_regions_copy: null argument");
  if (cap < r->recs.size()) return mfx_fail(MFX_E_INVAL, "mfx_regions_copy: %lu records, room for %lu", (unsigned long)r->recs.size(), (unsigned long)cap);
  if (!r->recs.empty()) memcpy(dst, r->recs.data(), r->recs.size() * sizeof(mfx_region));
  return MFX_OK;
}
extern "C" void mfx_regions_free(mfx_regions *r) { delete r; }

extern "C" int mfx_regions_write(const mfx_region *r, uint64_t n, const mfx_seq *seq, const char *const *names, int k, const char *bed_path) {
  if (!seq || (!r && n) || !names || !bed_path) return mfx_fail(MFX_E_INVAL, "mfx_regions_write: null argument");
  if (k < 1 || k > MFX_MAX_K) return mfx_fail(MFX_E_INVAL, "mfx_regions_write: k = %d is outside [1, %d]", k, MFX_MAX_K);
  static const char *const cls_name[MFX_RG_CLASSES] = {"missing", "collapsed", "expanded"};
  for (uint64_t i = 0; i < n; ++i) {
    const mfx_region &x = r[i];
    if (x.contig >= seq->ncontigs || x.cls >= MFX_RG_CLASSES || x.start >= x.end || x.n_kmers == 0 || x.end - 1 + (uint64_t)k > seq->len[x.contig])
      return mfx_fail(MFX_E_INVAL, "mfx_regions_write: record %lu is no region of these sequences (contig %u, class %u, [%lu, %lu), %lu k-mers)", (unsigned long)i,
                      x.contig, x.cls, (unsigned long)x.start, (unsigned long)x.end, (unsigned long)x.n_kmers);
  }
  mfx_file fh = mfx_open_writer(bed_path, false);             // compressedFileWriter: compressor chosen by suffix (mfx_pipe.h)
  if (!fh.f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", bed_path);
  fprintf(fh.f, "#chrom\tstart\tend\tclass\tn_kmers\tmean_readK\tmean_asmK\text_kstar\n");
  for (uint64_t i = 0; i < n; ++i) {
    const mfx_region &x = r[i];
    fprintf(fh.f, "%s\t%lu\t%lu\t%s\t%lu\t%.2f\t%.2f\t%.2f\n", names[x.contig], (unsigned long)x.start, (unsigned long)(x.end - 1 + (uint64_t)k), cls_name[x.cls],
            (unsigned long)x.n_kmers, (double)x.sum_readK / (double)x.n_kmers, (double)x.sum_asmK / (double)x.n_kmers, x.ext_kstar);
  }
  if (mfx_close(fh)) return mfx_fail(MFX_E_IO, "writing '%s' failed (stream error or the compressor exited with an error)", bed_path);
  return MFX_OK;
}

extern "C" int mfx_regions_from_planes_host(const uint64_t *planes, const uint64_t *contig_len, uint32_t ncontigs, const mfx_regions_opts *o, mfx_region *out,
                                            uint64_t cap, uint64_t *n_out) {
  if ((!contig_len && ncontigs) || !o || !n_out || (!out && cap)) return mfx_fail(MFX_E_INVAL, "mfx_regions_from_planes_host: null argument");
  std::vector<uint64_t> tile_start((size_t)ncontigs + 1, 0);
  for (uint32_t c = 0; c < ncontigs; ++c) tile_start[c + 1] = tile_start[c] + (contig_len[c] + MFX_RG_TILE - 1) / MFX_RG_TILE;
  const uint64_t ntiles = tile_start[ncontigs], nw = ntiles * MFX_RG_WORDS;
  if (ntiles && !planes) return mfx_fail(MFX_E_INVAL, "mfx_regions_from_planes_host: null argument");
  std::vector<uint32_t> tile_contig((size_t)ntiles);
  for (uint32_t c = 0; c < ncontigs; ++c) std::fill(tile_contig.begin() + (size_t)tile_start[c], tile_contig.begin() + (size_t)tile_start[c + 1], c);
  for (uint32_t c = 0; c < ncontigs; ++c) {                   // bits beyond a contig's end
    const uint64_t len = contig_len[c], w0 = tile_start[c] * MFX_RG_WORDS, w1 = tile_start[c + 1] * MFX_RG_WORDS;
    for (uint64_t w = w0 + len / 64; w < w1; ++w) {
      const uint64_t beyond = w == w0 + len / 64 ? ~0ull << (len % 64) : ~0ull;
      for (uint32_t cls = 0; cls < MFX_RG_CLASSES; ++cls)
        if (planes[cls * nw + w] & beyond)
          return mfx_fail(MFX_E_INVAL, "mfx_regions_from_planes_host: class %u flags a position beyond the %lu positions of contig %u", cls, (unsigned long)len, c);
    }
  }
  std::vector<mfx_region> recs;
  mfx_regions_planes_host(planes, ntiles, tile_start.data(), tile_contig.data(), o->gap, o->min_kmers, recs);
  *n_out = recs.size();
  const uint64_t n = std::min<uint64_t>(cap, recs.size());
  if (n) memcpy(out, recs.data(), n * sizeof(mfx_region));
  return MFX_OK;
}
