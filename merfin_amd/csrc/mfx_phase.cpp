// mfx_phase.cpp -- the driver of -phase (include/merfin_amd.h: mfx_phase_run; the scheme: csrc/mfx_phase.h): pass 1 over every tile (the two
// haplotype planes, the per-contig totals), the plane kernels of mfx_phase.hip with their scans (markers, runs, blocks), every array
// sized after the count in front of it, and the host side: the three texts and the same steps over caller-made planes
// (mfx_phase_from_planes_host).  No reference counterpart: merfin has no trio mode.
#include "mfx_host.h"
#include "mfx_kernels.h"
#include "mfx_pipe.h"
#include "mfx_phase.h"

#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

static_assert(sizeof(mfx_phase_block) == 48 && offsetof(mfx_phase_block, start) == 8 && offsetof(mfx_phase_block, n_switch_runs) == 40,
              "mfx_phase_block: the kernels address the record as 6 words");
static_assert(MFX_RG_TILE == MFX_TILE, "mfx_regions.h restates the tile");

struct mfx_phase {
  std::vector<mfx_phase_block> recs;   // contig, start order
  std::vector<uint64_t> counts;        // [ncontigs][4]
  double ms[2] = {0, 0};
};

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int no_room(const char *what, uint64_t n, double bytes) {
  (void)hipGetLastError();
  return mfx_fail(MFX_E_NOMEM, "mfx_phase_run: no device memory for %lu %s (%.2f GB)", (unsigned long)n, what, bytes / 1e9);
}
}  // namespace

extern "C" int mfx_phase_run(mfx_eval *ev, const mfx_seq *seq, const mfx_phase_opts *o, mfx_phase **out) {
  if (!ev || !seq || !o || !out) return mfx_fail(MFX_E_INVAL, "mfx_phase_run: null argument");
  *out = nullptr;
  if (ev->device != seq->device) return mfx_fail(MFX_E_INVAL, "mfx_phase_run: evaluator and sequence live on different devices");
  if (ev->ix->shard_n > 1)
    return mfx_fail(MFX_E_INVAL, "mfx_phase_run: the index is shard %u of %u: a marker needs both sets' whole membership; use a whole index", ev->ix->shard_rank,
                    ev->ix->shard_n);
  if (seq->partial) return mfx_seq_partial_error(seq, "-phase");
  DevGuard g(ev->device);
  int canon = 0;
  int rc = index_canonical(ev->ix, &canon);
  if (rc) return rc;
  if ((rc = mfx_check_seq_of_index(ev->ix, seq, "-phase")) != MFX_OK) return rc;
  mfx_phase *P = new mfx_phase;
  struct Drop { mfx_phase *p; ~Drop() { delete p; } } drop{P};
  const uint64_t ntiles = seq->ntiles, ncontigs = seq->ncontigs;
  P->counts.assign((size_t)ncontigs * 4, 0);
  if (ntiles == 0) { *out = P; drop.p = nullptr; return MFX_OK; }
  const bool planes = !ev->ix->wide() && (seq->planes_ok || seq->bases_stale);       // (the 128-bit kernels read one byte per base)
  if (!planes && (rc = mfx_seq_ensure_ascii(seq)) != MFX_OK) return rc;

  // ---- pass 1: the haplotype planes, the totals ----
  const uint64_t nwords = ntiles * MFX_RG_WORDS;
  DevBuf<uint64_t> dplanes, dcounts;
  if (dplanes.alloc(2 * nwords) != hipSuccess) return no_room("tiles' haplotype planes", ntiles, 16.0 * (double)nwords);
  MFX_HIP(dcounts.alloc(ncontigs * 4));
  MFX_HIP(mfx_memset_now(dcounts.p, 0, ncontigs * 4 * sizeof(uint64_t)));
  mfx_phase_args a;
  a.t = ev->ix->view();
  a.canonical = canon;
  a.bases = seq->d_bases;
  if (planes) { a.codes = seq->d_codes; a.valid = seq->d_valid; }
  a.contig_off = seq->d_contig_off;
  a.contig_len = seq->d_contig_len;
  a.tile_start = seq->d_tile_start;
  a.tile_contig = seq->d_tile_contig;
  a.ntiles = ntiles;
  a.planes = dplanes.p;
  a.counts = dcounts.p;
  double t0 = now_ms();
  MFX_HIP(ev->ix->wide() ? mfx_kw_phase_mark(a, nullptr) : mfx_k_phase_mark(a, nullptr));
  MFX_HIP(hipMemcpy(P->counts.data(), dcounts.p, ncontigs * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  P->ms[0] = now_ms() - t0;

  // ---- planes -> markers -> runs: tile, scans, count, scan, scatter ----
  // (the scans share one temporary buffer, grown when a later array is longer; what the host needs of a stage -- two totals -- is picked
  // into dtot and copied once: that copy is the stage's only wait)
  t0 = now_ms();
  struct Tmp {
    void *p = nullptr;
    size_t bytes = 0;
    ~Tmp() { if (p) (void)hipFree(p); }
    hipError_t room(uint64_t n) {
      const size_t need = mfx_k_ph_temp_bytes(n);
      if (need <= bytes) return hipSuccess;
      if (p) (void)hipFree(p);
      p = nullptr;
      bytes = 0;
      const hipError_t e = hipMalloc(&p, need);
      if (e == hipSuccess) bytes = need;
      return e;
    }
  } tmp;
  DevBuf<uint64_t> dtot, drank0, dcar, doff;
  MFX_HIP(dtot.alloc(4));
  MFX_HIP(drank0.alloc(ntiles + 1));
  MFX_HIP(dcar.alloc(ntiles));
  MFX_HIP(doff.alloc(ntiles + 1));
  MFX_HIP(tmp.room(ntiles + 1));
  MFX_HIP(mfx_k_ph_tile(dplanes.p, ntiles, seq->d_tile_start, seq->d_tile_contig, drank0.p, dcar.p, nullptr));
  MFX_HIP(mfx_k_rg_scan(drank0.p, ntiles + 1, tmp.p, tmp.bytes, nullptr));
  MFX_HIP(mfx_k_ph_join_scan(dcar.p, dcar.p, ntiles, tmp.p, tmp.bytes, nullptr));
  MFX_HIP(mfx_k_ph_count(dplanes.p, ntiles, seq->d_tile_start, seq->d_tile_contig, dcar.p, doff.p, nullptr));
  MFX_HIP(mfx_k_rg_scan(doff.p, ntiles + 1, tmp.p, tmp.bytes, nullptr));
  uint64_t tot[2];
  {
    const uint64_t at[1] = {ntiles};
    MFX_HIP(mfx_k_rg_pick(drank0.p, at, 1, dtot.p, nullptr));
    MFX_HIP(mfx_k_rg_pick(doff.p, at, 1, dtot.p + 1, nullptr));
    MFX_HIP(hipMemcpy(tot, dtot.p, sizeof(tot), hipMemcpyDeviceToHost));
  }
  const uint64_t nmarkers = tot[0], nruns = tot[1];
  {
    uint64_t by_counts = 0;
    for (uint64_t c = 0; c < ncontigs; ++c) by_counts += P->counts[4 * c + 1] + P->counts[4 * c + 2];
    if (by_counts != nmarkers)
      return mfx_fail(MFX_E_HIP, "mfx_phase_run: internal error: the planes hold %lu markers, the evaluation counted %lu", (unsigned long)nmarkers, (unsigned long)by_counts);
  }
  if (nruns) {
    DevBuf<uint32_t> drc, drh;
    DevBuf<uint64_t> drs, dre, drr, dlng, dlngx, dax, dbx, dhead, dfirst, dlast, drecs;
    if (drc.alloc(nruns) != hipSuccess || drh.alloc(nruns) != hipSuccess || drs.alloc(nruns) != hipSuccess || dre.alloc(nruns) != hipSuccess ||
        drr.alloc(nruns) != hipSuccess || dlng.alloc(nruns) != hipSuccess || dlngx.alloc(nruns) != hipSuccess || dax.alloc(nruns + 1) != hipSuccess ||
        dbx.alloc(nruns + 1) != hipSuccess || dhead.alloc(nruns + 1) != hipSuccess || tmp.room(nruns + 1) != hipSuccess)
      return no_room("runs", nruns, 72.0 * (double)nruns);
    MFX_HIP(mfx_k_ph_scatter(dplanes.p, ntiles, seq->d_tile_start, seq->d_tile_contig, dcar.p, drank0.p, doff.p, drc.p, drh.p, drs.p, dre.p, drr.p, nullptr));
    // ---- runs -> blocks ----
    MFX_HIP(mfx_k_ph_runs(drc.p, drh.p, drs.p, dre.p, drr.p, nruns, nmarkers, (uint64_t)a.t.k, o->switches, o->range, dlng.p, dax.p, dbx.p, nullptr));
    MFX_HIP(mfx_k_ph_join_scan(dlng.p, dlngx.p, nruns, tmp.p, tmp.bytes, nullptr));
    MFX_HIP(mfx_k_rg_scan(dax.p, nruns + 1, tmp.p, tmp.bytes, nullptr));
    MFX_HIP(mfx_k_rg_scan(dbx.p, nruns + 1, tmp.p, tmp.bytes, nullptr));
    MFX_HIP(mfx_k_ph_heads(drc.p, drh.p, dlng.p, dlngx.p, nruns, dhead.p, nullptr));
    MFX_HIP(mfx_k_rg_scan(dhead.p, nruns + 1, tmp.p, tmp.bytes, nullptr));
    uint64_t nblocks = 0;
    {
      const uint64_t at[1] = {nruns};
      MFX_HIP(mfx_k_rg_pick(dhead.p, at, 1, dtot.p, nullptr));
      MFX_HIP(hipMemcpy(&nblocks, dtot.p, sizeof(nblocks), hipMemcpyDeviceToHost));
    }
    if (nblocks == 0 || nblocks > nruns)
      return mfx_fail(MFX_E_HIP, "mfx_phase_run: internal error: %lu runs open %lu blocks", (unsigned long)nruns, (unsigned long)nblocks);
    if (dfirst.alloc(nblocks) != hipSuccess || dlast.alloc(nblocks) != hipSuccess || drecs.alloc(nblocks * MFX_PH_REC_WORDS) != hipSuccess)
      return no_room("blocks", nblocks, 64.0 * (double)nblocks);
    MFX_HIP(mfx_k_rg_bounds(dhead.p, nruns, dfirst.p, dlast.p, nullptr));
    MFX_HIP(mfx_k_ph_emit(dfirst.p, dlast.p, nblocks, drc.p, drh.p, drs.p, dre.p, dlngx.p, dax.p, dbx.p, drecs.p, nullptr));
    P->recs.resize((size_t)nblocks);
    MFX_HIP(hipMemcpy(P->recs.data(), drecs.p, nblocks * sizeof(mfx_phase_block), hipMemcpyDeviceToHost));
  }
  P->ms[1] = now_ms() - t0;
  *out = P;
  drop.p = nullptr;
  return MFX_OK;
}

extern "C" uint64_t mfx_phase_count(const mfx_phase *p) { return p ? p->recs.size() : 0; }
extern "C" void mfx_diag_phase_times(const mfx_phase *p, double *ms) {
  if (p && ms) memcpy(ms, p->ms, sizeof(p->ms));
}
extern "C" int mfx_phase_copy(const mfx_phase *p, mfx_phase_block *dst, uint64_t cap) {
  if (!p || (!dst && !p->recs.empty())) return mfx_fail(MFX_E_INVAL, "mfx_phase_copy: null argument");
  if (cap < p->recs.size()) return mfx_fail(MFX_E_INVAL, "mfx_phase_copy: %lu records, room for %lu", (unsigned long)p->recs.size(), (unsigned long)cap);
  if (!p->recs.empty()) memcpy(dst, p->recs.data(), p->recs.size() * sizeof(mfx_phase_block));
  return MFX_OK;
}
extern "C" int mfx_phase_contig_counts(const mfx_phase *p, uint64_t *dst, uint64_t cap) {
  if (!p || (!dst && !p->counts.empty())) return mfx_fail(MFX_E_INVAL, "mfx_phase_contig_counts: null argument");
  if (cap * 4 < p->counts.size())
    return mfx_fail(MFX_E_INVAL, "mfx_phase_contig_counts: %lu contigs, room for %lu", (unsigned long)(p->counts.size() / 4), (unsigned long)cap);
  if (!p->counts.empty()) memcpy(dst, p->counts.data(), p->counts.size() * sizeof(uint64_t));
  return MFX_OK;
}
extern "C" void mfx_phase_free(mfx_phase *p) { delete p; }

namespace {
// blocks, sum / min / mean / max of the base spans, N50, markers, switch markers: host integers
struct SetStats {
  std::vector<uint64_t> spans;
  uint64_t markers = 0, switches = 0;
  void line(FILE *f, const char *name) {
    std::sort(spans.begin(), spans.end(), [](uint64_t x, uint64_t y) { return x > y; });
    uint64_t sum = 0, n50 = 0, run = 0;
    for (uint64_t s : spans) sum += s;
    for (uint64_t s : spans) {                                  // the largest L such that blocks of span >= L hold at least half the sum
      run += s;
      if (2 * run >= sum) { n50 = s; break; }
    }
    const uint64_t n = spans.size();
    fprintf(f, "%s\t%lu\t%lu\t%lu\t%lu\t%lu\t%lu\t%lu\t%lu\t%.6f\n", name, (unsigned long)n, (unsigned long)sum, (unsigned long)(n ? spans.back() : 0),
            (unsigned long)(n ? sum / n : 0), (unsigned long)(n ? spans.front() : 0), (unsigned long)n50, (unsigned long)markers, (unsigned long)switches,
            markers ? (double)switches / (double)markers : 0.0);
  }
};
}  // namespace

extern "C" int mfx_phase_write(const mfx_phase_block *b, uint64_t n, const uint64_t *contig_counts, const mfx_seq *seq, const char *const *names, int k,
                               const mfx_phase_opts *o, const char *stem_in) {
  if (!seq || (!b && n) || (!contig_counts && seq->ncontigs) || !names || !o || !stem_in) return mfx_fail(MFX_E_INVAL, "mfx_phase_write: null argument");
  if (k < 1 || k > MFX_MAX_K) return mfx_fail(MFX_E_INVAL, "mfx_phase_write: k = %d is outside [1, %d]", k, MFX_MAX_K);
  for (uint64_t i = 0; i < n; ++i) {
    const mfx_phase_block &x = b[i];
    if (x.contig >= seq->ncontigs || x.hap > 1 || x.start >= x.end || x.n_hap + x.n_switch == 0 || x.end - 1 + (uint64_t)k > seq->len[x.contig])
      return mfx_fail(MFX_E_INVAL, "mfx_phase_write: record %lu is no block of these sequences (contig %u, haplotype %u, [%lu, %lu), %lu + %lu markers)", (unsigned long)i,
                      x.contig, x.hap, (unsigned long)x.start, (unsigned long)x.end, (unsigned long)x.n_hap, (unsigned long)x.n_switch);
  }
  std::string stem = stem_in, zsuf;                           // out.gz -> out.phased_block.bed.gz
  if (mfx_suffix_tool(stem)) { const size_t dot = stem.rfind('.'); zsuf = stem.substr(dot); stem.resize(dot); }
  const std::string bed = stem + ".phased_block.bed" + zsuf, cnt = stem + ".hapmers.count" + zsuf, sts = stem + ".phased_block.stats" + zsuf;
  {
    mfx_file fh = mfx_open_writer(bed.c_str(), false);
    if (!fh.f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", bed.c_str());
    fprintf(fh.f, "#chrom\tstart\tend\thap\tn_hap\tn_switch\tn_switch_runs\n");
    for (uint64_t i = 0; i < n; ++i)
      fprintf(fh.f, "%s\t%lu\t%lu\t%c\t%lu\t%lu\t%lu\n", names[b[i].contig], (unsigned long)b[i].start, (unsigned long)(b[i].end - 1 + (uint64_t)k), b[i].hap ? 'B' : 'A',
              (unsigned long)b[i].n_hap, (unsigned long)b[i].n_switch, (unsigned long)b[i].n_switch_runs);
    if (mfx_close(fh)) return mfx_fail(MFX_E_IO, "writing '%s' failed (stream error or the compressor exited with an error)", bed.c_str());
  }
  {
    mfx_file fh = mfx_open_writer(cnt.c_str(), false);
    if (!fh.f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", cnt.c_str());
    fprintf(fh.f, "#chrom\tA\tB\tshared\tkmers\n");
    for (uint64_t c = 0; c < seq->ncontigs; ++c)
      fprintf(fh.f, "%s\t%lu\t%lu\t%lu\t%lu\n", names[c], (unsigned long)contig_counts[4 * c + 1], (unsigned long)contig_counts[4 * c + 2],
              (unsigned long)contig_counts[4 * c + 3], (unsigned long)contig_counts[4 * c + 0]);
    if (mfx_close(fh)) return mfx_fail(MFX_E_IO, "writing '%s' failed (stream error or the compressor exited with an error)", cnt.c_str());
  }
  {
    SetStats st[3];
    for (uint64_t i = 0; i < n; ++i)
      for (SetStats *s : {&st[b[i].hap], &st[2]}) {
        s->spans.push_back(b[i].end - 1 + (uint64_t)k - b[i].start);
        s->markers += b[i].n_hap + b[i].n_switch;
        s->switches += b[i].n_switch;
      }
    mfx_file fh = mfx_open_writer(sts.c_str(), false);
    if (!fh.f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", sts.c_str());
    fprintf(fh.f, "#switches\t%lu\trange\t%lu\tk\t%d\n", (unsigned long)o->switches, (unsigned long)o->range, k);
    fprintf(fh.f, "#set\tblocks\tsum\tmin\tmean\tmax\tN50\tmarkers\tswitch_markers\tswitch_rate\n");
    st[0].line(fh.f, "A");
    st[1].line(fh.f, "B");
    st[2].line(fh.f, "all");
    if (mfx_close(fh)) return mfx_fail(MFX_E_IO, "writing '%s' failed (stream error or the compressor exited with an error)", sts.c_str());
  }
  return MFX_OK;
}

extern "C" int mfx_phase_from_planes_host(const uint64_t *planes, const uint64_t *contig_len, uint32_t ncontigs, int k, const mfx_phase_opts *o, mfx_phase_block *out,
                                          uint64_t cap, uint64_t *n_out) {
  if ((!contig_len && ncontigs) || !o || !n_out || (!out && cap)) return mfx_fail(MFX_E_INVAL, "mfx_phase_from_planes_host: null argument");
  if (k < 1 || k > MFX_MAX_K) return mfx_fail(MFX_E_INVAL, "mfx_phase_from_planes_host: k = %d is outside [1, %d]", k, MFX_MAX_K);
  std::vector<uint64_t> tile_start((size_t)ncontigs + 1, 0);
  for (uint32_t c = 0; c < ncontigs; ++c) tile_start[c + 1] = tile_start[c] + (contig_len[c] + MFX_RG_TILE - 1) / MFX_RG_TILE;
  const uint64_t ntiles = tile_start[ncontigs], nw = ntiles * MFX_RG_WORDS;
  if (ntiles && !planes) return mfx_fail(MFX_E_INVAL, "mfx_phase_from_planes_host: null argument");
  std::vector<uint32_t> tile_contig((size_t)ntiles);
  for (uint32_t c = 0; c < ncontigs; ++c) std::fill(tile_contig.begin() + (size_t)tile_start[c], tile_contig.begin() + (size_t)tile_start[c + 1], c);
  for (uint32_t c = 0; c < ncontigs; ++c) {                   // bits beyond a contig's end
    const uint64_t len = contig_len[c], w0 = tile_start[c] * MFX_RG_WORDS, w1 = tile_start[c + 1] * MFX_RG_WORDS;
    for (uint64_t w = w0 + len / 64; w < w1; ++w) {
      const uint64_t beyond = w == w0 + len / 64 ? ~0ull << (len % 64) : ~0ull;
      for (uint32_t h = 0; h < 2; ++h)
        if (planes[h * nw + w] & beyond)
          return mfx_fail(MFX_E_INVAL, "mfx_phase_from_planes_host: haplotype %u flags a position beyond the %lu positions of contig %u", h, (unsigned long)len, c);
    }
  }
  for (uint64_t w = 0; w < nw; ++w)
    if (planes[w] & planes[nw + w])
      return mfx_fail(MFX_E_INVAL, "mfx_phase_from_planes_host: word %lu flags a position in both planes: a k-mer of both sets is shared and no marker", (unsigned long)w);
  std::vector<mfx_phase_block> recs;
  mfx_phase_planes_host(planes, ntiles, tile_start.data(), tile_contig.data(), (uint64_t)k, o->switches, o->range, recs);
  *n_out = recs.size();
  const uint64_t n = std::min<uint64_t>(cap, recs.size());
  if (n) memcpy(out, recs.data(), n * sizeof(mfx_phase_block));
  return MFX_OK;
}
