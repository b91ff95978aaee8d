// mfx_db_trio.cpp -- mfx_db_trio, mfx_db_trio_hist, mfx_db_histogram: the hap-mer sets of a trio and the k-mer histograms their cutoffs are
// read off (include/merfin_amd.h; the rule: mfx_trio.h; the kernels: mfx_trio.hip; the session: mfx_db_windows.h).  Between decode and merge
// every input's k-mers take its role into their two low bits, so that the merged run knows its inputs.  Pass 1 (only where a cutoff is
// automatic, and for the two histogram calls) ends in the image; pass 2 in two compacted outputs, each behind the carry of a streamed writer
// of its own.
#include "mfx_db_windows.h"
#include "mfx_trio.h"
#include "mfx_pipe.h"

#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

namespace { enum TrioKind { TRIO_FULL, TRIO_HIST, TRIO_HISTOGRAM }; }

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
  MergeIns ins;
  if (int rc = db_open_inputs(paths.data(), n_in, who, "the sorted databases of this call hold", "the inputs are of one k", ins)) return rc;
  const int k = (int)ins[0]->h.k;
  if (kind == TRIO_FULL) {
    for (const char *out : {out_a, out_b}) {
      const int same = db_output_is_input(out, ins);
      if (same >= 0) return mfx_fail(MFX_E_INVAL, "mfx_db_trio: the output '%s' is the input '%s'", out, paths[same]);
    }
    struct stat sa, sb;
    if (strcmp(out_a, out_b) == 0 || (stat(out_a, &sa) == 0 && stat(out_b, &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino))
      return mfx_fail(MFX_E_INVAL, "mfx_db_trio: the two outputs '%s' and '%s' are the same file", out_a, out_b);
  }
  MergeWindows P;
  if (int rc = merge_plan_windows(ins, k, who, P)) return rc;
  uint32_t cuts[3] = {o->cut_mat, o->cut_pat, has_child ? o->cut_child : 1u};
  const bool need_hist = kind != TRIO_FULL || cuts[0] == 0 || cuts[1] == 0 || cuts[2] == 0;
  const uint64_t W = (uint64_t)o->max_mult + 1, cells = 3 * W;
  std::vector<uint64_t> image(cells + 1, 0);
  uint64_t dstats[MFX_TRIO_NSTATS] = {0, 0, 0, 0, 0, 0};
  struct { double merge = 0, hist = 0, classify = 0, write = 0; } T;
  DbPass pass(n_in);
  // ---- the device: the buffers of the largest window, for both passes
  std::unique_ptr<DeviceBack> back;
  DbDev own;
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
    // own.p[0], p[1]: two buffers of cap pairs, the k-mers in front of the counts: decoded runs, merge levels, set A behind its writer's carry, and
    // the packed words of the one that is free by then (p[1] only where something is merged or written).  p[2]: the classify's tile offsets (two
    // per tile), then the copies of the stats.  p[3]: set B behind its writer's carry.  p[4]: the image and its counter word.
    const uint64_t small = 2 * (tiles + 1) * 8 + MFX_TRIO_STAT_WORDS * 8;
    const bool two = kind == TRIO_FULL || n_in > 1;
    uint64_t total = 0;
    if (hipError_t e = db_alloc(dec, P, n_in, own, {cap * 12, two ? cap * 12 : 0, small, kind == TRIO_FULL ? cap * 12 : 0, need_hist ? (cells + 1) * 8 : 0}, &total))
      // (a writer's own: the plan and offsets of its blocks, 28 bytes per 4096 k-mers, and what a window escapes)
      return mfx_fail(MFX_E_NOMEM, "%s: the buffers of a window of %lu pairs (%.3f GB: %d of %lu pairs, the second output's among them; the blocks; the block plans "
                      "of both writers) do not fit the device: %s; lower MFX_MERGE_RANGE", who, (unsigned long)P.max_pairs,
                      ((double)total + (kind == TRIO_FULL ? 2.0 * (double)(cap / MFX_DELTA_BLOCK + 1) * (sizeof(mfx_delta_plan) + 12) : 0.0)) / 1e9,
                      kind == TRIO_FULL ? 3 : two ? 2 : 1, (unsigned long)cap, hipGetErrorString(e));
    for (int i = 0; i < 2; ++i) { bk[i] = (uint64_t *)own.p[i]; bv[i] = own.p[i] ? (uint32_t *)((char *)own.p[i] + cap * 8) : nullptr; }
    xk = (uint64_t *)own.p[3]; xv = own.p[3] ? (uint32_t *)((char *)own.p[3] + cap * 8) : nullptr;
    d_tile = (uint64_t *)own.p[2]; d_stats = d_tile + 2 * (tiles + 1); d_img = (uint64_t *)own.p[4];
    MFX_HIP(mfx_memset_now(d_stats, 0, MFX_TRIO_STAT_WORDS * 8));
    if (d_img) MFX_HIP(mfx_memset_now(d_img, 0, (cells + 1) * 8));
    if (int rc = db_grid(o->device, 4, &grid)) return rc;        // 32 KB of LDS bins per workgroup: four workgroups of four waves per CU
    sa = db_spectrum_args(1, o->max_mult, mfx_spec_lds_cols(1, o->max_mult), d_img);      // an image of copies + 2 = 3 rows
  }
  const bool timing = getenv("MFX_DB_TIMING") != nullptr;
  // one pass over the windows: decode, tag, merge, then the histogram (classify == false) or the two sets behind their writers
  auto run_pass = [&](bool classify) -> int {
    const mfx_trio_cuts tc{cuts[0], cuts[1], cuts[2], has_child};
    if (int rc = db_each_window(ins, P, k, who, dec, bk[0], bv[0], pass, [&](std::vector<MergeRun> &runs) -> int {
      double t0 = db_now(), t1;
      for (uint32_t i = 0; i < n_in; ++i)                        // the role into the key's two low bits (mfx_trio.h)
        MFX_HIP(mfx_k_trio_tag(bk[0] + runs[i].off, runs[i].len, roles[i], nullptr));
      int cur = 0;
      if (int rc = merge_tree(runs, bk, bv, cur)) return rc;
      if (timing) MFX_HIP(hipStreamSynchronize(nullptr));
      t1 = db_now();
      T.merge += t1 - t0;
      const uint64_t M = runs[0].len;
      if (!classify) {
        MFX_HIP(mfx_k_trio_hist(bk[cur] + runs[0].off, bv[cur] + runs[0].off, M, sa, grid, nullptr));
        if (timing) MFX_HIP(hipStreamSynchronize(nullptr));
        T.hist += db_now() - t1;
        return MFX_OK;
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
      return MFX_OK;
    })) return rc;
    return pass.check(ins);
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
    st->n_a = n_a; st->n_b = n_b; st->windows = pass.windows;
    if (kind == TRIO_FULL) {
      st->cut_mat = cuts[0]; st->cut_pat = cuts[1]; st->cut_child = has_child ? cuts[2] : 0;
      st->auto_mat = autos[0]; st->auto_pat = autos[1]; st->auto_child = has_child ? autos[2] : 0;
    }
    st->hist_pass = need_hist ? 1u : 0u;
    st->t_read = pass.t_read; st->t_decode = pass.t_decode; st->t_merge = T.merge; st->t_hist = T.hist; st->t_classify = T.classify; st->t_write = T.write;
    st->t_close = t_close; st->t_total = db_now() - t_begin;
  }
  return MFX_OK;
}

extern "C" int mfx_db_trio(const char *mat_path, const char *pat_path, const char *child_path, const char *out_a, const char *out_b, const mfx_db_trio_opts *o, uint64_t *img,
                           mfx_db_trio_stats *st) {
  return db_guard("mfx_db_trio", [&] { return trio_impl(TRIO_FULL, mat_path, pat_path, child_path, out_a, out_b, o, img, st); });
}

extern "C" int mfx_db_trio_hist(const char *mat_path, const char *pat_path, const char *child_path, uint32_t max_mult, uint64_t *img, mfx_db_trio_stats *st, int device) {
  const mfx_db_trio_opts o{0, 0, 0, max_mult, device};
  return db_guard("mfx_db_trio_hist", [&] { return trio_impl(TRIO_HIST, mat_path, pat_path, child_path, nullptr, nullptr, &o, img, st); });
}

extern "C" int mfx_db_histogram(const char *path, uint32_t max_mult, uint64_t *row, uint64_t *n_kmers, int device) {
  const mfx_db_trio_opts o{0, 0, 0, max_mult, device};
  mfx_db_trio_stats st;
  if (n_kmers) *n_kmers = 0;
  const int rc = db_guard("mfx_db_histogram", [&] { return trio_impl(TRIO_HISTOGRAM, nullptr, nullptr, path, nullptr, nullptr, &o, row, &st); });
  if (rc == MFX_OK && n_kmers) *n_kmers = st.n_child;
  return rc;
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
  return db_guard("mfx_db_trio_host", [&]() -> int {
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
  });
}
